/*
 * usvmpc.h — C ABI of the MI355X batched SQP-RTI solver (libusvmpc.so).
 *
 * Drop-in boundary: this is what a binding would call instead of the generated acados solver of
 * the reference.  Reference interfaces replaced (paths relative to /root/reference):
 *
 *   Python (acados_template.AcadosOcpSolver, used by the closed-loop scripts):
 *     AcadosOcpSolver(ocp, json_file=...)     catkin_ws/src/nmpc_ca/scripts/usv_guidance_ca1/acados_settings.py:207
 *                                             -> usvmpc_create
 *     solver.set(stage, "lbx"/"ubx", x0)      .../usv_guidance_ca1/main.py:111-112,174-175 -> usvmpc_set("x0")
 *     solver.set(stage, "yref", v)            .../usv_guidance_ca1/main.py:125,129         -> usvmpc_set("yref")
 *     solver.set(stage, "p", v)               .../usv_guidance_ca1/main.py:126,130         -> usvmpc_set("p")
 *     solver.constraints_set(stage, "lh", v)  .../usv_guidance_ca1/main.py:127             -> usvmpc_set("lh")
 *     solver.solve()                          .../usv_guidance_ca1/main.py:135             -> usvmpc_solve
 *     solver.get(stage, "x"|"u")              .../usv_guidance_ca1/main.py:147-148,169     -> usvmpc_get
 *   C (generated acados_solver_<model>.h + libacados, used by the ROS nodes):
 *     acados_create / acados_free             catkin_ws/src/nmpc_ca/src/nmpc_guidance_ca1.cpp:165,220 -> usvmpc_create / usvmpc_destroy
 *     ocp_nlp_constraints_model_set(lbx/ubx/lh) .../nmpc_guidance_ca1.cpp:515-516,571     -> usvmpc_set
 *     ocp_nlp_cost_model_set(yref)            .../nmpc_guidance_ca1.cpp:569,573            -> usvmpc_set
 *     acados_update_params(stage, p, np)      .../nmpc_guidance_ca1.cpp:570,574            -> usvmpc_set("p")
 *     acados_solve()                          .../nmpc_guidance_ca1.cpp:577                -> usvmpc_solve
 *     ocp_nlp_out_get(stage, "x"|"u")         .../nmpc_guidance_ca1.cpp:583,586            -> usvmpc_get
 *
 * One handle = one OCP definition x a batch of B independent instances on one HIP device.
 * All arrays are FP64, instance-major: element (b, stage, i) of a per-stage field of length n is
 * at [(b * n_stages + stage) * n + i].  The caller owns every host array; the library copies on
 * set and fills caller memory on get.  Return value 0 = ok; solver outcomes reuse acados'
 * status values (0 ok, 4 QP failure); negative values are API errors (usvmpc_last_error).
 * A handle is single-caller; distinct handles are independent.  Nothing here falls back to the
 * CPU: without a HIP device usvmpc_create fails.
 */
#ifndef USVMPC_H
#define USVMPC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define USVMPC_NX_MAX 14
#define USVMPC_NU_MAX 2
#define USVMPC_NY_MAX 16
#define USVMPC_K_MAX 32

enum { USVMPC_MODEL_USV = 0,             /* `usv_model`              nx 5  nu 2           */
       USVMPC_MODEL_GUIDANCE_CA1 = 1,    /* `usv_model_guidance_ca1` nx 8  nu 1, soft h   */
       USVMPC_MODEL_PF_CA = 2,           /* `usv_model_pf_ca`        nx 14 nu 2, hard h   */
       USVMPC_MODEL_GENERATED = 3 };     /* model compiled into THIS library from a symbolic definition
                                            (mpc_collisionavoidance_amd/codegen.py); only in libraries built for it */

/* The QP solver's argument profile.  The reference selects HPIPM through acados (qp_solver = "PARTIAL_CONDENSING_HPIPM":
 * catkin_ws/src/nmpc_ca/scripts/usv_pf_ca/acados_settings.py:172, usv_guidance_ca1/acados_settings.py:190) and leaves every knob at its default
 * (the tolerances are there, commented: :183-186 / :198-204), i.e. at what acados' ocp_qp_hpipm_opts_initialize_default produces: one of HPIPM's
 * modes (d_ocp_qp_ipm_arg_set_default) plus acados' own overwrites.  Neither source tree is in /root/reference; DESIGN.md section 2 lists every
 * field as recalled.  The modes differ, for this library, in nothing the kernels do (iterative refinement and the LQ fall-back are the checker's
 * business: oracle/usv_oracle.h); they are kept apart so that a binding can pass acados' `hpipm_mode` through:
 *   BALANCE / SPEED / ROBUST  cond_pred_corr = 1 (HPIPM, every mode), mu0 = 1, alpha_min = 1e-8, tolerances 1e-6 / 1e-8 / 1e-8 / 1e-8,
 *                             iter_max = 50 (acados' overwrites of the mode's values)
 *   R04                       this library's behaviour up to its round 5: cond_pred_corr = 0, mu0 = 10, alpha_min = 1e-12 (HPIPM's own
 *                             mode values without acados' overwrites) - kept reachable for comparison */
enum { USVMPC_HPIPM_BALANCE = 0, USVMPC_HPIPM_SPEED = 1, USVMPC_HPIPM_ROBUST = 2, USVMPC_HPIPM_R04 = 3 };

enum { USVMPC_E_ARG = -1, USVMPC_E_FIELD = -2, USVMPC_E_STAGE = -3, USVMPC_E_SIZE = -4,
       USVMPC_E_HIP = -5, USVMPC_E_NODEVICE = -6 };

/* The OCP definition (what AcadosOcp carries).  Dense row-major matrices with the model's
 * actual dimensions: W ny x ny, W_e nx x nx, Vx ny x nx, Vu ny x nu, Vx_e nx x nx. */
typedef struct usvmpc_desc {
    int model;
    int N;                 /* shooting intervals, >= 2 (the reference's OCPs: 20 .. 100); usvmpc_create refuses less */
    double Tf;
    int K;                 /* circular obstacles: nh = K, np = 2K */
    int batch;
    int device;            /* HIP device ordinal */
    double W[USVMPC_NY_MAX * USVMPC_NY_MAX];
    double W_e[USVMPC_NX_MAX * USVMPC_NX_MAX];
    double Vx[USVMPC_NY_MAX * USVMPC_NX_MAX];
    double Vu[USVMPC_NY_MAX * USVMPC_NU_MAX];
    double Vx_e[USVMPC_NX_MAX * USVMPC_NX_MAX];
    int nbu; int idxbu[USVMPC_NU_MAX]; double lbu[USVMPC_NU_MAX], ubu[USVMPC_NU_MAX];
    int nbx; int idxbx[USVMPC_NX_MAX]; double lbx[USVMPC_NX_MAX], ubx[USVMPC_NX_MAX];
    double uh[USVMPC_K_MAX];
    int soft;              /* 1: all h rows soft (idxsh = 0..K-1) */
    double lsh[USVMPC_K_MAX], ush[USVMPC_K_MAX];
    double zl[USVMPC_K_MAX], zu[USVMPC_K_MAX], Zl[USVMPC_K_MAX], Zu[USVMPC_K_MAX];
    int qp_iter_max;
    double mu0, thr0, tol_stat, tol_eq, tol_ineq, tol_comp, alpha_min;
    /* soft state bounds (acados idxsbx / lsbx / usbx, scripts/race_cars/acados_settings_dev.py:107-127), per entry of
     * the bx list: flag, lower bounds of the two slacks, slack penalties (acados keeps the penalties of all slacks in
     * one vector ordered [sbx.., sh..]; zl.. above are the sh part, these the sbx part) */
    int sbx[USVMPC_NX_MAX];
    double lsbx[USVMPC_NX_MAX], usbx[USVMPC_NX_MAX];
    double zl_bx[USVMPC_NX_MAX], zu_bx[USVMPC_NX_MAX], Zl_bx[USVMPC_NX_MAX], Zu_bx[USVMPC_NX_MAX];
    /* integrator: RK4 steps per shooting interval (acados sim_method_num_steps; 0 is read as 1) */
    int sim_num_steps;
    /* full SQP only (usvmpc_solve_sqp): nlp_solver_max_iter (0 is read as 100) and the exit tolerances on
     * the NLP residuals stat / eq / ineq / comp (0 is read as 1e-6, the acados default) */
    int nlp_max_iter;
    double nlp_tol_stat, nlp_tol_eq, nlp_tol_ineq, nlp_tol_comp;
    /* QP solver profile (USVMPC_HPIPM_*; usvmpc_hpipm_profile fills the fields it governs: mu0, alpha_min, the tolerances, qp_iter_max and the
     * two below) and HPIPM's conditional predictor-corrector: 1 = a corrected step that leaves the duality measure above cpc_factor (0 is read
     * as 2) x the predictor's mu_aff is redone with the centring-only step */
    int hpipm_mode;
    int cond_pred_corr;
    double cpc_factor;
} usvmpc_desc;

typedef struct usvmpc_handle usvmpc_handle;

/* nx, nu of a model id; returns 0 or USVMPC_E_ARG */
int usvmpc_model_dims(int model, int *nx, int *nu);
/* solver option defaults: thr0 0.1, one RK4 step per interval, the NLP tolerances, and the QP solver profile USVMPC_HPIPM_BALANCE
 * (iter_max 50, mu0 1, tolerances 1e-6/1e-8, alpha_min 1e-8, cond_pred_corr 1) */
void usvmpc_default_options(usvmpc_desc *d);
/* the fields of d that the QP solver profile `mode` governs (above); returns 0 or USVMPC_E_ARG */
int usvmpc_hpipm_profile(usvmpc_desc *d, int mode);

int usvmpc_create(const usvmpc_desc *d, usvmpc_handle **out);
int usvmpc_destroy(usvmpc_handle *h);

/* fields: "x0" (n = nx), "yref" (stage 0..N-1: n = ny; stage N: n = nx), "p" (stage 0..N,
 * n = 2K), "lh" (stage 0..N-1, n = K), "x" (stage 0..N, n = nx), "u" (stage 0..N-1, n = nu).
 * v holds [batch][n] for one stage, or, with stage = -1, [batch][n_stages][n] for all stages
 * ("yref" with stage -1 covers stages 0..N-1 only). */
int usvmpc_set(usvmpc_handle *h, const char *field, int stage, const double *v, size_t n);
/* fields: "x", "u", "pi" (stage 1..N), "sl", "su" (stage 0..N-1, n = K), "res" (stage ignored,
 * n = 4: QP residuals stat/eq/ineq/comp), "nlp_res" (the same for the NLP, full SQP only); same stage = -1
 * convention. */
int usvmpc_get(usvmpc_handle *h, const char *field, int stage, double *out, size_t n);
/* "lam" / "t" (stage 0..N, n = 2 (nrow + ns)): the inequality multipliers and slacks of the last QP, what acados'
 * ocp_nlp_out_get(.., stage, "lam" | "t") returns: rows of a stage in acados' order [bu.., bx.., h..] (nrow = nbu + nbx + K),
 * slack rows [sbx.., sh..] (ns = soft state bounds + K when the h rows are soft); the vector is
 * [lower (nrow) | upper (nrow) | lower-slack bound (ns) | upper-slack bound (ns)].  Rows a stage does not have (state bounds
 * and h rows at stage 0 - x0 is eliminated -, everything at stage N) read 0.  Gathered from the solver workspace by a kernel
 * of its own on the first such get after a solve. */
/* further get fields: "obs_tmin" (stage ignored, n = 1): the smallest lower-side slack t_l over the instance's obstacle rows
 * in the last QP (1e300 without rows) - below ~1e-3 the solution touches a keep-out circle, i.e. an obstacle row is active */
/* ---- Obstacle tracks: a position (ox, oy) and a constant velocity (vx, vy) per instance and obstacle slot, kept on the device, from which the
 * handle derives p itself - a closed loop against MOVING obstacles without rebuilding and uploading [B][N+1][2K] doubles every tick.
 *   set / get "obs_pos", "obs_vel": [batch][2K], pairs per obstacle in slot order, laid out like one stage of "p"; the stage argument is
 *       ignored (as for "x0").  The device buffers are made by the first set of either field (a handle that never uses tracks pays nothing);
 *       "obs_vel" defaults to 0.  USVMPC_E_FIELD for a model without obstacle rows (K = 0).  usvmpc_get_device_ptr serves both (a caller
 *       that holds such a pointer may move the obstacles with kernels of its own: the prediction then runs before every solve).  The
 *       keep-out radii stay where they are: "lh".
 *   option "obstacle_tracks" = 1 (after "obs_pos" was set; default 0): every usvmpc_solve / _solve_async / _solve_sqp first writes
 *           p[b][k][2i + c] = obs_pos[b][2i + c] + ((double)k * dt) * obs_vel[b][2i + c]      k = 0 .. N,  dt = Tf / N
 *       on the handle's stream (kernel usv_obstacle_predict; product and sum rounded separately, no fused multiply-add: the bits numpy makes
 *       from the same expression), behind the upload of pending host writes and ahead of every kernel that reads p; skipped while neither
 *       the tracks nor the world clock changed.  With "static_obstacles" = 1 only stage 0 is written (a world that moves between ticks and is
 *       held still inside the horizon).  While the option is on usvmpc_set "p" is refused (USVMPC_E_ARG) and usvmpc_get "p" returns what the
 *       device holds; switched off, p is the caller's again, as it stands.  The lineariser does not read p: linearisations made ahead of
 *       time (option "pipeline_linearize") stay valid.
 *   usvmpc_obstacles_step(h, T): the world moves on, obs_pos += T * obs_vel (unfused), then per instance
 *           clearance = min over slots i of  sqrt((X - ox_i)^2 + (Y - oy_i)^2) - lh[b][0][i]
 *       with (X, Y) the position states of x0 (the states the model's obstacle rows read); enqueued on the handle's stream (kernel
 *       usv_obstacle_step).  While the option is on usvmpc_advance calls it with T = dt and usvmpc_advance_sim with the plant's period, behind
 *       their own kernel - one call is still the tick's hand-over; option "obstacle_step_on_advance" = 0 (default 1) leaves the world to the
 *       caller (a tracker that sets "obs_pos" every tick).
 *   get "clearance" [batch] (n = 1): the value after the last world step; "clearance_min": its running minimum since the caller last set
 *       "obs_pos" (which resets it to 1e300).  Parked slots ((1000, 1000), lh 0) need no special case. */
int usvmpc_obstacles_step(usvmpc_handle *h, double T);
/* integer per-instance results: "status" (0 | 4; after usvmpc_solve_sqp 0 | 2 | 4), "qp_status" (0 ok,
 * 1 max iter, 2 min step, 3 nan, 4 x0 violates a hard obstacle row of stage 0 - the QP has no feasible point), "qp_iter", "sqp_iter" */
int usvmpc_get_int(usvmpc_handle *h, const char *field, int *out);

/* One SQP-RTI iteration for every instance; returns the worst status. status may be NULL. */
int usvmpc_solve(usvmpc_handle *h, int *status);
/* Full SQP (acados nlp_solver_type "SQP": the option the reference's settings files mention but leave
 * commented, scripts/usv_guidance_ca1/acados_settings.py:192-204; used by scripts/race_cars/
 * acados_settings_dev.py:157): per instance, linearise - test the NLP residuals - solve the QP - full step,
 * until the residuals are below the tolerances (status 0), nlp_max_iter QPs have been solved (2) or a QP
 * fails (4).  Converged instances are frozen while the rest of the batch continues.  The multipliers of
 * the last QP are kept between calls, so a call from a converged point returns after 0 iterations.  Afterwards
 * usvmpc_get_int "sqp_iter" and usvmpc_get "nlp_res" (n = 4) describe the run. */
int usvmpc_solve_sqp(usvmpc_handle *h, int *status);
/* Enqueue one RTI iteration on the handle's stream without synchronising or reading back */
int usvmpc_solve_async(usvmpc_handle *h);
int usvmpc_sync(usvmpc_handle *h);

/* device pointer of a field ("x","u","x0","yref","yref_e","p","lh","pi","sl","su","status",
 * "qp_iter","res") for zero-copy use from torch / RCCL */
int usvmpc_get_device_ptr(usvmpc_handle *h, const char *field, void **dptr);
/* HIP-event durations (ms) of the two kernels of the most recent solve / of the last n solves
 * (oldest first, n <= 64), measured on the stream the kernels were launched on */
int usvmpc_last_kernel_ms(usvmpc_handle *h, float *linearize_ms, float *qp_ms);
int usvmpc_kernel_ms(usvmpc_handle *h, int n, float *linearize_ms, float *qp_ms);
/* tick-to-tick times (ms) over the last n solves: ms[i] = start of solve i + 1 minus start of solve i on the handle's stream (n - 1 values,
 * oldest first, 2 <= n <= 64) - everything a closed-loop step enqueued in between (QP launch, hand-over, the caller's own kernels) included;
 * what bench.py reports the median of ("report median") */
int usvmpc_tick_ms(usvmpc_handle *h, int n, float *ms);
/* number of instances whose solve ended with status != 0, for each of the last n solves (oldest first, n <= 64); counted on
 * the device by the solve itself, so a closed loop can be audited without a read-back per tick */
int usvmpc_fail_counts(usvmpc_handle *h, int n, int *counts);
/* ... and the number whose QP did not converge to the IPM tolerances (qp_status != 0: iteration cap, step-length floor, NaN, x0 inside
 * a hard keep-out circle), per solve likewise: solves minus this = "solves" as SURVEY.md 8(d) counts them (IPM converged to the stated
 * tolerance).  RTI solves (usvmpc_solve / usvmpc_solve_async); counted by a small kernel behind the QP launch. */
int usvmpc_unconverged_counts(usvmpc_handle *h, int n, int *counts);
/* ... and their sum over every RTI solve since the handle was created (a device-side running sum: no limit of 64 solves) */
int usvmpc_unconverged_total(usvmpc_handle *h, long long *total);
/* option "handover_iter": how many instances each of the last n RTI launches handed over to its follow-up launch (oldest first, n <= 64) */
int usvmpc_handover_counts(usvmpc_handle *h, int n, int *counts);
/* ... and how long that follow-up launch (kernel usv_qp_resume) took, in ms, for each of the last n solves - part of usvmpc_kernel_ms' qp_ms;
 * 0 for a solve without one */
int usvmpc_followup_ms(usvmpc_handle *h, int n, float *ms);
/* option "handover_co": of those, how many the follow-up kernel running BESIDE the launch (usv_qp_resume_co) finished, and how many of its
 * waits for a list entry ran into the spin limit (left to the follow-up launch behind the main one; timeouts may be NULL) */
int usvmpc_handover_co_counts(usvmpc_handle *h, int n, int *finished, int *timeouts);
/* option "pipeline_linearize": how many linearisations made ahead of time (on the second stream, beside the previous tick's QP launch)
 * were used by the following solve / discarded because the caller wrote x, u or yref in between.  The lineariser only runs ahead after
 * two solves in a row without such a write, so a caller that sets yref every tick (the reference's protocol) discards none. */
int usvmpc_pipeline_stats(usvmpc_handle *h, long *used, long *discarded);
/* option "lin_pairs": how many lineariser launches of the handle so far ran the kernels that serve two (instance, stage) pairs per row */
int usvmpc_lin_pair_launches(usvmpc_handle *h, long *launches);
/* Which mapping the last solve (RTI, or the last launch of a full SQP) ran on: 0 = four instances per wavefront (one per 16-lane row: the throughput mapping), 1 = ONE
 * instance per wavefront (option "wide": the latency mapping north_star names - the four rows of the wave share out the stage-local
 * constraint-row work of four consecutive stages), 4 = one instance per workgroup of FOUR wavefronts (option "wide_waves": a whole CU
 * shares out the row work of 16 consecutive stages; default for soft-row OCPs in batches of at most one instance per CU).  The latency
 * mapping is taken by default for batches that leave SIMDs idle (RTI solves and the launches of a full SQP; every layout with a diagonal
 * Hessian - i.e. every OCP of the reference: up to 32 obstacle rows, soft state bounds); the planes live in the CU's LDS when the horizon
 * fits, else - and for a full SQP - in HBM.
 * WHICH mapping ran does not show in the results: all of them take every sum in the same order and contract multiply-adds the same way
 * (qp_ipm.hpp: #pragma clang fp contract(on)), so statuses, iteration counts, iterates and multipliers are the same BITS - an instance
 * solved in a handle of 1, of 512 or of 65 536 returns the same answer (tests/test_gpu_wide.py, test_gpu_closed_loop.py::
 * test_shards_that_land_on_the_other_mapping_equal_the_unsharded_batch).  The reference solves one instance per call:
 * nmpc_guidance_ca1.cpp:577,612, usv_pf_ca/main.py:142-186. */
int usvmpc_last_mapping(usvmpc_handle *h, int *mapping);
/* Closed-loop hand-over on the device: x0 <- x_1 (+ sigma * N(0,1) on the states selected by option
 * "disturbance_mask", default all; the draw of state j of instance b is keyed by (option "instance_offset" + b) * nx + j), enqueued on
 * the stream.  A plant other than the model's own prediction: usvmpc_advance_sim below.
 * Replaces x0 = solver.get(1,"x"); solver.set(0,"lbx",x0); solver.set(0,"ubx",x0)
 * (catkin_ws/src/nmpc_ca/scripts/usv_guidance_ca1/main.py:169-175). */
int usvmpc_advance(usvmpc_handle *h, double sigma, unsigned long long seed);
/* Adopt a caller-owned HIP stream (e.g. torch's current stream) for all subsequent work */
int usvmpc_set_stream(usvmpc_handle *h, void *stream);
/* run-time options (scheduling / placement only: results are the same bits whatever they are set to - except "merge_box_rows", which
 * changes rounding, and "qp_cond_N", which selects another formulation of the same QP):
 *   "qp_cond_N" (default 0) - acados' qp_solver_cond_N (qp_solver = PARTIAL_CONDENSING_HPIPM:
 *       catkin_ws/src/nmpc_ca/scripts/usv_pf_ca/acados_settings.py:172; the reference never sets it, i.e. blocks of one stage = the
 *       default here).  A value N2 < N makes every RTI solve condense its QP to N2 dense stages first (HPIPM d_part_cond_qp:
 *       states of N / N2 consecutive stages - one more in the first N mod N2 blocks - eliminated through the dynamics;
 *       nx + ceil(N / N2) nu <= 64), solve THAT QP with the same
 *       interior-point method and expand the solution (x, u, pi) - a kernel of its own (csrc/cond_ipm.hpp: one instance per
 *       workgroup, the block's matrices in LDS).  Obstacle rows hard or soft; E_ARG for soft state bounds; "lam" / "t" only when
 *       their buffers exist before the solve (option "keep_multipliers"); usvmpc_solve_sqp keeps solving the uncondensed stages.  Same solution as the default path up to the IPM exit
 *       tolerances; which of the two is faster is measured in DESIGN.md section 6.  0 or N: off;
 *   "sort_by_difficulty" (default 1) - instances are handed to the wavefront rows in the order of their IPM iteration counts of
 *       the previous solve, hardest first (an instance that runs long must not start late); "sort_two_ticks" = 1 (default 0)
 *       orders by the larger of the last two solves' counts instead;
 *   "static_obstacles" (default 0) - every stage uses stage 0's p and lh (what the reference's callers set:
 *       scripts/usv_pf_ca/main.py puts one obstacle set on all stages), which the kernel then keeps in registers;
 *   "pack_box_rows" (default 1 when the rows fit) - box-row multipliers share the obstacle rows' planes;
 *   "dynamic_rows" (default 1) - an RTI solve is one persistent launch whose wavefront rows pull instances from a device
 *       queue as their QPs converge (0: every row keeps its first instance and idles until its wave is done);
 *   "lds_workspace" (default -1) - per-stage planes of the QP in the CU's LDS instead of HBM: -1 when one round of
 *       workgroups covers the batch (an instance's whole horizon must fit in 160 KB), 0 never, 1 whenever it fits.  The same
 *       bits as the HBM placement (a separately compiled instantiation of the same code, contracted the same way);
 *   "merge_box_rows" (default 1) - when every box row rides in an idle lane of the last obstacle chunk's planes the sweeps
 *       process them there (one row pass instead of two).  THE option that changes rounding: a row's share of the complementarity
 *       sums is added in another lane, so statuses and iteration counts are equal and iterates agree to rounding, not to the bit;
 *       a handle keeps one setting for its lifetime unless the caller changes it;
 *   "wide_waves" (default -1) - wavefronts per instance of the latency mapping: -1 four for OCPs with soft obstacle rows or two obstacle
 *       chunks (K > 16) while the batch is at most one instance per CU - two from N = 40 - (their row work is the larger share: 6 - 25 % per
 *       tick), one otherwise; 1; 4 (built for the packed row layouts and the one without obstacle rows; the others stay at one);
 *   "wide" (default -1) - the latency mapping, ONE instance per wavefront (usvmpc_last_mapping): -1 while the batch fits the device's
 *       SIMDs twice over, 0 never, 1 whenever the OCP's layout allows it; results do not change by a bit;
 *   "aux_in_lds" (default 1) - an RTI solve keeps the per-stage aux plane (dense box rows, linearisation point, r_g, l_u) in the
 *       wavefronts' LDS instead of streaming it, when the horizon fits without costing a resident wavefront (a separately
 *       compiled instantiation of the same arithmetic: the same bits);
 *   "pipeline_linearize" (default 1; RTI solves of handles with >= 16384 instances) - the lineariser of the NEXT tick is enqueued on a
 *       second stream behind the QP launch and runs in that launch's tail, instance by instance as results become final (the
 *       few it has to skip are redone in front of the next QP launch); any usvmpc_set, option change or device-pointer access in
 *       between makes the next solve linearise afresh.  The queue order of a tick is then made one tick earlier.  Scheduling
 *       only: results are bit-identical to the un-pipelined sequence;
 *   "lin_force_modes" (default 0; for tests) - 1 / 2: an RTI solve that would run the whole-batch lineariser runs the pipeline's two kernels
 *       in its place, the speculative one with every instance taken as final (1) or none (2: the fix-up pass then does all the work).  The
 *       same bits as 0;
 *   "lin_pairs" (default 1 for usv_model and usv_model_pf_ca, 0 for usv_model_guidance_ca1 and a generated model) - 1: the lineariser's kernels that serve two (instance,
 *       stage) pairs per 16-lane row (for models that declare the at most eight sensitivity columns to integrate); 0: one pair per row.  The
 *       same bits either way; 1 on a model without the declaration is an error;
 *   "host_mirror" (default: on for handles whose caller-visible arrays total <= 1 MiB, i.e. the single-instance drop-in faces) -
 *       usvmpc_set writes a pinned host mirror and the next solve uploads the dirty fields in one asynchronous copy instead
 *       (ordering: a set becomes visible on the device with the NEXT launch of the handle, not at the call - except once a device pointer
 *       has been handed out (usvmpc_get_device_ptr): from then on stage-wise sets are enqueued on the handle's stream at the call, so that a
 *       caller's own kernels on that stream see them in program order)
 *       of one synchronising copy per call (the reference issues 3N+4 setters per tick: scripts/usv_guidance_ca1/main.py:
 *       123-130, src/nmpc_guidance_ca1.cpp:567-574); x / u / status come back in one copy and usvmpc_get "x" / "u" is served
 *       from it.  0 switches it off for the handle (it cannot be switched on again);
 *   "hpipm_mode" (USVMPC_HPIPM_*; default: the descriptor's) - re-applies a QP solver profile to the handle: mu0, alpha_min and cond_pred_corr
 *       as the profile says (tolerances and iter_max are the same in every profile and keep the descriptor's values);
 *   "cond_pred_corr" (default: the descriptor's, 1 in every profile but R04), "cpc_factor" (default 2) - HPIPM's conditional predictor-corrector,
 *       an option of the QP solver the reference selects (qp_solver = PARTIAL_CONDENSING_HPIPM: catkin_ws/src/nmpc_ca/scripts/usv_pf_ca/
 *       acados_settings.py:172) that every mode acados can pick switches on (DESIGN.md section 2 lists every HPIPM argument, adopted or not): an
 *       IPM iteration whose corrected step leaves the duality measure above cpc_factor x the predictor's is redone with the centring-only step.
 *       THE option that changes results beyond rounding (another iteration path to the same tolerance).  The test is built into every kernel -
 *       every mapping, the follow-up launch of the hand-over, the launches of a full SQP, the partially condensed solve; switched off, the same
 *       kernels return the bits of kernels without it;
 *   "handover_iter" (default -1) - RTI launches on the throughput mapping: once every instance of the launch has been handed out, a row
 *       whose instance has passed this many IPM iterations leaves it to a follow-up launch on the latency mapping (kernel usv_qp_resume: one
 *       instance per wavefront, the suspended solve's planes copied into LDS first), which finishes it at half the time per iteration of a lone
 *       16-lane row - a launch ends with its 30 - 50 iteration instances on an otherwise idle device.  Scheduling only: the mappings return the
 *       same bits.  -1: past 20 iterations where the horizon's planes fit a CU's LDS AND the batch is at most three times what the device holds at
 *       once (re-measured under the default QP solver profile, whose solves are shorter: with "handover_co" -18 % per tick at 4 096 instances,
 *       -13 % at 8 192, -4 % at 16 384, nothing from 32 768 up), never otherwise; 0: never; n > 0: past n, whatever the batch.  Layouts: one
 *       obstacle chunk / no obstacle rows, packed box rows, no soft state bounds;
 *   "handover_lds" (default 1) - 0: the follow-up launch works over the planes in HBM whatever the horizon (measured: a loss);
 *   "handover_co" (default -1 = on where the follow-up works in LDS and the handle owns its stream; 0: off) - the follow-up kernel also runs
 *       BESIDE the draining launch (kernel usv_qp_resume_co on a stream of its own): its workgroups come onto the device as wavefronts of the
 *       main launch leave, wait - a bounded wait, "handover_co_spin" polls - for list entries to appear and finish those instances while the
 *       main launch is still draining; what they do not get to is done by the launch behind it (every entry is taken by exactly one of the
 *       two).  Scheduling only.  "handover_co_wgs": workgroups of that kernel (0 = one per CU: what finds room beside the main launch's workgroups at once);
 *   "disturbance_mask" (default all ones) - bit j set: usvmpc_advance / usvmpc_advance_sim add their noise to state j (the reference's
 *       commented hooks disturb x0[3] and x0[5] only: catkin_ws/src/nmpc_ca/scripts/usv_pf_ca/main.py:181-183);
 *   "instance_offset" (default 0) - the global index of the handle's first instance.  The disturbance of state j of instance b is drawn
 *       from the key (instance_offset + b) * nx + j, so a batch split over several handles (shards: set each handle's offset to the
 *       index of its first instance) draws the same noise as one handle over the whole batch.  0 leaves the draws as they were;
 *   "obstacle_tracks" (default 0), "obstacle_step_on_advance" (default 1) - p derived from the obstacle tracks, the world stepped by the
 *       hand-over: "Obstacle tracks" above;
 *   "pf_predict" (default 1), "pf_lh_margin" (default 0.2; finite, >= 0) - the path-following front end's moving world predicted per stage
 *       or held still inside the horizon, and the margin it adds to every keep-out radius: "Path-following front end" below;
 *   "keep_multipliers" (an action, no state) - a value != 0 creates the buffers behind usvmpc_get "lam" / "t" now instead of at the first
 *       get (a partially condensed solve fills them only if they exist before it);
 *   "max_waves" (default 0) - 0: as many persistent wavefronts of the QP kernel as the device holds; n > 0 caps them, and the teams of a
 *       partially condensed solve (a measurement aid; a negative value behaves as 0).
 * A refused value (USVMPC_E_ARG, usvmpc_last_error names the option) or an unknown name (USVMPC_E_FIELD) changes nothing.  Options kept
 * as integers ("max_waves", "disturbance_mask", "qp_cond_N", "hpipm_mode", "instance_offset", "handover_iter", "handover_co_spin",
 * "handover_co_wgs") refuse a NaN and a value their type does not hold. */
int usvmpc_set_option(usvmpc_handle *h, const char *name, double value);
/* ---- Guidance front end (model usv_model_guidance_ca1 only): the arithmetic either side of the solver
 * call in the reference's ROS node, batched on the device (class NMPC in
 * catkin_ws/src/nmpc_ca/src/nmpc_guidance_ca1.cpp).  Per-instance state (waypoint index k, past_psied) lives in
 * the handle.  Arrays are host pointers, instance-major.
 *   reset   = main(), new waypoint list                        :616-632  (waypoints [B][2*npts], psi [B])
 *   prepare = velocityCallback / obstaclesCallback / body2NED / waypoint_manager / control (input part)
 *                                                               :223-230,252-376,441-574
 *             vel_uv [B][2], pose [B][3] = (nedx, nedy, psi), obstacles [B][lmax][3] = body (x, y, R),
 *             n_obstacles [B], lmax <= 64; writes x0 and the (stage-independent) p / lh of the solver and switches
 *             the solver to static obstacles; asynchronous on the handle's stream
 *   publish = control (output part)                             :583-600  desired heading / r / speed, ye
 * The "static_obstacles" option (usvmpc_set_option) makes every stage use stage 0's p and lh. */
int usvmpc_guidance_reset(usvmpc_handle *h, const double *waypoints, int npts, const double *psi);
int usvmpc_guidance_prepare(usvmpc_handle *h, const double *vel_uv, const double *pose, const double *obstacles,
                            const int *n_obstacles, int lmax);
/* The obstacle simulator's simulate() (catkin_ws/src/simulation/scripts/obstacle_sim_node.py:56-81,101-117):
 * world[batch][n_world][3] = (X, Y, R) in NED, pose[batch][3] = (ned_x, ned_y, yaw); every obstacle closer than
 * max_radius (the node: 100) is reported in the body frame, in list order, at most 64 per instance.  The lists
 * stay on the device as the input of the next usvmpc_guidance_prepare when that is called with
 * n_obstacles == NULL; obstacles [batch][64][3] / n_obstacles [batch] (both optional) receive a copy. */
int usvmpc_guidance_sense(usvmpc_handle *h, const double *pose, const double *world, int n_world, double max_radius,
                          double *obstacles, int *n_obstacles);
int usvmpc_guidance_publish(usvmpc_handle *h, double *heading, double *r_des, double *speed, double *ye, int *active);
int usvmpc_guidance_state(usvmpc_handle *h, int *wp_index, float *past_psied);
/* DEVICE-RESIDENT MISSIONS (the arithmetic: csrc/ca_guidance.hpp; the kernel: usv_guidance_tick).  The calls above talk to the host on every
 * tick; the ones below keep a mission on the device: a tick is prepare(NULL, NULL) -> usvmpc_solve_async -> publish(all NULL) ->
 * usvmpc_advance / usvmpc_advance_sim, with no host array and no stream synchronisation.  usv_model_guidance_ca1 only (any other model:
 * USVMPC_E_ARG with a message); all need usvmpc_guidance_reset first.
 *   world     : world [B][n_world][3] = NED (X, Y, R), 0 <= n_world <= 64, uploaded ONCE; replaces the previous list.  A NaN entry is refused.
 *   prepare   with vel_uv and pose both NULL (one of them NULL: USVMPC_E_ARG): needs a world list (an empty one will do).  A pending host
 *             mirror is uploaded first; then ONE kernel launch on the handle's stream, no synchronisation.  Per instance: (u, v) = x0[0..1] and
 *             (nedx, nedy, psi) = x0[5..7] as usvmpc_advance / usvmpc_advance_sim left them; the simulator's visible entries at that pose in
 *             list order (never stored); the nearest-K choice, body -> NED through float32, stage 0 of p / lh; the waypoint manager; x0 when
 *             the tick is active; the running minimum clearance; finish_tick at the first tick that finds the mission over.  These are the bits
 *             usvmpc_guidance_sense + the host-fed prepare make from the same pose.  An instance whose mission was over before the tick keeps
 *             its x0, p and lh.  The call writes x0, p and lh only - nothing a lineariser reads - so with option "pipeline_linearize" the
 *             linearisation made a tick ahead stands (the path-following front end's prepare discards it).
 *   publish   with every output NULL: enqueues and returns without synchronising.
 *   mission_state: wp_index [B], past_psied [B], finish_tick [B] (device-resident prepares since reset, from 0, at the first one that found
 *             the mission over; -1 before), min_clearance [B] (min over the visible entries and the resident ticks of
 *             sqrt(dx^2 + dy^2) - (R + 0.5) at the tick's pose, squares and sum rounded one by one; 1e300 before the first update; reset by
 *             usvmpc_guidance_reset).  Any may be NULL.
 *   world_vel : vel [B][n_world][2], NED m/s, for the current list: the world moves.  predict != 0: a resident prepare still selects on the
 *             current positions exactly as above and then writes EVERY stage for the K slots it chose: p[k][2 slot + c] = P_c + ((double)k * dt)
 *             * v_c, k = 0 .. N (unfused: csrc/obstacle_tracks.hpp), P_c the float32-rounded NED coordinate the node would have computed;
 *             lh[k][slot] replicated for k = 0 .. N-1; unused slots (1000, 1000) / 0 at every stage; "static_obstacles" goes off.  predict == 0:
 *             the world moves between ticks but is held still inside the horizon - stage 0 only, "static_obstacles" stays on.  NULL: the world
 *             is at rest again, "static_obstacles" on again.  USVMPC_E_ARG with a message, nothing changed: option "obstacle_tracks" on (and
 *             switching it on while this world moves is refused likewise: both would own p); an entry that is not finite; no world list yet.
 *             usvmpc_guidance_world on a moving world KEEPS the velocities when n_world is unchanged; otherwise the new list is at rest.
 *   world_step: enqueues world[i][c] += T * vel[i][c] (unfused; R untouched); refused while the world is at rest.  While the world moves
 *             usvmpc_advance calls it with dt and usvmpc_advance_sim with the plant's period, behind their own kernel, unless option
 *             "obstacle_step_on_advance" is 0.
 *   world_read: what the device holds - world [B][n_world][3], vel [B][n_world][2] (zeros for a world at rest); either may be NULL. */
int usvmpc_guidance_world(usvmpc_handle *h, const double *world, int n_world, double max_radius);
int usvmpc_guidance_world_vel(usvmpc_handle *h, const double *vel, int predict);
int usvmpc_guidance_world_step(usvmpc_handle *h, double T);
int usvmpc_guidance_world_read(usvmpc_handle *h, double *world, double *vel);
int usvmpc_guidance_mission_state(usvmpc_handle *h, int *wp_index, float *past_psied, int *finish_tick, double *min_clearance);
/* VESSEL ENCOUNTERS for the guidance front end: a scene's vessels as each other's moving obstacles (the arithmetic: csrc/ca_fleet_world.hpp;
 * scenes, slots and layout as usvmpc_pf_fleet below).  The batch is cut into scenes of scene_size = S consecutive instances (scene s:
 * instances s S .. s S + S - 1; shards of a larger batch must be cut at multiples of S).  Every instance keeps its own waypoints, mission
 * state and OCP, and sees the other S - 1 vessels of its scene as moving world entries that every DEVICE-RESIDENT prepare refreshes on the
 * device (kernel usv_guidance_fleet_gather, ahead of usv_guidance_tick on the handle's stream); a tick stays prepare -> solve -> publish ->
 * advance, no synchronisation, and a linearisation made a tick ahead still stands.
 *   fleet, scene_size >= 2: the world list becomes the caller's n_fixed entries followed by S - 1 fleet entries the front end owns, parked at
 *             (1000, 1000, 0) with velocity 0 until the first gather.  The world counts as moving from then on: velocities and the `predict`
 *             choice already given (usvmpc_guidance_world_vel) are kept, a world that was at rest gets zero velocities and predict 1.  With
 *             a = i mod S, fleet slot e = 0 .. S-2 of instance i is vessel j = i - a + (e < a ? e : e + 1), and list index n_fixed + e
 *             receives from x0 as usvmpc_advance / usvmpc_advance_sim left it
 *                 X = x0_j[5], Y = x0_j[6], R = radius, vX = u cos psi - v sin psi, vY = u sin psi + v cos psi
 *             with u, v, psi = x0_j[0], x0_j[1], x0_j[7]: sine and cosine evaluated once each, in double, every product and sum rounded on
 *             its own - a host that restates it agrees to 8 * 2^-52 * (|u| + |v|), the two libraries' sin / cos apart.  The entries then
 *             go the way of any moving entry: the sensor's max_radius, the nearest-K choice, the per-stage prediction (predict 0: held still
 *             inside the horizon), the running minimum clearance, the world step of usvmpc_advance / usvmpc_advance_sim.  The gather also
 *             keeps, per instance and over the other vessels of its scene, the smallest d = sqrt(dx^2 + dy^2) between the two positions
 *             and the prepare it was met at - for every instance, whatever its mission phase: a vessel whose mission is over is still in
 *             the water and is still gathered by the others.
 *   fleet, scene_size 0 or 1: the fleet is off and the list is cut back to the fixed entries, which keep their velocities
 *             (usvmpc_guidance_world_vel(NULL) puts the world at rest as ever).
 *   While the fleet is on: usvmpc_guidance_world takes the fixed entries only (n_world <= 64 - (S - 1)) and keeps the fleet slots (the fixed
 *             entries' velocities too when n_world is unchanged, else they are zero); usvmpc_guidance_world_vel takes [B][n_fixed][2];
 *             usvmpc_guidance_world_read returns all n_fixed + S - 1 entries as the device holds them; usvmpc_guidance_world_step moves every
 *             entry - the fleet slots are overwritten by the next gather.
 *   USVMPC_E_ARG with a message, nothing changed: another model; no usvmpc_guidance_reset or no world list yet (an empty list will do);
 *             B % scene_size != 0; n_fixed + S - 1 > 64; a negative or non-finite radius; option "obstacle_tracks" on (and switching it on
 *             while the fleet is on); a HOST-FED usvmpc_guidance_sense or usvmpc_guidance_prepare while the fleet is on (the scene exists on
 *             the device only); usvmpc_guidance_world_vel(NULL) while the fleet is on.
 *   fleet_state: min_separation [B] (1e300 after usvmpc_guidance_reset; a NaN never wins), separation_tick [B] (device-resident prepares since
 *             reset, from 0; -1: none yet).  Either may be NULL. */
int usvmpc_guidance_fleet(usvmpc_handle *h, int scene_size, double radius);
int usvmpc_guidance_fleet_state(usvmpc_handle *h, double *min_separation, int *separation_tick);
/* ---- Path-following front end (model usv_model_pf_ca only; any other model: USVMPC_E_ARG with a message): the arithmetic either side
 * of the solver call in the reference's path-following ROS node, batched on the device (class NMPC in catkin_ws/src/nmpc_ca/src/nmpc_pf.cpp;
 * nmpc_pf_ca.cpp is the same file; the arithmetic: csrc/pf_guidance.hpp).  Per-instance state (waypoint index k, past thrust, the reference
 * triple last written, running minimum clearance) lives in the handle.  Arrays are host pointers, instance-major.
 *   reset   = main(), new waypoint list                  :392-401   waypoints [B][2*npts], npts >= 2; k = 1, past thrust 0 (:172-173); switches
 *             "static_obstacles" on; refused while option "obstacle_tracks" is on (the tracks own p)
 *   world   = the obstacle field, uploaded once: world [B][n_world][3] = NED (X, Y, R), 0 <= n_world <= 64; an obstacle is visible when
 *             sqrt((X-nedx)^2 + (Y-nedy)^2) < max_radius (obstacle_sim_node.py:71).  The node itself has no obstacle callback: the nearest K
 *             visible ones by distance - (R + 0.5), ties by list index, go to stage 0 of p in the NED frame, bit for bit, and
 *             lh = (R + 0.5) + margin (option "pf_lh_margin", default 0.2: scripts/usv_pf_ca/main.py:126); unused slots (1000, 1000), lh 0
 *   prepare = velocityCallback / waypoint_manager / control (input part)   :198-206, :226-268, :273-335
 *             HOST-FED: vel_uvr [B][3] = (u, v, r), pose [B][3] = (nedx, nedy, psi); past thrust from the front end's state; returns when the
 *             arrays may be reused.  DEVICE-RESIDENT: both NULL - the vessel's state is read from the handle's own x0 as usvmpc_advance /
 *             usvmpc_advance_sim left it (u, v, r = x0[3..5]; psi, nedx, nedy = x0[0], x0[10], x0[11]; past thrust = x0[12..13]) and the
 *             solver inputs are written in place: the call enqueues on the handle's stream and returns, no synchronisation.
 *             Per instance: distance to the segment's end > 1: ACTIVE - x0, and yref / yref_e ONLY when (sin ak, cos ak, u_des) differ bit
 *             for bit from what the front end last wrote there (or the caller has written yref / yref_e since, by usvmpc_set or through a
 *             device pointer: then every active instance is rewritten once); distance <= 1: SWITCH TICK - k += 1 and nothing else (:252-256:
 *             x0, yref and the published values keep what they hold; the batched solve still runs); k >= npts: MISSION OVER.  Obstacles and the
 *             running minimum clearance are updated for every instance whose mission is not over.  A pending host mirror is uploaded first;
 *             usvmpc_get of "x0", "yref", "yref_e", "p", "lh" afterwards returns what the kernel wrote.  For the pipelined lineariser a prepare
 *             counts as a caller write of yref (a handle driven by this front end linearises inside its solves).
 *   publish = control (output part) :347-376   active: thr_port / thr_stbd = x_1[12], x_1[13] (kept as past thrust), e_u = (float)(0.7 - u),
 *             e_ye = (float)(0 - ye), Tx = port + 0.78 stbd, Tz = (port - 0.78 stbd) 0.41 / 2 (the node's constants), speed 0.7; mission over:
 *             thrusters and speed 0 (:260-266); switch tick: unchanged.  active [B]: 1 for an active tick.  Any output may be NULL; with all NULL the
 *             call only enqueues, otherwise it synchronises the stream.
 *   state   : wp_index [B], finish_tick [B] (prepares since reset, from 0, at the first one that found the mission over; -1 before),
 *             min_clearance [B] (smallest distance - (R + 0.5) over the visible obstacles, any tick; 1e300 before the first update),
 *             yref_writes [1] (instance rewrites of yref since reset).  Any may be NULL.
 * A MOVING WORLD: every entry of the world list has a constant velocity, and a mission tick stays prepare -> solve -> publish -> advance.
 *   world_vel : vel [B][n_world][2], NED m/s, for the list last given to usvmpc_pf_world.  Non-NULL: the world moves - "static_obstacles" goes
 *             off and every following prepare, having selected the nearest K on the CURRENT positions exactly as above, writes the predicted
 *             set of every stage for the K it chose: p[k][2 slot + c] = X_c + ((double)k * dt) * v_c, k = 0 .. N (unfused, the arithmetic of the
 *             obstacle tracks: csrc/obstacle_tracks.hpp; stage 0 is the world's coordinates), lh[k][slot] = (R + 0.5) + margin, k = 0 .. N-1; an
 *             unused slot stays (1000, 1000), lh 0 at every stage.  Instances whose mission is over keep their p and lh; switch ticks write.
 *             NULL: back to a world at rest, "static_obstacles" on again - the front end behaves exactly as described above.
 *             USVMPC_E_ARG with a message: another model; no world list yet; an entry that is not finite; option "obstacle_tracks" on (and
 *             switching "obstacle_tracks" on while the world moves is refused likewise: both would own p).
 *             usvmpc_pf_world on a handle whose world moves replaces the positions and KEEPS the velocities when n_world is unchanged; with
 *             another n_world the new list is at rest until its velocities are given.
 *   world_step: enqueues world[i][c] += T * vel[i][c] (unfused; R untouched) on the handle's stream; refused while the world is at rest.  While
 *             the world moves usvmpc_advance calls it with dt and usvmpc_advance_sim with the plant's period, behind their own kernel, unless
 *             option "obstacle_step_on_advance" is 0 (one meaning for tracks and front end: the world is the caller's to move).
 *   world_read: what the device holds - world [B][n_world][3], vel [B][n_world][2] (zeros for a world at rest); either may be NULL.
 *   option "pf_predict" (default 1) - 0: the world moves between ticks but is held still inside the horizon: "static_obstacles" stays on and a
 *             prepare writes stage 0 only, as for a world at rest (what the obstacle tracks do under "static_obstacles"; the baseline that shows
 *             what prediction buys).
 *   min_clearance, finish_tick, yref_writes and the yref rule are those of a world at rest. */
int usvmpc_pf_reset(usvmpc_handle *h, const double *waypoints, int npts);
int usvmpc_pf_world(usvmpc_handle *h, const double *world, int n_world, double max_radius);
int usvmpc_pf_prepare(usvmpc_handle *h, const double *vel_uvr, const double *pose);
int usvmpc_pf_publish(usvmpc_handle *h, double *thr_port, double *thr_stbd, double *Tx, double *Tz, float *e_u, float *e_ye, double *speed,
                      int *active);
int usvmpc_pf_state(usvmpc_handle *h, int *wp_index, int *finish_tick, double *min_clearance, long long *yref_writes);
int usvmpc_pf_world_vel(usvmpc_handle *h, const double *vel);
int usvmpc_pf_world_step(usvmpc_handle *h, double T);
int usvmpc_pf_world_read(usvmpc_handle *h, double *world, double *vel);
/* VESSEL ENCOUNTERS: a scene's vessels as each other's moving obstacles (the arithmetic: csrc/fleet_world.hpp).  The batch is cut into scenes
 * of scene_size = S consecutive instances (scene s: instances s S .. s S + S - 1; shards of a larger batch must be cut at multiples of S).
 * Every instance keeps its own waypoints, mission state and OCP, and sees the other S - 1 vessels of its scene as moving world entries that
 * every DEVICE-RESIDENT prepare refreshes on the device (kernel usv_pf_fleet_gather, ahead of the prepare's own kernel on the handle's stream);
 * a tick stays prepare -> solve -> publish -> advance, no synchronisation.
 *   fleet, scene_size >= 2: the world list becomes the caller's n_fixed entries followed by S - 1 fleet entries the front end owns, parked at
 *             (1000, 1000, 0) with velocity 0 until the first gather.  The world counts as moving from then on ("static_obstacles" off;
 *             option "pf_predict" 0 holds the scene still inside the horizon): velocities already given to the fixed entries are kept, a world
 *             that was at rest gets zero velocities.  With a = i mod S, fleet slot e = 0 .. S-2 of instance i is vessel
 *             j = i - a + (e < a ? e : e + 1), and list index n_fixed + e receives from x0 as usvmpc_advance / usvmpc_advance_sim left it
 *                 X = x0_j[10], Y = x0_j[11], R = radius, sog = sqrt(x0_j[3]^2 + x0_j[4]^2), vX = sog * x0_j[2], vY = sog * x0_j[1]
 *             (x0[1], x0[2]: the model's sin / cos of the course angle; no trigonometric call, every product and sum rounded on its own).
 *             The gather also keeps, per instance and over the other vessels of its scene, the smallest d = sqrt(dx^2 + dy^2) between the
 *             two positions and the prepare it was met at - for every instance, whatever its mission phase: a vessel whose mission is over
 *             is still in the water and is still gathered by the others.
 *   fleet, scene_size 0 or 1: the fleet is off and the list is cut back to the fixed entries, which keep their velocities
 *             (usvmpc_pf_world_vel(NULL) puts the world at rest as ever).
 *   While the fleet is on: usvmpc_pf_world takes the fixed entries only (n_world <= 64 - (S - 1)) and keeps the fleet slots (the fixed
 *             entries' velocities too when n_world is unchanged, else they are zero); usvmpc_pf_world_vel takes [B][n_fixed][2];
 *             usvmpc_pf_world_read returns all n_fixed + S - 1 entries as the device holds them; usvmpc_pf_world_step moves every entry - the
 *             fleet slots are overwritten by the next gather.
 *   USVMPC_E_ARG with a message, nothing changed: another model; no usvmpc_pf_reset or no world list yet (an empty list will do);
 *             B % scene_size != 0; n_fixed + S - 1 > 64; a negative or non-finite radius; option "obstacle_tracks" on (and switching it on
 *             while the fleet is on); a HOST-FED prepare while the fleet is on (the scene exists on the device only);
 *             usvmpc_pf_world_vel(NULL) while the fleet is on.
 *   fleet_state: min_separation [B] (1e300 after usvmpc_pf_reset; a NaN never wins), separation_tick [B] (prepares since reset, from 0;
 *             -1: none yet).  Either may be NULL. */
int usvmpc_pf_fleet(usvmpc_handle *h, int scene_size, double radius);
int usvmpc_pf_fleet_state(usvmpc_handle *h, double *min_separation, int *separation_tick);
/* EXCHANGED PLANS for both front ends' fleets (the arithmetic: csrc/fleet_plan.hpp; the rule for when a plan is usable: csrc/world_plan.hpp,
 * PlanState).  Off by default.  A scene-mate is a vessel of this batch, and its own NMPC has just solved where it will go: x[j][1 .. N].  With
 * plans on a device-resident prepare does all it did - gather, nearest-K choice on current positions, tracks, every stage of p and lh from
 * pos + (k dt) vel - and ONE more kernel behind it on the handle's stream (usv_pf_fleet_plans / usv_guidance_fleet_plans) rewrites stages
 * 1 .. N of the slots that hold a scene-mate with a usable plan: with P_k the position pair of x[j][k], q the slot's stage-0 position and
 * e = q - P_1,   p[k] = P_{k+1} + e  (k = 1 .. N-1),   p[N] = (P_N + (P_N - P_{N-1})) + e;   stage 0 stays q and lh is untouched.
 *   A plan is used only when the iterate is exactly ONE HAND-OVER OLD: solved (usvmpc_solve*), then handed over once (usvmpc_advance,
 *             _advance_sim, the cascade's hand-over step), and not since written by the caller (usvmpc_set "x", its device pointer handed
 *             out), nor the front end reset, nor the fleet switched off, nor plans switched on.  The prepare that uses it uses it up: a second
 *             prepare without a solve and a hand-over in between is the constant-velocity prepare, as is one after two hand-overs.
 *             Besides: the instance streams this tick, the mate's mission is not over, and status[j] of the last solve is 0.  Every other
 *             slot keeps the constant-velocity bits.  While the world is not predicted inside the horizon ("pf_predict" 0, predict 0) the
 *             kernel is not launched.
 *   fleet_plans refuses, in this order: another model; (guidance) before usvmpc_guidance_reset; no fleet on (path following: or before
 *             usvmpc_pf_reset) - "... come first"; N < 2.  A refused call changes nothing.
 *   fleet_plan_state: source [B][K] of the last prepare - the vessel whose plan fed each slot, -1: none; plan_fed - plan-fed (instance, slot)
 *             pairs so far, counted on the device; plan_launches - launches of the plan kernel so far.  Any may be NULL.  A handle that never
 *             switched plans on answers -1, 0, 0. */
int usvmpc_pf_fleet_plans(usvmpc_handle *h, int on);
int usvmpc_pf_fleet_plan_state(usvmpc_handle *h, int *source, long long *plan_fed, long long *plan_launches);
int usvmpc_guidance_fleet_plans(usvmpc_handle *h, int on);
int usvmpc_guidance_fleet_plan_state(usvmpc_handle *h, int *source, long long *plan_fed, long long *plan_launches);
/* Profiling aid: stream `nplanes` workspace planes with the solver kernels' access instruction
 * (kernel usv_calib_stream) and report the exact byte counts, to calibrate HBM PMC counters.
 * Overwrites solver scratch; the next usvmpc_solve re-initialises it. */
int usvmpc_calibrate_traffic(usvmpc_handle *h, int nplanes, double *bytes_read, double *bytes_written);
/* Test entry points (no handle): the device transcription of the reference's model files evaluated on caller-supplied
 * points - f [n][nx] and the Jacobian J [n][nx][nu+nx] with respect to z = [u; x] exactly as the lineariser obtains them
 * (one tangent column per call of the model's fjvp), for the CasADi expressions of
 * catkin_ws/src/nmpc_ca/scripts/{usv_acados,usv_guidance_ca1,usv_pf_ca}/usv_model.py; and the obstacle row
 * h = sqrt((px-ox)^2 + (py-oy)^2) with its position gradient exactly as the QP kernel evaluates it:
 * pos [n][2], p [n][2K] -> h [n][K], grad [n][K][2]. */
int usvmpc_debug_model_eval(int model, int device, int n, const double *x, const double *u, double *f, double *J);
int usvmpc_debug_obstacle_eval(int device, int n, int K, const double *pos, const double *p, double *h, double *grad);
/* ... the same f and J as the kernels obtain them INSIDE a shooting interval: the model's per-interval preparation at x_start [n][nx]
 * (ModelCall<M>::prepare), then the evaluation at x [n][nx] (ModelCall<M>::fjvp).  For usv_model_pf_ca this takes sin / cos(psi)
 * from those at x_start by the series in d = x[0] - x_start[0] (or the library call beyond |d| > 0.125); models without a
 * preparation give what usvmpc_debug_model_eval gives.  And the two fast-math primitives of the kernels on n operands:
 * rcp[i] = lanes::frcp(x[i]), rsq[i] = lanes::frsqrt(x[i]) (hardware estimate + two Newton steps). */
int usvmpc_debug_model_eval_from(int model, int device, int n, const double *x_start, const double *x, const double *u, double *f, double *J);
int usvmpc_debug_fast_math(int device, int n, const double *x, double *rcp, double *rsq);
/* ... and every cross-lane primitive the kernels are written against (csrc/gfx950/lanes.hpp) on caller-supplied operands, through the probe
 * body of csrc/lanes_probe.hpp: in [ngroups][NIN][16], iin [ngroups][NIIN][16] -> out [ngroups][NOUT][16], iout [ngroups][NIOUT][16] (both
 * in/out: a result the workgroup shape does not produce keeps the caller's value; the atomics start from the caller's entries).
 * block_threads is 64 (one wave per workgroup) or 256 (four).  planes is an allocation of planes_doubles doubles that holds the probe's
 * plane window of ngroups * 3 * 16 doubles from element 64 on, with at least 64 more behind it; it is copied back, so that the caller
 * sees what the stores changed and that nothing outside the window was touched. */
int usvmpc_debug_lanes(int device, int ngroups, int block_threads, const double *in, const int *iin, double *out, int *iout, double *planes,
                       long planes_doubles);
/* ---- Integrator (acados_template.AcadosSimSolver): B instances of a model's explicit RK4 over one sampling period T, in num_steps
 * steps of T / num_steps, with the forward sensitivities when sens_forw != 0.  The same model functions and RK4 arithmetic as the
 * lineariser's (csrc/sim.hpp); x_next is the same bits with sens_forw on or off, and an instance's result does not depend on the batch.
 * Arrays are FP64, instance-major; n is the length PER INSTANCE:
 *   set "x" [B][nx] (n = nx), "u" [B][nu] (n = nu), "T" (n = 1: the period, one value for the batch);
 *   get "x" [B][nx]: x_next of the last solve; "S_forw" [B][nx][nx + nu] (n = nx * (nx + nu)): [Sx | Su] row-major, the layout of
 *       acados' S_forw as recalled (the acados sources are not at hand); "T".
 * usvmpc_sim_solve is synchronous.  Device pointers: "x", "u" (inputs), "x_next", "S_forw" (outputs).  usvmpc_sim_create refuses
 * (USVMPC_E_ARG) an unknown model, T <= 0 or NaN, num_steps < 1, batch < 1; usvmpc_sim_last_error(NULL) describes the last failed
 * create of the calling thread.  No adjoint or second-order sensitivities, no implicit integrators. */
typedef struct usvmpc_sim_desc {
    int model;             /* USVMPC_MODEL_*; USVMPC_MODEL_GENERATED only in a library built for it */
    int batch;
    int device;
    double T;              /* sampling period */
    int num_steps;         /* RK4 steps per period (acados sim_method_num_steps) */
    int sens_forw;         /* 1: also S_forw */
} usvmpc_sim_desc;
typedef struct usvmpc_sim usvmpc_sim;
int usvmpc_sim_create(const usvmpc_sim_desc *d, usvmpc_sim **out);
int usvmpc_sim_destroy(usvmpc_sim *s);
int usvmpc_sim_set(usvmpc_sim *s, const char *field, const double *v, size_t n);
int usvmpc_sim_solve(usvmpc_sim *s);
int usvmpc_sim_get(usvmpc_sim *s, const char *field, double *out, size_t n);
int usvmpc_sim_get_device_ptr(usvmpc_sim *s, const char *field, void **dptr);
/* Adopt a caller-owned HIP stream for the integrator's copies and kernels */
int usvmpc_sim_set_stream(usvmpc_sim *s, void *stream);
const char *usvmpc_sim_last_error(usvmpc_sim *s);
/* Closed-loop plant step on the device: x0 <- sim(x0, u at stage 0) over the plant's T in its num_steps RK4 steps, plus
 * sigma * N(0,1) on the states of option "disturbance_mask" (keyed as usvmpc_advance: option "instance_offset"); enqueued on the
 * solver's stream.  The plant must come from this library and have the solver's model, nx and device (else USVMPC_E_ARG); only its
 * T and num_steps are read - its buffers are not touched. */
int usvmpc_advance_sim(usvmpc_handle *h, const usvmpc_sim *plant, double sigma, unsigned long long seed);
/* ---- Closed-loop log: the trajectory a closed loop leaves behind (the reference's simX[i] = get(0, "x"), simU[i] = get(0, "u") and its
 * tracking-error statistics: scripts/usv_pf_ca/main.py:153-176), kept on the device so that a device-resident loop stays free of host
 * arrays and synchronisation (the schedule and layout: csrc/log_plan.hpp; the arithmetic: csrc/closed_loop_log.hpp; the kernel:
 * usv_log_record).  A HAND-OVER is a call of usvmpc_advance or usvmpc_advance_sim; hand-overs are counted from 0 since usvmpc_log_start.
 * While a log runs each of them first enqueues usv_log_record on the handle's stream, AHEAD of its own kernel; a handle without a log
 * launches exactly what it did before.
 *   A RECORD is made at hand-over i when i >= first, (i - first) % every == 0 and fewer than `capacity` records exist; with the buffer
 *   full `missed` counts it and nothing is stored (no ring).  It holds the values at the moment the hand-over was called, before its kernel
 *   overwrites x0: the selected states of x0 as the solve saw them, u of stage 0, and status | qp_iter << 8 of the last solve.
 *   ERROR SUMS: at every hand-over i >= err_first, recorded or not, each (instance, channel c) takes e = x0[err_a[c]] - (err_b[c] >= 0 ?
 *   x0[err_b[c]] : err_c[c]) into sum_abs += |e| and sum_sq += e e - each operation rounded on its own, in tick order: the bits a
 *   sequential numpy loop makes.  Means are the caller's division by `count`.
 *   log_start : allocates the buffers, zeroes sums and counters.  USVMPC_E_ARG with a message, nothing changed: a log already runs
 *               ("usvmpc_log_stop first"); capacity < 1, every < 1, first < 0; a state_mask bit >= nx; n_err outside 0 .. 4; err_a or err_b
 *               >= nx, err_a < 0; a non-finite err_c that is used; a descriptor that records nothing; sizes that overflow 64 bits.  A failed
 *               allocation: USVMPC_E_HIP, nothing changed.
 *   log_stop  : frees the buffers (usvmpc_destroy does too); usvmpc_device_bytes includes them while the log runs.
 *   log_info  : records made, hand-overs counted, hand-overs missed, states per record; any output may be NULL.
 *   log_read  : channel "x", "u" or "status" -> out [nrec][nb][n], tick-major, for records rec0 .. rec0 + nrec - 1 and instances b0 ..
 *               b0 + nb - 1; n = nsel, nu or 1, FP64 or int32; `bytes` must be exactly that size; records not made yet, instances outside the
 *               batch and a channel that is not recorded are refused.  One 2-D copy; synchronises the stream.
 *   log_errors: sum_abs, sum_sq [B][n_err], count = hand-overs that entered the sums; any may be NULL; synchronises the stream.
 *   log_device_ptr: "x" [capacity][B][nsel], "u" [capacity][B][nu], "status" [capacity][B], "sum_abs", "sum_sq" [B][n_err] on the device.
 * The record kernel reads x0, u, status and qp_iter and writes log memory only: it is no caller write - the pipelined lineariser's work
 * made a tick ahead stands, and log_device_ptr, which exposes log memory only, leaves it alone as well.
 * Not provided: a ring mode; the front ends' published values and waypoint index (positions, ak and the thrusts are states); a cost
 * channel - the realised closed-loop cost is usvmpc_cost_track's ("Objective value" below).  A loop around usvmpc_solve_sqp is logged like
 * any other: whatever the solve, the hand-over records. */
typedef struct usvmpc_log_desc {
    int capacity;        /* records kept, >= 1 */
    int every;           /* one record every `every`-th hand-over, >= 1 */
    int first;           /* first hand-over recorded, counted from 0 since usvmpc_log_start, >= 0 */
    unsigned state_mask; /* bit j: state j of x0 is recorded (bits >= nx refused); 0: no state channel */
    int record_u;        /* 1: u of stage 0 */
    int record_status;   /* 1: one int32 per instance = status | qp_iter << 8 */
    int n_err;           /* 0 .. 4 error channels: e = x0[a] - (b >= 0 ? x0[b] : c) */
    int err_a[4], err_b[4]; double err_c[4];
    int err_first;       /* first hand-over that enters the sums (main.py: 401) */
} usvmpc_log_desc;
int usvmpc_log_start(usvmpc_handle *h, const usvmpc_log_desc *d);
int usvmpc_log_stop(usvmpc_handle *h);
int usvmpc_log_info(usvmpc_handle *h, int *records, long long *handovers, long long *missed, int *nsel);
int usvmpc_log_read(usvmpc_handle *h, const char *channel, int rec0, int nrec, int b0, int nb, void *out, size_t bytes);
int usvmpc_log_errors(usvmpc_handle *h, double *sum_abs, double *sum_sq, long long *count);
int usvmpc_log_device_ptr(usvmpc_handle *h, const char *channel, void **dptr);
/* ---- Objective value (acados' AcadosOcpSolver.get_cost()): the cost of the iterate the handle holds and the realised closed-loop cost, on
 * the device, so that a device-resident loop compares weightings, horizons and prediction modes without reading x, u, yref, sl and su back
 * every tick (the arithmetic: csrc/cost_eval.hpp; the kernels: usv_cost_eval, usv_cost_track).  With z = [u_k; x_k], V = [Vu Vx], dt = Tf / N:
 *       r = V z - yref[k],  ls_k = (0.5 dt) r' W r,  slack_k = dt * sum_i (zl_i sl_i + zu_i su_i + 0.5 Zl_i sl_i^2 + 0.5 Zu_i su_i^2)   (soft h rows;
 *       hard ones: 0),  c_k = ls_k + slack_k  for k < N;   c_N = 0.5 r' W_e r,  r = Vx_e x_N - yref_e;   cost = c_0 + .. + c_N
 * Every product, difference and sum is rounded on its own (no fused multiply-add) and every sum runs sequentially from 0.0 in the order
 * csrc/cost_eval.hpp writes down - the order is part of the interface: a sequential numpy loop over get "x", "u", "yref", "sl", "su"
 * returns the same bits.  No clamp: a negative slack enters as it is; a NaN stays a NaN in its instance and in no other.
 *   get "cost" [batch] (n = 1, stage ignored), "cost_stage" (stage 0..N, n = 1; stage -1: [batch][N+1]), "cost_parts" [batch][3] (n = 3, stage
 *       ignored) = [sum of ls_k, c_N, sum of slack_k]: every such usvmpc_get uploads pending host writes, enqueues usv_cost_eval on the
 *       handle's stream, copies and synchronises - no staleness state is kept, the value is that of the arrays as the device holds them
 *       (whichever solve produced them, or the caller's own sets).  usvmpc_set of them is refused like any output.
 *   usvmpc_eval_cost: enqueues the evaluation without synchronising - for resident loops that read the result through
 *       usvmpc_get_device_ptr "cost" | "cost_stage" | "cost_parts".  The three buffers and the kernels' tables are made by the first call of
 *       either kind: a handle that never asks for a cost allocates nothing and launches what it always did.
 *   usvmpc_cost_track(h, 1): allocates sum [batch], zeroes sum and count and starts (while running: zeroes again); (h, 0): stops and frees.
 *       While tracking runs every hand-over (usvmpc_advance, usvmpc_advance_sim) first enqueues usv_cost_track AHEAD of its own kernel (where
 *       the log's record goes):  sum[b] = sum[b] + c_0(x0[b], u[b][0], yref[b][0], sl[b][0], su[b][0]) - the stage function with z = [u_0; x0],
 *       the state the solve saw (after a status-4 solve x of stage 0 may be something else), in hand-over order.
 *   usvmpc_cost_track_now: one step of the tracked sum outside a hand-over, for loops that never call usvmpc_advance (a cascade's two
 *       solvers): uploads pending host writes, enqueues the same usv_cost_track and counts one.  USVMPC_E_ARG with a message while no tracking
 *       runs.  Call it after the solve whose stage 0 it should cost and ahead of whatever overwrites x0.
 *   usvmpc_cost_tracked: sum [batch] (may be NULL) and the hand-overs counted; synchronises.  USVMPC_E_ARG with a message while no tracking
 *       runs.  usvmpc_get_device_ptr "cost_tracked" is the sum on the device (while tracking runs).
 * Neither kernel is a caller write: they read x, u, yref and write cost memory only, so the pipelined lineariser's pass made a tick ahead
 * stands and the device pointers above cancel nothing.  usvmpc_device_bytes includes every cost buffer while it exists.
 * Not built for handles with soft state bounds, whose slack values are not among the arrays a caller can get: every entry point answers
 * USVMPC_E_ARG, "cost: not built for soft state bounds".  No option and no channel of the log. */
int usvmpc_eval_cost(usvmpc_handle *h);
int usvmpc_cost_track(usvmpc_handle *h, int on);
int usvmpc_cost_track_now(usvmpc_handle *h);
int usvmpc_cost_tracked(usvmpc_handle *h, double *sum, long long *count);
/* ---- Cascade: the two-layer control stack the reference deploys, closed on a vessel with inertia.  The guidance layer (a
 * usv_model_guidance_ca1 handle of THIS library with its device-resident front end) runs every `ratio`-th tick and publishes a desired
 * heading and speed; the low-level NMPC (OCP usv_model_low_level: nx = 8, nu = 2, no obstacles; the node: nmpc_low_level.cpp) runs every
 * tick and turns them into thrusts; a 3-DOF vessel s = (nedx, nedy, psi, u, v, r) integrates the PUBLISHED thrusts over T in num_steps RK4
 * steps, with the starboard factor c (0.78: the low-level model's).  The low-level solver lives in a library generated for its model, so it
 * is handed over as raw device pointers (usvmpc_get_device_ptr of ITS library: "x0", "x", "yref", "yref_e"), its horizon ll_N and its batch;
 * the caller keeps it on the guidance handle's stream, with options "pipeline_linearize" 0 and "host_mirror" 0 (its yref and x0 are written
 * behind its back: every solve must linearise afresh from device memory).  One low-level tick t = 0, 1, ..:
 *     [t % ratio == 0:  usvmpc_guidance_prepare(h, NULL ..) -> usvmpc_solve_async(h) -> usvmpc_guidance_publish(h, NULL ..)]
 *     usvmpc_cascade_refs -> low-level usvmpc_solve_async -> usvmpc_cascade_step
 * No usvmpc_advance of either solver: the handles' closed-loop logs hang on the hand-overs and do not see cascade ticks.  A cascade's runs are
 * recorded by its own log ("Cascade log" below) and costed by usvmpc_cost_track_now on either solver: the guidance handle's right after its
 * usvmpc_solve_async, the low-level solver's right after its usvmpc_solve_async and ahead of usvmpc_cascade_step.
 *   create   USVMPC_E_ARG with a message (usvmpc_cascade_last_error(NULL)), nothing made: another guidance model; no usvmpc_guidance_reset
 *            or no world list yet; ratio < 1, num_steps < 1, T <= 0; T or c not finite; ratio * T different from the guidance handle's
 *            shooting interval; a null device pointer; ll_batch different from the guidance handle's batch; yref / yref_e not 16-byte
 *            aligned.  The object owns its device buffers; the guidance handle allocates nothing and launches what it launched before.
 *   reset    pose [batch][3] = (nedx, nedy, psi), vel [batch][3] = (u, v, r): the vessel's state; published and past thrusts 0, tick 0, error
 *            sums 0, yref_writes 0, every instance's reference rows due at the first refs.  Writes the guidance handle's x0[0, 1, 5, 6, 7] =
 *            (u, v, nedx, nedy, psi).  Synchronises.  The low-level initial iterate is the caller's business.  Refused while a log runs
 *            ("usvmpc_cascade_log_stop first").
 *   refs     kernel usv_cascade_refs, enqueued: low-level x0 = (psi, sin psi, cos psi, u (0 -> 0.001), v, r, past thrusts); yref rows
 *            (psi_des, sin, cos, u_des, 0 ..) x ll_N and yref_e rewritten for the instances whose (heading, speed) bits differ from what was
 *            last written - yref_writes counts them.
 *   step     kernel usv_cascade_step, enqueued: thrusts = (x_1[6], x_1[7]) of the low-level iterate, both 0 while u_des == 0; past thrusts =
 *            x_1[6], x_1[7] regardless; e_u = (float)(u_des - u), e_psi = (float)(psi_des - psi) into the running sums; one plant period;
 *            sigma * N(0,1) on (u, v, r), drawn as usvmpc_advance draws (key (instance_offset + b) * 6 + j, j = 3, 4, 5).  When the next tick is
 *            a guidance tick the vessel's state goes into the guidance handle's x0[0, 1, 5, 6, 7] and a moving guidance world moves on by
 *            ratio * T (option "obstacle_step_on_advance").
 *   state    state [batch][6], thrust [batch][2], past_thrust [batch][2], ticks [batch], yref_writes, err_sums [batch][4] = (sum |e_u|,
 *            sum |e_psi|, sum e_u^2, sum e_psi^2); any may be NULL; synchronises.
 *   destroy  before the guidance handle is destroyed. */
typedef struct usvmpc_cascade usvmpc_cascade;
int usvmpc_cascade_create(usvmpc_handle *guidance, int ratio, double T, int num_steps, double c, long long instance_offset, int ll_batch,
                          int ll_N, void *ll_x0, void *ll_x, void *ll_yref, void *ll_yref_e, usvmpc_cascade **out);
int usvmpc_cascade_destroy(usvmpc_cascade *c);
int usvmpc_cascade_reset(usvmpc_cascade *c, const double *pose, const double *vel);
int usvmpc_cascade_refs(usvmpc_cascade *c);
int usvmpc_cascade_step(usvmpc_cascade *c, double sigma, unsigned long long seed);
int usvmpc_cascade_state(usvmpc_cascade *c, double *state, double *thrust, double *past_thrust, int *ticks, long long *yref_writes,
                         double *err_sums);
const char *usvmpc_cascade_last_error(usvmpc_cascade *c);
/* ---- Cascade log: the trajectory a cascade leaves behind (the reference's simX[i], simU[i] and status, of the stack it deploys), kept on the
 * device so that a tick stays free of host arrays and synchronisation (the schedule and layout: csrc/cascade_log_plan.hpp; the kernel:
 * usv_cascade_record).  Low-level ticks are counted from 0 since usvmpc_cascade_log_start.  While a log runs, usvmpc_cascade_step of a tick that
 * records first enqueues usv_cascade_record on the shared stream, AHEAD of usv_cascade_step; a cascade without a log launches exactly what
 * it did before.
 *   A RECORD is made at tick i when i >= first, (i - first) % every == 0 and fewer than `capacity` records exist; with the buffer full
 *   `missed` counts it and nothing is stored (no ring).  Its channels, tick-major:
 *     "state"  [capacity][batch][nsel] FP64   the selected entries of (nedx, nedy, psi, u, v, r) as the tick's low-level solve saw them,
 *                                             before the plant period
 *     "thrust" [capacity][batch][2]    FP64   the thrusts the tick publishes: what usv_cascade_step is about to write, 0 while u_des == 0
 *     "ref"    [capacity][batch][2]    FP64   the (heading, speed) the low level tracks at the tick: the guidance layer's last published pair
 *     "err"    [capacity][batch][2]    FP32   (e_u, e_psi) of the tick: the values usv_cascade_step feeds into its sums
 *     "status" [capacity][batch]       int32  low-level status in bits 0-7 and qp_iter in bits 8-15, guidance status in bits 16-23 and
 *                                             qp_iter in bits 24-30, both of the guidance layer's most recent solve
 *   Thrusts and errors are computed by the function usv_cascade_step calls, on the same values: the recorded bits are the published bits.
 *   log_start : allocates the buffers through the guidance handle (usvmpc_device_bytes of it counts them), zeroes the counters.  ll_status
 *               and ll_qp_iter are the low-level solver's device pointers (usvmpc_get_device_ptr of ITS library: "status", "qp_iter"), needed
 *               only when record_status is set.  USVMPC_E_ARG with a message, nothing changed: a log already runs
 *               ("usvmpc_cascade_log_stop first"); capacity < 1, every < 1, first < 0; a state_mask bit >= 6; a descriptor that records
 *               nothing; sizes that overflow 64 bits; record_status with a null pointer.  A failed allocation: USVMPC_E_HIP, nothing changed.
 *   log_stop  : frees the buffers (usvmpc_cascade_destroy does too).
 *   log_info  : records made, ticks counted, ticks missed, states per record; any output may be NULL.
 *   log_read  : channel -> out [nrec][nb][n], tick-major, for records rec0 .. rec0 + nrec - 1 and instances b0 .. b0 + nb - 1; n = nsel, 2, 2,
 *               2 or 1; `bytes` must be exactly that size; records not made yet, instances outside the batch and a channel that is not
 *               recorded are refused.  One 2-D copy; synchronises the stream.
 *   log_device_ptr: the channel's buffer on the device.
 * The record kernel reads the cascade's state, the low-level iterate and both solvers' status and writes log memory only.
 * Not provided: a ring mode; error sums (usvmpc_cascade_state has the cascade's own); a cascade's ticks in the handles' own logs. */
typedef struct usvmpc_cascade_log_desc {
    int capacity;        /* records kept, >= 1 */
    int every;           /* one record every `every`-th low-level tick, >= 1 */
    int first;           /* first tick recorded, counted from 0 since usvmpc_cascade_log_start, >= 0 */
    unsigned state_mask; /* bit j: entry j of (nedx, nedy, psi, u, v, r) is recorded (bits >= 6 refused); 0: no state channel */
    int record_thrust;   /* 1: the two published thrusts */
    int record_ref;      /* 1: the tracked (heading, speed) */
    int record_err;      /* 1: (e_u, e_psi) as float32 */
    int record_status;   /* 1: one int32 per instance, both layers' status and qp_iter */
} usvmpc_cascade_log_desc;
int usvmpc_cascade_log_start(usvmpc_cascade *c, const usvmpc_cascade_log_desc *d, const int *ll_status, const int *ll_qp_iter);
int usvmpc_cascade_log_stop(usvmpc_cascade *c);
int usvmpc_cascade_log_info(usvmpc_cascade *c, int *records, long long *ticks, long long *missed, int *nsel);
int usvmpc_cascade_log_read(usvmpc_cascade *c, const char *channel, int rec0, int nrec, int b0, int nb, void *out, size_t bytes);
int usvmpc_cascade_log_device_ptr(usvmpc_cascade *c, const char *channel, void **dptr);
/* bytes of device memory held by the handle */
size_t usvmpc_device_bytes(usvmpc_handle *h);
const char *usvmpc_last_error(usvmpc_handle *h);

#ifdef __cplusplus
}
#endif
#endif
