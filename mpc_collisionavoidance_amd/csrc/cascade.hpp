// cascade.hpp — the coupling arithmetic of the two-layer control stack the reference deploys: the guidance NMPC (nmpc_guidance_ca1.cpp, 20 Hz)
// publishes a desired heading and speed, the low-level NMPC (catkin_ws/src/nmpc_ca/src/nmpc_low_level.cpp, 100 Hz; OCP usv_model_low_level)
// turns them into thruster commands, and a vessel with 3-DOF dynamics answers.  Per instance, as pure functions: host + device, no dependency
// on the kernels (usvmpc.hip: usv_cascade_refs, usv_cascade_step, usv_cascade_record; tests/cascade_harness.cpp).
//     low-level inputs   velocityCallback :177-185, positionCallback :187-192, desired*Callback :194-204, control :206-245
//     low-level outputs  control :256-285
//     the vessel         state s = (nedx, nedy, psi, u, v, r), input the two published thrusts held over the period:
//                        s' = (u cos psi - v sin psi, u sin psi + v cos psi, r, Dof3::eval(c, u, v, r, Tport, Tstbd)), c a run-time value
//                        (0.78: the low-level model's).  A model struct for erk_period<CasVessel, false> (sim.hpp), NOT a registry model; c
//                        travels as a third, constant "input" so that the struct stays stateless.
// Quirks of the node are kept: u == 0 becomes 0.001; the thrusts come from x_1, not u_0 ("because of the derivative", :256); they are
// published as 0 while u_des == 0 but past_T follows x_1 regardless; the errors are rounded through float.
// Rounding.  Nothing here is a sum of products: the inputs are copies plus one sine and one cosine, evaluated once each in double (host and
// device agree to the difference between two maths libraries); the plant period is erk_period's arithmetic (fused on the device, to 1e-12
// of an unfused restatement: tests/test_gpu_sim.py's rule).
#pragma once

#include <cmath>

#include "ca_guidance.hpp"
#include "models.hpp"
#include "sim.hpp"

namespace usv {

constexpr int CAS_NX = 8;       // low-level state (psi, sinpsi, cospsi, u, v, r, Tport, Tstbd)
constexpr int CAS_NY = 10;      // a reference row: the state and (UTportdot, UTstbddot)
constexpr int CAS_NS = 6;       // vessel state (nedx, nedy, psi, u, v, r)
constexpr double CAS_C = 0.78;  // usv_low_level/usv_model.py: the starboard thruster's factor

// the bits of a double (set-points are compared bit for bit: -0.0 and 0.0 differ, a NaN equals itself)
USV_HD unsigned long long cas_bits(double v)
{
    unsigned long long b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}

// ---- the multi-rate schedule: low-level tick t (counted from 0) is a guidance tick when ratio divides it
USV_HD bool cas_guidance_tick(long long tick, int ratio) { return tick % ratio == 0; }
// ... and the plant step of tick t hands the vessel's state to the guidance layer when tick t + 1 is one
USV_HD bool cas_hands_over(long long tick, int ratio) { return cas_guidance_tick(tick + 1, ratio); }

// velocityCallback :179-182
USV_HD double cas_fix_u(double u) { return (u == 0.0) ? 0.001 : u; }

// ---- control :208-215: the low-level initial state from the vessel's state s [6] and the past thrusts
USV_HD void cas_ll_x0(const double *s, const double *past, double *x0)
{
    const double psi = s[2];
    x0[0] = psi; x0[1] = sin(psi); x0[2] = cos(psi);
    x0[3] = cas_fix_u(s[3]); x0[4] = s[4]; x0[5] = s[5];
    x0[6] = past[0]; x0[7] = past[1];
}

// ---- control :221-239: the reference row (psi_des, sin, cos, u_des, 0 ...); yref_e is its first CAS_NX entries
struct CasRef {
    double psi, s, c, u;
};
USV_HD CasRef cas_ref(double psi_des, double u_des)
{
    CasRef r;
    r.psi = psi_des; r.s = sin(psi_des); r.c = cos(psi_des); r.u = u_des;
    return r;
}
USV_HD double cas_yref_entry(int j, const CasRef &r) { return j == 0 ? r.psi : j == 1 ? r.s : j == 2 ? r.c : j == 3 ? r.u : 0.0; }

// the rows are rewritten only when the set-points' bits differ from what was last written (last [2]; NaN payloads of the reset never match
// a published set-point's bits)
USV_HD bool cas_ref_changed(const double *last, double psi_des, double u_des)
{
    return cas_bits(last[0]) != cas_bits(psi_des) || cas_bits(last[1]) != cas_bits(u_des);
}
constexpr unsigned long long CAS_NEVER = 0x7ff8dead00000001ull; // (a quiet NaN no arithmetic produces: "nothing written yet")
USV_HD double cas_never()
{
    const unsigned long long b = CAS_NEVER;
    double v;
    __builtin_memcpy(&v, &b, sizeof v);
    return v;
}

// ---- control :256-279 from stage 1 of the low-level iterate: the published thrusts thr [2], the past thrusts, the two errors
USV_HD void cas_ll_outputs(const double *x1, double psi_des, double u_des, double psi, double u_cb, double *thr, double *past, float &e_u,
                           float &e_psi)
{
    thr[0] = x1[6]; thr[1] = x1[7];
    if (u_des == 0.0) { thr[0] = 0.0; thr[1] = 0.0; }
    past[0] = x1[6]; past[1] = x1[7];
    e_u = (float)(u_des - u_cb);
    e_psi = (float)(psi_des - psi);
}

// ---- the vessel: x = s [6], U = (Tport, Tstbd, c)
struct CasVessel {
    static constexpr int NX = CAS_NS, NU = 3;
    USV_DEV static void fjvp(const double *x, const double *U, const double *s, const double *, double *f, double *js)
    {
        const double psi = x[2], u = x[3], v = x[4], r = x[5];
        double sp, cp, f3[3], j3[3];
        sincos(psi, &sp, &cp);
        Dof3::eval(U[2], u, v, r, U[0], U[1], s[3], s[4], s[5], 0.0, 0.0, f3, j3);
        f[0] = u * cp - v * sp;
        f[1] = u * sp + v * cp;
        f[2] = r;
        f[3] = f3[0]; f[4] = f3[1]; f[5] = f3[2];
        // (the plant is never linearised: erk_period<CasVessel, false> hands in a zero tangent and drops what comes back)
        js[0] = 0.0; js[1] = 0.0; js[2] = s[5]; js[3] = j3[0]; js[4] = j3[1]; js[5] = j3[2];
    }
};

// one period T of the vessel under the held thrusts, `steps` RK4 steps; s in place
USV_DEV void cas_plant_period(double *s, const double *thr, double c, double T, int steps)
{
    double U[3] = {thr[0], thr[1], c}, z[CAS_NS], zu[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < CAS_NS; i++) z[i] = 0.0;
    erk_period<CasVessel, false>(s, U, z, zu, T, steps);
}

// ---- what the two kernels need beside the guidance handle's own buffers (usvmpc_cascade_create)
struct CascadePtrs {
    // the low-level solver, in ITS library: reached by the device pointers usvmpc_get_device_ptr hands out, never by a handle
    double *ll_x0;        // [B][8]
    const double *ll_x;   // [B][ll_N + 1][8]
    double *ll_yref;      // [B][ll_N][10]
    double *ll_yref_e;    // [B][8]
    int ll_N;
    // the cascade's own state
    double *s;            // [B][6] vessel
    double *thr;          // [B][2] published thrusts
    double *past;         // [B][2] past thrusts
    double *last;         // [B][2] the (psi_des, u_des) the reference rows hold
    int *ticks;           // [B]
    double *sums;         // [B][4] sum |e_u|, sum |e_psi|, sum e_u^2, sum e_psi^2
    unsigned long long *yref_writes;
};

// ---- the arguments of usv_cascade_record (usvmpc.hip; the schedule and layout: cascade_log_plan.hpp).  Nothing in here is indexed at run
// time - the selected states are a nibble list (closed_loop_log.hpp) - so that the kernel needs no scratch.
struct CasLogRec {
    const double *s, *last, *ll_x;     // CascadePtrs' s, last and ll_x
    const int *ll_status, *ll_qp_iter; // [B] of the low-level solver (its library's device pointers); read only when r_status is set
    const int *g_status, *g_qp_iter;   // [B] of the guidance handle
    double *r_state, *r_thrust, *r_ref; // the record's slabs [B][nsel], [B][2], [B][2]; nullptr: channel not recorded
    float *r_err;                      // [B][2]
    int *r_status;                     // [B]
    long B;
    int ll_N, nsel;
    unsigned long long sel;            // nibble list: the selected states, ascending
};

} // namespace usv
