// pf_guidance.hpp — the arithmetic either side of the solver call in the reference's path-following ROS node (class NMPC,
// catkin_ws/src/nmpc_ca/src/nmpc_pf.cpp; nmpc_pf_ca.cpp is the same file), per instance, as pure functions: host + device, no dependency on
// the kernels (usvmpc.hip: usv_pf_prepare, usv_pf_publish; tests/pf_frontend_harness.cpp).  Model usv_model_pf_ca, state order
// (psi, sinpsi, cospsi, u, v, r, ye, x1, y1, ak, nedx, nedy, Tport, Tstbd).
//     input side    velocityCallback :198-206, waypoint_manager :226-268, control :273-335
//     output side   control :347-376
//     new list      main :392-401 (k = 1)
// The node has no obstacle callback; the obstacle side is this project's: nearest-K selection in the NED frame, in double precision (the
// simulator's NED -> body transform followed by a node's body -> NED one is the identity up to float32 rounding), the visibility test of
// catkin_ws/src/simulation/scripts/obstacle_sim_node.py:71 and lh = (R + boat radius) + margin of scripts/usv_pf_ca/main.py:126.
// Every product and every sum is rounded on its own - no fused multiply-add (as obstacle_tracks.hpp: the pragma on the device and under
// clang, -ffp-contract=off for another host compiler) - so that whatever does not pass through sin / cos / atan2 is the same bits on host
// and device.
// The pipelined lineariser: a prepare counts as a caller write of yref (whether a reference changed is known on the device only), so a
// handle driven by this front end linearises inside its solves.  Keeping the pipeline alive through ticks without a change is out of scope.
#pragma once

#include <cmath>

#include "obstacle_tracks.hpp"

#ifndef USV_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define USV_HD __host__ __device__ inline
#else
#define USV_HD inline
#endif
#endif

#if defined(__clang__)
#define USV_PF_NOFMA _Pragma("clang fp contract(off)")
#else
#define USV_PF_NOFMA
#endif

namespace usv {

constexpr int PF_LMAX = 64;            // world obstacles per instance (GUIDANCE_LMAX)
constexpr double PF_BOAT_RADIUS = 0.5; // (nmpc_guidance_ca1.cpp:139: the node of this family that has obstacles)
constexpr double PF_FAR = 1000.0;      // an unused obstacle slot sits at (1000, 1000), lh 0
constexpr double PF_SPEED = 0.7;       // :241-242
constexpr int PF_NX = 14, PF_NY = 16;

enum { PF_OVER = 0, PF_ACTIVE = 1, PF_SWITCH = 2 };

// device buffers of the front end (usvmpc.hip: the handle owns them)
struct PfPtrs {
    const double *wp;    // [B][2*npts]
    int npts;
    const double *world; // [B][nworld][3] NED (X, Y, R)
    int nworld;
    double max_radius, margin;
    const double *wvel;  // [B][nworld][2] NED m/s: the world moves and prepare writes every stage; null: a world at rest (stage 0 only)
    double *trk_pv;      // [B][K][4] (X, Y, vX, vY) } the slot tracks of the last moving prepare: written by its decide step,
    double *trk_lh;      // [B][K]                   } read by its streaming step
    const double *vel;   // [B][3] u, v, r     } host-fed; both null: the vessel's state is read from the handle's x0
    const double *pose;  // [B][3] nedx, nedy, psi
    int *k, *phase, *finish_tick; // [B] state: waypoint index, PF_* of the last prepare, tick of the first PF_OVER prepare (-1: none yet)
    double *past;        // [B][2] thrust of the last published tick (host-fed mode reads it)
    double *last;        // [B][3] (sin ak, cos ak, u_des) of the instance's last yref rewrite (NaN: none that still stands)
    double *u, *ye;      // [B] of the last active prepare (the errors publish reports)
    double *min_clear;   // [B]
    unsigned long long *yref_writes; // [1]
    double *thr_port, *thr_stbd, *Tx, *Tz, *speed; // [B] published
    float *e_u, *e_ye;
    int *active;
    double *min_sep;     // [B] smallest distance to a vessel of the instance's scene (fleet_world.hpp; 1e300 after a reset)
    int *sep_tick;       // [B] the prepare it was met at (-1: none yet)
    int *chosen;         // [B][K] exchanged plans (fleet_plan.hpp): the list index behind each slot of this prepare, -1 for a parked one and
                         // for every slot of an instance that does not stream; null: plans are off and nothing is recorded
};

// velocityCallback :201-203
USV_HD double pf_fix_u(double u) { return u == 0.0 ? 0.001 : u; }

struct PfSegment {
    double x1, y1, ak, ye, sin_ak, cos_ak, u_des;
};

// waypoint_manager :226-268 for waypoint index k (wp: [2 * npts]).  PF_ACTIVE: the segment's fields are filled; PF_SWITCH: the caller
// advances k and does nothing else this tick (:252-256); PF_OVER: k >= npts.
USV_HD int pf_waypoint(const double *wp, int npts, int k, double nedx, double nedy, PfSegment &s)
{
    USV_PF_NOFMA
    if (k >= npts) { s.u_des = 0.0; return PF_OVER; }
    const double x1 = wp[2 * k - 2], y1 = wp[2 * k - 1], x2 = wp[2 * k], y2 = wp[2 * k + 1];
    const double dx = x2 - nedx, dy = y2 - nedy;
    const double distance = sqrt(dx * dx + dy * dy); // :237-239
    s.u_des = PF_SPEED;
    if (!(distance > 1)) return PF_SWITCH;
    s.x1 = x1; s.y1 = y1;
    s.ak = atan2(y2 - y1, x2 - x1);                  // :245
    s.sin_ak = sin(s.ak); s.cos_ak = cos(s.ak);      // :246-247
    s.ye = -(nedx - x1) * s.sin_ak + (nedy - y1) * s.cos_ak; // :248-249
    return PF_ACTIVE;
}

// control :273-291: the initial state
USV_HD void pf_x0(double psi, double u, double v, double r, const PfSegment &s, double nedx, double nedy, double past_port, double past_stbd,
                  double *x0)
{
    USV_PF_NOFMA
    const double beta = atan2(v, u + .001);
    const double chi = psi + beta;
    x0[0] = psi; x0[1] = sin(chi); x0[2] = cos(chi); x0[3] = u; x0[4] = v; x0[5] = r; x0[6] = s.ye; x0[7] = s.x1; x0[8] = s.y1;
    x0[9] = s.ak; x0[10] = nedx; x0[11] = nedy; x0[12] = past_port; x0[13] = past_stbd;
}

// ---- the reference rows (:299-335): yref_k = [0, sin ak, cos ak, u_des, 0 ...] for every stage, yref_e its first 14 entries.  The node rewrites
// them every tick; here an instance's rows are rewritten only when the triple it last wrote differs, bit for bit, from the tick's.
USV_HD bool pf_same_bits(double a, double b)
{
    unsigned long long x, y;
    __builtin_memcpy(&x, &a, 8);
    __builtin_memcpy(&y, &b, 8);
    return x == y;
}

// last: (sin ak, cos ak, u_des) of the instance's last rewrite; stale: the caller may have written yref since
USV_HD bool pf_yref_write(int phase, bool stale, const double *last, const PfSegment &s)
{
    if (phase != PF_ACTIVE) return false;
    return stale || !pf_same_bits(last[0], s.sin_ak) || !pf_same_bits(last[1], s.cos_ak) || !pf_same_bits(last[2], s.u_des);
}

// entry j (0 .. 15) of a reference row
USV_HD double pf_yref_entry(int j, double sin_ak, double cos_ak, double u_des) { return j == 1 ? sin_ak : j == 2 ? cos_ak : j == 3 ? u_des : 0.0; }

// ---- obstacles.  World entry (X, Y, R): visible when closer than max_radius (strictly: obstacle_sim_node.py:71); ranked by the distance
// to its keep-out circle d = distance - (R + boat radius).
USV_HD bool pf_obstacle_d(double X, double Y, double R, double nedx, double nedy, double max_radius, double &d)
{
    USV_PF_NOFMA
    const double dx = X - nedx, dy = Y - nedy;
    const double dist = sqrt(dx * dx + dy * dy);
    d = dist - (R + PF_BOAT_RADIUS);
    return dist < max_radius;
}

USV_HD double pf_lh(double R, double margin)
{
    USV_PF_NOFMA
    return (R + PF_BOAT_RADIUS) + margin;
}

// The selection over the world list w ([L][3]): the K visible obstacles with the smallest d, ties by list index.  d: scratch of L entries,
// entry i at d[i * stride] (the kernel keeps it in LDS, one column per lane).  place(slot, i): list entry i takes slot `slot` (each slot
// at most once, in list order, not in slot order).  Returns the smallest d (1e300: nothing visible).
template <class Place>
USV_HD double pf_rank(const double *w, int L, int K, double nedx, double nedy, double max_radius, double *d, int stride, Place place)
{
    double dmin = 1e300;
    for (int i = 0; i < L; i++) {
        double di;
        const bool vis = pf_obstacle_d(w[3 * i], w[3 * i + 1], w[3 * i + 2], nedx, nedy, max_radius, di);
        d[i * stride] = vis ? di : HUGE_VAL; // (an invisible one ranks behind every visible one and is never placed)
        if (vis && di < dmin) dmin = di;
    }
    for (int i = 0; i < L; i++) {
        const double di = d[i * stride];
        if (di == HUGE_VAL) continue;
        int rank = 0;
        for (int j = 0; j < L; j++) {
            const double dj = d[j * stride];
            rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
        }
        if (rank < K) place(rank, i);
    }
    return dmin;
}

// Stage 0 of p ([2K]) and lh ([K]) from the world list: the chosen ones in rank order, the rest of the slots parked.
// chosen (optional, [K]): the list index behind each slot, -1 for a parked one.
USV_HD double pf_select(const double *w, int L, int K, double nedx, double nedy, double max_radius, double margin, double *d, int stride,
                        double *p, double *lh, int *chosen)
{
    for (int i = 0; i < K; i++) {
        p[2 * i] = PF_FAR; p[2 * i + 1] = PF_FAR; lh[i] = 0.0;
        if (chosen) chosen[i] = -1;
    }
    return pf_rank(w, L, K, nedx, nedy, max_radius, d, stride, [&](int slot, int i) {
        p[2 * slot] = w[3 * i]; p[2 * slot + 1] = w[3 * i + 1]; // (the world's coordinates, bit for bit)
        lh[slot] = pf_lh(w[3 * i + 2], margin);
        if (chosen) chosen[slot] = i;
    });
}

// ---- a moving world: list entry i also has a constant velocity wv[i] = (vX, vY), NED m/s.  The selection is the same, on the current
// positions; each slot gets a TRACK instead of a point - pv [K][4] = (X, Y, vX, vY), lh [K]; a parked slot (1000, 1000) with velocity 0 and
// lh 0 - from which every stage follows (obstacle_tracks.hpp: the tracks' arithmetic, not a second copy of it):
//     p[k][2 slot + c] = track_predict(pv[slot][c], pv[slot][2 + c], k, dt)   k = 0 .. N   (stage 0: the world's coordinates, (0 dt) v = 0;
//     lh[k][slot]      = lh[slot]                                             k = 0 .. N-1  a parked slot: 1000.0 at every stage)
// and the world moves on by T with track_step, R untouched.
USV_HD double pf_select_tracks(const double *w, const double *wv, int L, int K, double nedx, double nedy, double max_radius, double margin,
                               double *d, int stride, double *pv, double *lh, int *chosen)
{
    for (int i = 0; i < K; i++) {
        pv[4 * i] = PF_FAR; pv[4 * i + 1] = PF_FAR; pv[4 * i + 2] = 0.0; pv[4 * i + 3] = 0.0; lh[i] = 0.0;
        if (chosen) chosen[i] = -1;
    }
    return pf_rank(w, L, K, nedx, nedy, max_radius, d, stride, [&](int slot, int i) {
        pv[4 * slot] = w[3 * i]; pv[4 * slot + 1] = w[3 * i + 1]; pv[4 * slot + 2] = wv[2 * i]; pv[4 * slot + 3] = wv[2 * i + 1];
        lh[slot] = pf_lh(w[3 * i + 2], margin);
        if (chosen) chosen[slot] = i;
    });
}

// coordinate c (0, 1) of a slot's track (pv: its four entries) at stage k
USV_HD double pf_stage(const double *pv, int c, int k, double dt) { return track_predict(pv[c], pv[2 + c], k, dt); }

// one world entry w = (X, Y, R) with velocity wv = (vX, vY) after a step of T
USV_HD void pf_world_step(double *w, const double *wv, double T)
{
    w[0] = track_step(w[0], wv[0], T);
    w[1] = track_step(w[1], wv[1], T);
}

// ---- output side, control :347-376, for an instance whose tick was PF_ACTIVE: the thrusters are x_1's (the thrust is a state), the errors
// `float` as in the node, and the node's own mixing constants 0.78 and 0.41 / 2 although this model's c is 1.0.  (The test `u_des == 0.0` of
// :352-355 never holds: control() is called with u_des = 0.7 only.)
struct PfOutputs {
    double thr_port, thr_stbd, Tx, Tz, speed;
    float e_u, e_ye;
};

USV_HD void pf_publish(double x1_port, double x1_stbd, double u_des, double u, double ye, PfOutputs &o)
{
    USV_PF_NOFMA
    o.thr_port = x1_port; o.thr_stbd = x1_stbd;
    o.e_u = (float)(u_des - u);                        // :362
    o.e_ye = (float)(0.0 - ye);                        // :363
    o.Tx = x1_port + 0.78 * x1_stbd;                   // :372
    o.Tz = (x1_port - 0.78 * x1_stbd) * 0.41 / 2;      // :373
    o.speed = PF_SPEED;                                // :241, :370
}

} // namespace usv
