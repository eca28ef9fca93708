// ca_guidance.hpp — the arithmetic either side of the solver call in the reference's obstacle-avoidance ROS node (class NMPC,
// catkin_ws/src/nmpc_ca/src/nmpc_guidance_ca1.cpp) and of the obstacle simulator that feeds it (catkin_ws/src/simulation/scripts/
// obstacle_sim_node.py), per instance, as pure functions: host + device, no dependency on the kernels (guidance.hpp: usv_obstacle_sim,
// usv_guidance_pre, usv_guidance_post; usvmpc.hip: usv_guidance_tick; tests/ca_guidance_harness.cpp).  Model usv_model_guidance_ca1, state
// order (u, v, ye, chie, psied, nedx, nedy, psi).
//     simulator     simulate :56-81, ned_to_body :101-117 (the inverse rotation written out: adjugate / determinant)
//     input side    velocityCallback :223-230, obstaclesCallback :252-346, body2NED :348-363 (single-precision Eigen product),
//                   waypoint_manager :441-491, control :493-511
//     output side   control :583-600
//     new list      main :616-632
// Quirks of the node are kept: the float `past_psied` member (:156), the always-true enum test at :496 (beta = atan2(v, u)).
// Rounding.  Every sum of two products goes through ca_dot2 / ca_dot2f (below): unfused on the host, as the node computes it and bit for bit
// the CPU oracle; on the device the one fused form the kernels have always been compiled to, written out, so that the host-fed kernels keep
// the bits they returned before this header existed and the device-resident kernel returns the same ones.  Host and device therefore agree
// to rounding (and to the difference between two libms), not bit for bit.  The running minimum clearance and the moving world use the
// arithmetic of obstacle_tracks.hpp: never fused, the bits numpy makes from the same expression.  A host compiler other than clang needs
// -ffp-contract=off.
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

namespace usv {

constexpr int GUIDANCE_LMAX = 64;   // obstacles per instance on input
constexpr double BOAT_RADIUS = 0.5; // :139
constexpr double INIT_OBS_POS = 1000.0;
constexpr double D_SPEED = 0.7;     // :453
constexpr int CA_NX = 8;

// ---- a * b + c * d, the one shape in which this arithmetic meets a sum of products (the Eigen product of body2NED, the simulator's inverse
// rotation, the squared distances, ye).  The node rounds each product and the sum; so does the host build of this header.  The device
// kernels have been compiled, since they exist, to the form written out here: the SECOND product rounded, the first fused into the sum - and
// which product a compiler fuses depends on the code around the expression, so it is pinned (no contraction is left to the compiler in this
// header: every kernel that calls a function of it returns the same bits).
#if defined(__HIP_DEVICE_COMPILE__)
USV_HD double ca_dot2(double a, double b, double c, double d)
{
#pragma clang fp contract(off)
    return fma(a, b, c * d);
}
USV_HD float ca_dot2f(float a, float b, float c, float d)
{
#pragma clang fp contract(off)
    return fmaf(a, b, c * d);
}
#else
USV_HD double ca_dot2(double a, double b, double c, double d) { return track_add(track_mul(a, b), track_mul(c, d)); }
USV_HD float ca_dot2f(float a, float b, float c, float d)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float ab = a * b, cd = c * d;
    return ab + cd;
}
#endif

USV_HD double wrap_pi(double a)
{
    if (fabs(a) > M_PI) a = (a / fabs(a)) * (fabs(a) - 2.0 * M_PI);
    return a;
}
USV_HD float wrap_pi_f(float a)
{ // float variable, double arithmetic, rounded on assignment (as the node's float members)
    if (fabs((double)a) > M_PI) a = (float)(((double)a / fabs((double)a)) * (fabs((double)a) - 2.0 * M_PI));
    return a;
}

// velocityCallback :225-228
USV_HD double ca_fix_u(double u) { return (u == 0.0) ? 0.001 : u; }

// ---- the obstacle simulator: every world obstacle (X, Y, R) closer to the vessel than max_radius (strictly) is reported in the body frame
struct CaSensor {
    double nedx, nedy, i00, i01, i10, i11; // the pose and the inverse of the yaw rotation
};

USV_HD CaSensor ca_sensor(double nedx, double nedy, double yaw)
{
    const double c = cos(yaw), s = sin(yaw);
    const double det = ca_dot2(c, c, s, s); // c * c - (-s) * s
    CaSensor S;
    S.nedx = nedx; S.nedy = nedy;
    S.i00 = c / det; S.i01 = s / det; S.i10 = -s / det; S.i11 = c / det;
    return S;
}

// world entry w = (X, Y, R): visible -> true and out = body (x, y, R)
USV_HD bool ca_sense(const CaSensor &S, const double *w, double max_radius, double *out)
{
    const double dx = w[0] - S.nedx, dy = w[1] - S.nedy;
    const double dist = sqrt(ca_dot2(dx, dx, dy, dy));
    if (dist < max_radius) {
        out[0] = ca_dot2(S.i00, dx, S.i01, dy);
        out[1] = ca_dot2(S.i10, dx, S.i11, dy);
        out[2] = w[2];
        return true;
    }
    return false;
}

// simulate(): the visible entries of world [nw][3] in list order into out [lmax][3]; returns their number
USV_HD int ca_sense_list(double nedx, double nedy, double yaw, const double *world, int nw, double max_radius, double *out, int lmax)
{
    const CaSensor S = ca_sensor(nedx, nedy, yaw);
    int n = 0;
    for (int i = 0; i < nw && n < lmax; i++)
        if (ca_sense(S, world + 3 * i, max_radius, out + 3 * n)) n++;
    return n;
}

// ---- body2NED :348-363
USV_HD void body2ned(double psi, double nedx, double nedy, double bx, double by, double &ox, double &oy)
{ // Matrix3f * Vector3f, row i = (R_i0*b0 + R_i1*b1) + R_i2*b2
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float c = (float)cos(psi), s = (float)sin(psi);
    const float b0 = (float)bx, b1 = (float)by;
    const float r0 = ca_dot2f(c, b0, -s, b1) + 0.0f;
    const float r1 = ca_dot2f(c, b1, s, b0) + 0.0f;
    ox = (double)(float)((double)r0 + nedx);
    oy = (double)(float)((double)r1 + nedy);
}

// ---- obstaclesCallback :252-346
// what the nearest-K choice ranks by (:262-270): the distance to the keep-out circle, in the body frame
USV_HD double ca_rank_d(double bx, double by, double R) { return sqrt(ca_dot2(bx, bx, by, by)) - (R + BOAT_RADIUS); }

USV_HD double ca_lh(double R) { return (double)(float)(R + BOAT_RADIUS); }

// initializeObstacles :365-376
USV_HD void ca_park(double *p, double *lh, int K)
{
    for (int i = 0; i < K; i++) {
        p[2 * i] = (double)(float)INIT_OBS_POS;
        p[2 * i + 1] = (double)(float)INIT_OBS_POS;
        lh[i] = 0.0;
    }
}

// The choice over a list of L candidate entries.  entry(i, e): candidate i is on the node's list (for a body-frame list: always; for a world
// list: when the simulator reports it) and e = its body (x, y, R).  With n entries on the list: n <= K - list order; else the K smallest of
// ca_rank_d, ties by list index, each in the slot of its rank.  The distance is computed ONCE per entry into the scratch d, entry i at
// d[i * stride] (the kernels keep it in LDS, one column per lane; HUGE_VAL: not on the list); ranks come from comparisons.
// place(slot, i, ox, oy, lh): candidate i takes slot `slot` with the float32-rounded NED position (ox, oy) - each slot at most once, in list
// order, not in slot order.  Returns n.
template <class Entry, class Place>
USV_HD int ca_select(Entry entry, int L, int K, double psi, double nedx, double nedy, double *d, int stride, Place place)
{
    int n = 0;
    for (int i = 0; i < L; i++) {
        double e[3];
        const bool on = entry(i, e);
        d[i * stride] = on ? ca_rank_d(e[0], e[1], e[2]) : HUGE_VAL;
        n += on ? 1 : 0;
    }
    int ord = 0;
    for (int i = 0; i < L; i++) {
        const double di = d[i * stride];
        if (di == HUGE_VAL) continue;
        int slot = ord++;
        if (n > K) {
            slot = 0;
            for (int j = 0; j < L; j++) {
                const double dj = d[j * stride];
                slot += (dj < di || (dj == di && j < i)) ? 1 : 0;
            }
        }
        if (slot < K) {
            double e[3] = {0.0, 0.0, 0.0}, ox, oy;
            entry(i, e); // (again: the list is not kept)
            body2ned(psi, nedx, nedy, e[0], e[1], ox, oy);
            place(slot, i, ox, oy, ca_lh(e[2]));
        }
    }
    return n;
}

// stage 0 of p ([2K]) and lh ([K]) from the body-frame list ob [n][3]; chosen (optional, [K]): the list index behind each slot, -1: parked
USV_HD void ca_select_body(const double *ob, int n, int K, double psi, double nedx, double nedy, double *d, int stride, double *p, double *lh,
                           int *chosen)
{
    ca_park(p, lh, K);
    if (chosen)
        for (int i = 0; i < K; i++) chosen[i] = -1;
    ca_select([&](int i, double *e) { e[0] = ob[3 * i]; e[1] = ob[3 * i + 1]; e[2] = ob[3 * i + 2]; return true; }, n, K, psi, nedx, nedy, d, stride,
              [&](int slot, int i, double ox, double oy, double l) {
                  p[2 * slot] = ox; p[2 * slot + 1] = oy; lh[slot] = l;
                  if (chosen) chosen[slot] = i;
              });
}

// ... and straight from the world list w [L][3] at the pose: the simulator's list is never materialised.  chosen: world indices.
USV_HD int ca_select_world(const double *w, int L, int K, double psi, double nedx, double nedy, double max_radius, double *d, int stride, double *p,
                           double *lh, int *chosen)
{
    const CaSensor S = ca_sensor(nedx, nedy, psi);
    ca_park(p, lh, K);
    if (chosen)
        for (int i = 0; i < K; i++) chosen[i] = -1;
    return ca_select([&](int i, double *e) { return ca_sense(S, w + 3 * i, max_radius, e); }, L, K, psi, nedx, nedy, d, stride,
                     [&](int slot, int i, double ox, double oy, double l) {
                         p[2 * slot] = ox; p[2 * slot + 1] = oy; lh[slot] = l;
                         if (chosen) chosen[slot] = i;
                     });
}

// ... as TRACKS for a moving world (wv [L][2] NED m/s): pv [K][4] = (X, Y, vX, vY) with (X, Y) the float32-rounded position above, lh [K]; a
// parked slot (1000, 1000), velocity 0, lh 0.  Every stage follows with track_predict (obstacle_tracks.hpp): ca_stage.
USV_HD int ca_select_tracks(const double *w, const double *wv, int L, int K, double psi, double nedx, double nedy, double max_radius, double *d,
                            int stride, double *pv, double *lh, int *chosen)
{
    const CaSensor S = ca_sensor(nedx, nedy, psi);
    for (int i = 0; i < K; i++) {
        pv[4 * i] = (double)(float)INIT_OBS_POS; pv[4 * i + 1] = (double)(float)INIT_OBS_POS; pv[4 * i + 2] = 0.0; pv[4 * i + 3] = 0.0; lh[i] = 0.0;
        if (chosen) chosen[i] = -1;
    }
    return ca_select([&](int i, double *e) { return ca_sense(S, w + 3 * i, max_radius, e); }, L, K, psi, nedx, nedy, d, stride,
                     [&](int slot, int i, double ox, double oy, double l) {
                         pv[4 * slot] = ox; pv[4 * slot + 1] = oy; pv[4 * slot + 2] = wv[2 * i]; pv[4 * slot + 3] = wv[2 * i + 1]; lh[slot] = l;
                         if (chosen) chosen[slot] = i;
                     });
}

// coordinate c (0, 1) of a slot's track (pv: its four entries) at stage k
USV_HD double ca_stage(const double *pv, int c, int k, double dt) { return track_predict(pv[c], pv[2 + c], k, dt); }

// one world entry w = (X, Y, R) with velocity wv = (vX, vY) after a step of T
USV_HD void ca_world_step(double *w, const double *wv, double T)
{
    w[0] = track_step(w[0], wv[0], T);
    w[1] = track_step(w[1], wv[1], T);
}

// distance from the pose to the keep-out circle of world entry (X, Y, R): sqrt(dx^2 + dy^2) - (R + 0.5), squares and sum rounded one by one
USV_HD double ca_clearance(double X, double Y, double R, double nedx, double nedy)
{
    const double dx = track_add(nedx, -X), dy = track_add(nedy, -Y);
    return track_add(sqrt(track_add(track_mul(dx, dx), track_mul(dy, dy))), -track_add(R, BOAT_RADIUS));
}

// the smallest ca_clearance over the entries the scratch of a ca_select over the same list marks as visible (1e300: none)
USV_HD double ca_min_clearance(const double *w, int L, double nedx, double nedy, const double *d, int stride)
{
    double c = 1e300;
    for (int i = 0; i < L; i++) {
        if (d[i * stride] == HUGE_VAL) continue;
        const double ci = ca_clearance(w[3 * i], w[3 * i + 1], w[3 * i + 2], nedx, nedy);
        c = ci < c ? ci : c;
    }
    return c;
}

// ---- main :616-632: a new waypoint list w ([2 npts])
USV_HD void ca_reset(const double *w, double psi, int &k, float &past_psied)
{
    const double ak = atan2(w[3] - w[1], w[2] - w[0]);
    k = 1;
    past_psied = wrap_pi_f((float)(psi - ak));
}

// ---- waypoint_manager :441-491 for waypoint index k (w: [2 npts]).  active: the tick is a control tick (ak, ye valid); the `float`
// past_psied is re-referenced at a segment switch; k >= npts on return: the mission is over.
USV_HD void ca_waypoint(const double *w, int npts, double nedx, double nedy, int &k, float &pp, int &active, double &ak, double &ye)
{
    active = 0;
    ak = 0.0; ye = 0.0;
    if (k < npts) {
        double x1 = w[2 * k - 2], y1 = w[2 * k - 1], x2 = w[2 * k], y2 = w[2 * k + 1];
        const double distance = sqrt(ca_dot2(x2 - nedx, x2 - nedx, y2 - nedy, y2 - nedy));
        ak = atan2(y2 - y1, x2 - x1);
        active = 1;
        if (distance > 1) {
            ye = ca_dot2(nedy - y1, cos(ak), -(nedx - x1), sin(ak)); // -(nedx - x1) * sin(ak) + (nedy - y1) * cos(ak)
        } else {
            k += 1;
            if (k < npts) {
                x1 = w[2 * k - 2]; y1 = w[2 * k - 1]; x2 = w[2 * k]; y2 = w[2 * k + 1];
                const double ak2 = atan2(y2 - y1, x2 - x1);
                ye = ca_dot2(nedy - y1, cos(ak2), -(nedx - x1), sin(ak2));
                pp = wrap_pi_f((float)((double)pp - ak2 + ak));
                ak = ak2;
            } else {
                active = 0;
            }
        }
    }
}

// ---- control :493-511: the initial state
USV_HD void ca_x0(double u_cb, double v_cb, double ye, double psi, double ak, float pp, double nedx, double nedy, double *x0)
{
    const double beta = atan2(v_cb, u_cb);
    x0[0] = u_cb; x0[1] = v_cb; x0[2] = ye; x0[3] = wrap_pi(psi + beta - ak); x0[4] = (double)pp;
    x0[5] = nedx; x0[6] = nedy; x0[7] = psi;
}

// ---- control :583-600: the published set-points of an active tick
USV_HD void ca_publish(double x1_psied, double ak, double u0, float &past_psied, double &heading, double &rdes, double &speed)
{
    const float psid = wrap_pi_f((float)(x1_psied + ak));
    past_psied = (float)x1_psied;
    heading = (double)psid;
    rdes = u0;
    speed = D_SPEED;
}

// ---- the device-resident tick (usvmpc.hip: usv_guidance_tick; usvmpc_guidance_world): what it needs beside the front end's own buffers
struct CaTickPtrs {
    const double *world; // [B][nworld][3] NED (X, Y, R)
    int nworld;
    double max_radius;
    const double *wvel;  // [B][nworld][2] NED m/s: the world moves and is predicted - the tick writes every stage; null: stage 0 only
    double *trk_pv;      // [B][K][4] } the slot tracks of a predicted tick: written by its decide step, read by its streaming step
    double *trk_lh;      // [B][K]    }
    double *min_clear;   // [B] running minimum of ca_min_clearance
    int *finish_tick;    // [B] tick of the first prepare that found the mission over (-1: none yet)
    int tick;
    int *chosen;         // [B][K] exchanged plans (fleet_plan.hpp): the list index behind each slot of this tick, -1 for a parked one and for
                         // every slot of an instance that does not stream; null: plans are off and nothing is recorded
};

} // namespace usv
