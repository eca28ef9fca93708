// fleet_world.hpp — vessel encounters for the path-following front end (model usv_model_pf_ca): the batch is cut into SCENES of S consecutive
// instances (scene s: instances s S .. s S + S - 1), the scene's vessels sail in one world, and every instance sees the other S - 1 vessels
// of its scene as moving world entries behind the caller's own n_fixed ones.  Pure functions, host + device, no dependency on the kernels
// (usvmpc.hip: usv_pf_fleet_gather, usvmpc_pf_fleet; tests/fleet_world_harness.cpp).
//     world list of instance i = s S + a     [ fixed 0 .. n_fixed - 1 | fleet slot e = 0 .. S - 2 ]
//     fleet slot e holds vessel              j = s S + (e < a ? e : e + 1)       (the scene's vessels in order, the instance itself left out)
//     entry                                  X = x0_j[10], Y = x0_j[11], R = radius
//     velocity                               sog = sqrt(u u + v v), (vX, vY) = (sog cos chi, sog sin chi) with u, v = x0_j[3], x0_j[4] and
//                                            sin chi, cos chi = x0_j[1], x0_j[2]: the model's own states (pf_x0), carried by the plant
//     separation                             d = sqrt(dx dx + dy dy) between the two vessels' positions; per instance the running minimum
//                                            over its scene-mates and the tick it was met at
// No trigonometric call is made, and every product and every sum is rounded on its own - no fused multiply-add (as pf_guidance.hpp: the
// pragma on the device and under clang, -ffp-contract=off for another host compiler) - so numpy gives the same bits.
#pragma once

#include <cmath>

#ifndef USV_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define USV_HD __host__ __device__ inline
#else
#define USV_HD inline
#endif
#endif

#if defined(__clang__)
#define USV_FLEET_NOFMA _Pragma("clang fp contract(off)")
#else
#define USV_FLEET_NOFMA
#endif

namespace usv {

constexpr int FLEET_LMAX = 64; // world entries per instance, fixed and fleet together (PF_LMAX)
constexpr int FLEET_NX = 14;   // (PF_NX)
constexpr double FLEET_FAR = 1000.0; // a fleet slot is parked at (1000, 1000, 0), velocity 0, until the first gather (PF_FAR)

// ---- what usvmpc_pf_fleet refuses
USV_HD bool fleet_on(int scene_size) { return scene_size >= 2; }
USV_HD int fleet_slots(int scene_size) { return fleet_on(scene_size) ? scene_size - 1 : 0; }
USV_HD bool fleet_scene_ok(long B, int scene_size) { return scene_size >= 0 && (!fleet_on(scene_size) || B % scene_size == 0); }
USV_HD bool fleet_fits(int n_fixed, int scene_size) { return n_fixed >= 0 && n_fixed + fleet_slots(scene_size) <= FLEET_LMAX; }
USV_HD bool fleet_radius_ok(double radius) { return radius - radius == 0.0 && radius >= 0.0; } // (finite and not negative)

// the vessel behind fleet slot e of instance i (scene size S): the scene's vessels in order, i itself left out
USV_HD long fleet_vessel(long i, int e, int S)
{
    const long a = i % S;
    return i - a + (e < a ? e : e + 1);
}

// world entry w = (X, Y, R) and velocity wv = (vX, vY) of the vessel whose state is xj
USV_HD void fleet_entry(const double *xj, double radius, double *w, double *wv)
{
    USV_FLEET_NOFMA
    const double sog = sqrt(xj[3] * xj[3] + xj[4] * xj[4]);
    w[0] = xj[10]; w[1] = xj[11]; w[2] = radius;
    wv[0] = sog * xj[2];
    wv[1] = sog * xj[1];
}

// distance between the vessels whose states are xi and xj
USV_HD double fleet_separation(const double *xi, const double *xj)
{
    USV_FLEET_NOFMA
    const double dx = xj[10] - xi[10], dy = xj[11] - xi[11];
    return sqrt(dx * dx + dy * dy);
}

// this model for a gather written once for both front ends' models (usvmpc.hip: fleet_gather_body; ca_fleet_world.hpp: CaFleet)
struct PfFleet {
    static constexpr int NX = FLEET_NX;
    static constexpr int PX = 10, PY = 11; // the position pair of a state (fleet_plan.hpp)
    static USV_HD void entry(const double *xj, double radius, double *w, double *wv) { fleet_entry(xj, radius, w, wv); }
    static USV_HD double separation(const double *xi, const double *xj) { return fleet_separation(xi, xj); }
};

// the running minimum and the tick it was met at (a NaN never wins)
USV_HD void fleet_closest(double d, int tick, double &min_separation, int &separation_tick)
{
    if (d < min_separation) { min_separation = d; separation_tick = tick; }
}

// One instance's gather, as the kernel's lanes do it between them: the S - 1 fleet entries behind the n_fixed fixed ones of its world list
// w ([nworld][3]) / wv ([nworld][2]) and the separation bookkeeping.  x0: the whole batch's states [B][14].
USV_HD void fleet_gather(const double *x0, long i, int S, int n_fixed, double radius, int tick, double *w, double *wv, double &min_separation,
                         int &separation_tick)
{
    for (int e = 0; e < S - 1; e++) {
        const double *xj = x0 + fleet_vessel(i, e, S) * FLEET_NX;
        fleet_entry(xj, radius, w + 3 * (n_fixed + e), wv + 2 * (n_fixed + e));
        fleet_closest(fleet_separation(x0 + i * FLEET_NX, xj), tick, min_separation, separation_tick);
    }
}

// ---- the world list's layout when the fleet is switched, or the fixed entries are replaced: fixed entries first, fleet slots behind them.
// One instance: old list (w0, v0: n0_fixed fixed entries and f0 fleet slots; v0 null: at rest) -> new list (w1, v1: n1_fixed and f1).
//   fixed entries    positions from `fixed` ([n1_fixed][3]) when given, else the old ones (n1_fixed == n0_fixed then); velocities kept when the
//                    count is unchanged and the old world moved, else zero
//   fleet slots      slot e < min(f0, f1) is kept as it stands; a new one is parked with velocity 0
inline void fleet_relayout(const double *w0, const double *v0, int n0_fixed, int f0, const double *fixed, int n1_fixed, int f1, double *w1,
                           double *v1)
{
    for (int i = 0; i < n1_fixed; i++) {
        const double *src = fixed ? fixed + 3 * i : w0 + 3 * i;
        w1[3 * i] = src[0]; w1[3 * i + 1] = src[1]; w1[3 * i + 2] = src[2];
        const bool keep = v0 && n1_fixed == n0_fixed;
        v1[2 * i] = keep ? v0[2 * i] : 0.0;
        v1[2 * i + 1] = keep ? v0[2 * i + 1] : 0.0;
    }
    for (int e = 0; e < f1; e++) {
        double *w = w1 + 3 * (n1_fixed + e), *v = v1 + 2 * (n1_fixed + e);
        if (e < f0) {
            const double *ws = w0 + 3 * (n0_fixed + e);
            w[0] = ws[0]; w[1] = ws[1]; w[2] = ws[2];
            v[0] = v0 ? v0[2 * (n0_fixed + e)] : 0.0;
            v[1] = v0 ? v0[2 * (n0_fixed + e) + 1] : 0.0;
        } else {
            w[0] = FLEET_FAR; w[1] = FLEET_FAR; w[2] = 0.0;
            v[0] = 0.0; v[1] = 0.0;
        }
    }
}

} // namespace usv
