// ca_fleet_world.hpp — vessel encounters for the guidance front end (model usv_model_guidance_ca1, state order (u, v, ye, chie, psied, xned,
// yned, psi)): the batch is cut into SCENES of S consecutive instances, the scene's vessels sail in one world, and every instance sees the
// other S - 1 vessels of its scene as moving world entries behind the caller's own n_fixed ones.  Scenes, slots and the list's layout are
// those of fleet_world.hpp (fleet_vessel, fleet_slots, fleet_scene_ok, fleet_fits, fleet_radius_ok, fleet_closest, fleet_relayout), which
// do not depend on the model; this header adds what does.  Pure functions, host + device, no dependency on the kernels (usvmpc.hip:
// usv_guidance_fleet_gather, usvmpc_guidance_fleet; tests/ca_fleet_world_harness.cpp).
//     entry         X = x0_j[5], Y = x0_j[6], R = radius
//     velocity      vX = u cos psi - v sin psi, vY = u sin psi + v cos psi with u, v = x0_j[0], x0_j[1] and psi = x0_j[7]: this model's
//                   state carries the heading, not its sine and cosine, so each is evaluated once, in double
//     separation    d = sqrt(dx dx + dy dy) between the two vessels' positions; per instance the running minimum over its scene-mates
//                   and the tick it was met at
// Every product and every sum is rounded on its own - no fused multiply-add (track_mul / track_add of obstacle_tracks.hpp) - so positions,
// radius and separations are the bits numpy makes from the same expressions.  The velocities are those bits only as far as the two libraries'
// sin / cos agree: with 4 ulp each (OpenCL's bound for the device's) and three separately rounded operations,
// |vX - numpy's| and |vY - numpy's| <= 8 * 2^-52 * (|u| + |v|).
#pragma once

#include <cmath>

#include "fleet_world.hpp"
#include "obstacle_tracks.hpp"

namespace usv {

constexpr int CA_FLEET_NX = 8; // (CA_NX)

// world entry w = (X, Y, R) and velocity wv = (vX, vY) of the vessel whose state is xj
USV_HD void ca_fleet_entry(const double *xj, double radius, double *w, double *wv)
{
    const double u = xj[0], v = xj[1];
    double s, c;
    sincos(xj[7], &s, &c); // (one argument reduction for both: see profiles/guidance_fleet_resources.txt)
    w[0] = xj[5]; w[1] = xj[6]; w[2] = radius;
    wv[0] = track_add(track_mul(u, c), -track_mul(v, s));
    wv[1] = track_add(track_mul(u, s), track_mul(v, c));
}

// distance between the vessels whose states are xi and xj
USV_HD double ca_fleet_separation(const double *xi, const double *xj)
{
    const double dx = track_add(xj[5], -xi[5]), dy = track_add(xj[6], -xi[6]);
    return sqrt(track_add(track_mul(dx, dx), track_mul(dy, dy)));
}

// this model for the gather written once for both (fleet_world.hpp: PfFleet)
struct CaFleet {
    static constexpr int NX = CA_FLEET_NX;
    static constexpr int PX = 5, PY = 6; // the position pair of a state (fleet_plan.hpp)
    static USV_HD void entry(const double *xj, double radius, double *w, double *wv) { ca_fleet_entry(xj, radius, w, wv); }
    static USV_HD double separation(const double *xi, const double *xj) { return ca_fleet_separation(xi, xj); }
};

// One instance's gather, as the kernel's lanes do it between them: the S - 1 fleet entries behind the n_fixed fixed ones of its world list
// w ([nworld][3]) / wv ([nworld][2]) and the separation bookkeeping.  x0: the whole batch's states [B][8].
USV_HD void ca_fleet_gather(const double *x0, long i, int S, int n_fixed, double radius, int tick, double *w, double *wv, double &min_separation,
                            int &separation_tick)
{
    for (int e = 0; e < S - 1; e++) {
        const double *xj = x0 + fleet_vessel(i, e, S) * CA_FLEET_NX;
        ca_fleet_entry(xj, radius, w + 3 * (n_fixed + e), wv + 2 * (n_fixed + e));
        fleet_closest(ca_fleet_separation(x0 + i * CA_FLEET_NX, xj), tick, min_separation, separation_tick);
    }
}

} // namespace usv
