// obstacle_tracks.hpp — the arithmetic of the obstacle tracks (usvmpc.hip: usv_obstacle_predict, usv_obstacle_step; include/usvmpc.h:
// fields "obs_pos" / "obs_vel", option "obstacle_tracks"), as pure functions: host + device, no dependency on the kernels
// (tests/obstacle_tracks_harness.cpp).
//
// A track is a position and a constant velocity per obstacle slot.  The three operations:
//     predict   p[k]      = pos + ((double)k * dt) * vel          the obstacle set of stage k (what scenario.make_batch writes on the host)
//     step      pos      <- pos + T * vel                          the world moves on by T
//     clearance             min over slots of  sqrt((X - ox)^2 + (Y - oy)^2) - lh
// Every product and every sum is rounded on its own - NO fused multiply-add - so that the device's p is, bit for bit, the array numpy makes
// from the same expression (a host that rebuilds p and a handle that derives it hand the QP the same bits).  HIP's __dmul_rn / __dadd_rn are
// plain `*` / `+` in this toolchain and contract once inlined, hence the pragma; a host compiler must not contract either (x86-64 without
// FMA cannot; otherwise -ffp-contract=off).
#pragma once

#include <cmath>

#ifndef USV_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define USV_HD __host__ __device__ inline
#else
#define USV_HD inline
#endif
#endif

namespace usv {

USV_HD double track_mul(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a * b;
}

USV_HD double track_add(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a + b;
}

// one entry of p at stage k (pos, vel: the same coordinate of the same slot)
USV_HD double track_predict(double pos, double vel, int k, double dt) { return track_add(pos, track_mul(track_mul((double)k, dt), vel)); }

// one entry of obs_pos after a world step of T
USV_HD double track_step(double pos, double vel, double T) { return track_add(pos, track_mul(T, vel)); }

// distance from (X, Y) to the nearest keep-out circle of one instance: pos [2K] = (ox, oy) pairs, lh [K]; K = 0: 1e300
USV_HD double track_clearance(double X, double Y, const double *pos, const double *lh, int K)
{
    double c = 1e300;
    for (int i = 0; i < K; i++) {
        const double dx = track_add(X, -pos[2 * i]), dy = track_add(Y, -pos[2 * i + 1]);
        const double d = track_add(sqrt(track_add(track_mul(dx, dx), track_mul(dy, dy))), -lh[i]);
        c = d < c ? d : c;
    }
    return c;
}

} // namespace usv
