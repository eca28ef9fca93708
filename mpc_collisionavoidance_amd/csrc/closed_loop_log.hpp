// closed_loop_log.hpp — the arithmetic of the closed-loop log (usvmpc.hip: usv_log_record; include/usvmpc.h: usvmpc_log_*), as pure
// functions: host + device, no dependency on the kernels (tests/closed_loop_log_harness.cpp).
//
//     error       e        = x0[a] - rhs,   rhs = x0[b] or a constant     (scripts/usv_pf_ca/main.py: psi - ak, u - u_ref, ye)
//     accumulate  sum_abs += |e|,  sum_sq += e e                           one step per hand-over, in tick order
//     selection   the recorded states as a list of 4-bit indices in 64 bits, ascending - a kernel argument that needs no indexed array
// Every difference, product and sum is rounded on its own - NO fused multiply-add (the pragma, as in obstacle_tracks.hpp) - so that the sums
// are, bit for bit, what a sequential numpy loop over the recorded states makes.  A NaN state stays a NaN in its sums.
#pragma once

#include <cmath>
#include <cstdint>

#ifndef USV_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define USV_HD __host__ __device__ inline
#else
#define USV_HD inline
#endif
#endif

namespace usv {

USV_HD double log_error(double xa, double rhs)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return xa - rhs;
}

USV_HD void log_accumulate(double e, double *sum_abs, double *sum_sq)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double sq = e * e;
    *sum_abs = *sum_abs + fabs(e);
    *sum_sq = *sum_sq + sq;
}

// entry i of a nibble list
USV_HD int log_nibble(uint64_t list, int i) { return (int)((list >> (4 * i)) & 15u); }

// the set bits of mask (bits 0 .. 15), ascending, as a nibble list; *nsel: how many
USV_HD uint64_t log_pack_mask(unsigned mask, int *nsel)
{
    uint64_t list = 0;
    int n = 0;
    for (int j = 0; j < 16; j++)
        if ((mask >> j) & 1u) list |= (uint64_t)j << (4 * n++);
    *nsel = n;
    return list;
}

// up to 16 indices 0 .. 15 as a nibble list (the error channels' states)
USV_HD uint64_t log_pack_list(const int *idx, int n)
{
    uint64_t list = 0;
    for (int i = 0; i < n; i++) list |= (uint64_t)(idx[i] & 15) << (4 * i);
    return list;
}

// The arguments of usv_log_record (usvmpc.hip): nothing in here is indexed at run time - the lists are nibble lists, the error channels'
// constants four scalars - so that the kernel needs no scratch.
struct LogRec {
    const double *x0, *u;        // [B][nx], [B][N][nu]
    const int *status, *qp_iter; // [B]
    double *rx, *ru;             // the record's slabs [B][nsel], [B][nu]; nullptr: channel not recorded, or no record at this hand-over
    int *rs;                     // [B]
    double *sum_abs, *sum_sq;    // [B][n_err]; nullptr: the sums rest at this hand-over
    long B;
    int nx, nu, ustride, nsel, n_err; // (ustride = N nu: from one instance's u of stage 0 to the next one's)
    uint64_t sel, err_a, err_b;  // nibble lists: the selected states, the error channels' states
    unsigned err_const;          // bit c: channel c subtracts its constant
    double c0, c1, c2, c3;
};

} // namespace usv
