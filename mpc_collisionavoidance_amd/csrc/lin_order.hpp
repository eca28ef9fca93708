// lin_order.hpp — the order in which the pipelined lineariser (linearize.hpp MODE 1 / 2, usvmpc.hip launch_solve) visits the
// (group, stage) pairs of its grid, as pure functions of the index: host + device, no dependency on the kernels (tests/lin_order_harness.cpp).
//
// The speculative pass of tick t + 1 runs beside the QP launch of tick t, and that launch retires its instances in a known order: the
// groups of ITS map (perm_cur) in ascending index - the first rows x blocks at once, then its queue.  Work item i of the speculative pass
// is therefore (position q in the running launch's order, stage k), k fastest:
//     instance  b  = perm_cur[q]
//     group     g' = inv_next[b]          (inv_next: inverse of the NEXT tick's group -> instance map; identity maps: nullptr)
// so that items handed out early belong to instances that finished early, and the N + 1 stages of an instance (contiguous in x / u) are
// neighbours.  Positions q >= B are the padded groups (Bp > B: they replay the instance of the last map entry, lin_slot): they keep their
// own index.  Every (group, stage) of the [Bp][N + 1] grid is produced exactly once.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define USV_HD __host__ __device__ inline
#else
#define USV_HD inline
#endif

namespace usv {

struct LinItem {
    long g; // group of the next tick's map (target planes)
    int k;  // stage
};

// entry of a group -> instance map that group g linearises (padded groups replay the last one)
USV_HD long lin_slot(long g, long B) { return g < B ? g : B - 1; }

USV_HD LinItem lin_item(long item, int N, long B, const int *perm_cur, const int *inv_next)
{
    const long q = item / (N + 1);
    LinItem it;
    it.k = (int)(item - q * (N + 1));
    it.g = q;
    if (q < B) {
        const long b = perm_cur ? (long)perm_cur[q] : q;
        it.g = inv_next ? (long)inv_next[b] : b;
    }
    return it;
}

// ---- the paired lineariser (linearize.hpp run_pair_at: one 16-lane row serves two (group, stage) pairs, its halves 0 and 1).  Each of the three
// orders produces every (group, stage) of the [Bp][N + 1] grid exactly once over its rows; a half with nothing to do gets k = -1 (g = 0).

// stage-major (whole batch, speculative, fix-up): half number 2 row + half is the (group, stage) index k Bp + g of the 16-lane form, so the
// halves of a row hold neighbouring groups of one stage (Bp is even)
USV_HD long lin_pair_plain_rows(int N, long Bp) { return ((long)(N + 1) * Bp + 7) / 8 * 4; } // (whole waves of four rows; halves past the grid: none)
USV_HD LinItem lin_pair_plain(long row, int half, int N, long Bp)
{
    const long hid = 2 * row + half;
    LinItem it;
    it.g = 0;
    it.k = -1;
    if (hid < (long)(N + 1) * Bp) {
        it.k = (int)(hid / Bp);
        it.g = hid - (long)it.k * Bp;
    }
    return it;
}

// retire order (lin_item): position q of the running launch's order takes (N + 2) / 2 consecutive rows, row i of them the stages 2 i and
// 2 i + 1 - never two instances in one row; the second half of an instance's last row idles when N + 1 is odd.  The row count is padded to
// whole waves of four rows (a one-wave workgroup takes 8 items).
USV_HD long lin_pair_retire_rows(int N, long Bp) { return ((long)((N + 2) / 2) * Bp + 3) / 4 * 4; }
USV_HD LinItem lin_pair_retire(long row, int half, int N, long B, long Bp, const int *perm_cur, const int *inv_next)
{
    const long rpi = (N + 2) / 2;
    const long q = row / rpi;
    const int k = 2 * (int)(row - q * rpi) + half;
    LinItem it;
    it.g = 0;
    it.k = -1;
    if (q < Bp && k <= N) {
        it.k = k;
        it.g = q;
        if (q < B) {
            const long b = perm_cur ? (long)perm_cur[q] : q;
            it.g = inv_next ? (long)inv_next[b] : b;
        }
    }
    return it;
}

// fix-up by groups: the halves of a group's wave (2 x rows of them) take the stages half number, + 2 rows, ...: stage of pass t (may exceed N: none)
USV_HD int lin_pair_marked(int t, int row, int half, int rows) { return 2 * row + half + 2 * rows * t; }

} // namespace usv
