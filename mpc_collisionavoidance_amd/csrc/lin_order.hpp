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

} // namespace usv
