// The work order of the pipelined lineariser (csrc/lin_order.hpp) on the host: for "B Bp N seed sorted" on the command line, every
// (group, stage) of the [Bp][N + 1] grid must come out of lin_item exactly once, an instance's stages as N + 1 consecutive items in
// ascending stage, instances in the order of the running launch's map, and padded groups must linearise map entry B - 1.
// Prints "ok <items>" or the first violation.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "lin_order.hpp"

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    const long B = atol(argv[1]), Bp = atol(argv[2]);
    const int N = atoi(argv[3]), seed = atoi(argv[4]), sorted = atoi(argv[5]);
    std::vector<int> perm_cur(B), perm_next(B), inv_next(B);
    std::iota(perm_cur.begin(), perm_cur.end(), 0);
    std::iota(perm_next.begin(), perm_next.end(), 0);
    std::mt19937 rng((unsigned)seed);
    if (sorted & 1) std::shuffle(perm_cur.begin(), perm_cur.end(), rng);
    if (sorted & 2) std::shuffle(perm_next.begin(), perm_next.end(), rng);
    for (long g = 0; g < B; g++) inv_next[perm_next[g]] = (int)g;
    const int *pc = (sorted & 1) ? perm_cur.data() : nullptr; // (identity maps are passed as nullptr, as the library does)
    const int *in = (sorted & 2) ? inv_next.data() : nullptr;
    std::vector<int> seen((size_t)Bp * (N + 1), 0);
    const long items = Bp * (N + 1);
    for (long i = 0; i < items; i++) {
        const usv::LinItem it = usv::lin_item(i, N, B, pc, in);
        if (it.g < 0 || it.g >= Bp || it.k < 0 || it.k > N) { printf("item %ld out of the grid: g %ld k %d\n", i, it.g, it.k); return 1; }
        if (seen[(size_t)it.g * (N + 1) + it.k]++) { printf("item %ld: (g %ld, k %d) produced twice\n", i, it.g, it.k); return 1; }
        const long q = i / (N + 1);
        if (it.k != (int)(i % (N + 1))) { printf("item %ld: stage %d is not the fastest index\n", i, it.k); return 1; }
        const long slot = usv::lin_slot(it.g, B);
        if (q < B) {
            // the instance the target group linearises under the next map is the one at position q of the running launch
            if (it.g >= B || perm_next[slot] != perm_cur[q]) { printf("item %ld: group %ld holds instance %d, position %ld holds %d\n", i, it.g, perm_next[slot], q, perm_cur[q]); return 1; }
        } else if (it.g != q || slot != B - 1) {
            printf("item %ld: padded position %ld -> group %ld, map entry %ld (want %ld)\n", i, q, it.g, slot, B - 1);
            return 1;
        }
    }
    for (size_t j = 0; j < seen.size(); j++)
        if (seen[j] != 1) { printf("(g %zu, k %zu) produced %d times\n", j / (N + 1), j % (N + 1), seen[j]); return 1; }
    for (long g = 0; g < Bp; g++)
        if (usv::lin_slot(g, B) != (g < B ? g : B - 1)) { printf("lin_slot(%ld)\n", g); return 1; }
    printf("ok %ld\n", items);
    return 0;
}
