// The three orders of the paired lineariser (csrc/lin_order.hpp: lin_pair_plain, lin_pair_retire, lin_pair_marked) on the host: for
// "B Bp N seed sorted" every (group, stage) of the [Bp][N + 1] grid must come out exactly once over the halves of each order's rows; the halves
// of a row of the stage-major order hold neighbouring groups of one stage, those of the retire order stages 2 i and 2 i + 1 of ONE instance, in
// the order of the running launch's map, padded groups on map entry B - 1; the retire order's row count is a whole number of waves.
// Prints "ok <rows plain> <rows retire>" or the first violation.
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
    const int *pc = (sorted & 1) ? perm_cur.data() : nullptr;
    const int *in = (sorted & 2) ? inv_next.data() : nullptr;
    const size_t cells = (size_t)Bp * (N + 1);
    auto in_grid = [&](const usv::LinItem &it) { return it.g >= 0 && it.g < Bp && it.k >= 0 && it.k <= N; };

    // stage-major
    std::vector<int> seen(cells, 0);
    const long rows_plain = usv::lin_pair_plain_rows(N, Bp);
    for (long r = 0; r < rows_plain + 3; r++) { // (rows past the count: the kernel's last workgroup)
        const usv::LinItem a = usv::lin_pair_plain(r, 0, N, Bp), b = usv::lin_pair_plain(r, 1, N, Bp);
        for (const usv::LinItem &it : {a, b}) {
            if (it.k < 0) continue;
            if (r >= rows_plain || !in_grid(it)) { printf("plain row %ld: g %ld k %d\n", r, it.g, it.k); return 1; }
            seen[(size_t)it.g * (N + 1) + it.k]++;
        }
        if (a.k >= 0 && b.k >= 0 && (a.k != b.k || b.g != a.g + 1)) { printf("plain row %ld: halves are not neighbouring groups of a stage\n", r); return 1; }
    }
    for (size_t j = 0; j < cells; j++)
        if (seen[j] != 1) { printf("plain: (g %zu, k %zu) produced %d times\n", j / (N + 1), j % (N + 1), seen[j]); return 1; }

    // retire order
    std::fill(seen.begin(), seen.end(), 0);
    const long rows_retire = usv::lin_pair_retire_rows(N, Bp), rpi = (N + 2) / 2;
    if (rows_retire % 4 != 0 || rows_retire < rpi * Bp || rows_retire >= rpi * Bp + 4) { printf("retire: %ld rows\n", rows_retire); return 1; }
    for (long r = 0; r < rows_retire; r++) {
        const usv::LinItem a = usv::lin_pair_retire(r, 0, N, B, Bp, pc, in), b = usv::lin_pair_retire(r, 1, N, B, Bp, pc, in);
        const long q = r / rpi;
        for (const usv::LinItem &it : {a, b}) {
            if (it.k < 0) continue;
            if (q >= Bp || !in_grid(it)) { printf("retire row %ld: g %ld k %d\n", r, it.g, it.k); return 1; }
            seen[(size_t)it.g * (N + 1) + it.k]++;
            const long slot = usv::lin_slot(it.g, B);
            if (q < B) {
                if (it.g >= B || perm_next[slot] != perm_cur[q]) { printf("retire row %ld: group %ld holds instance %d, position %ld holds %d\n", r, it.g, perm_next[slot], q, perm_cur[q]); return 1; }
            } else if (it.g != q || slot != B - 1) {
                printf("retire row %ld: padded position %ld -> group %ld, map entry %ld\n", r, q, it.g, slot);
                return 1;
            }
        }
        if (q < Bp && (a.k != 2 * (int)(r - q * rpi) || (b.k >= 0 && (b.k != a.k + 1 || b.g != a.g)) || (b.k < 0 && a.k != N))) {
            printf("retire row %ld: stages %d, %d of groups %ld, %ld\n", r, a.k, b.k, a.g, b.g);
            return 1;
        }
    }
    for (size_t j = 0; j < cells; j++)
        if (seen[j] != 1) { printf("retire: (g %zu, k %zu) produced %d times\n", j / (N + 1), j % (N + 1), seen[j]); return 1; }

    // fix-up by groups: the 2 x rows halves of a group's wave, pass after pass, for the device's four rows and the emulator's one
    for (int rows : {1, 4}) {
        std::vector<int> st(N + 1, 0);
        for (int row = 0; row < rows; row++)
            for (int t = 0; usv::lin_pair_marked(t, row, 0, rows) <= N; t++)
                for (int half = 0; half < 2; half++) {
                    const int k = usv::lin_pair_marked(t, row, half, rows);
                    if (k <= N) st[k]++;
                }
        for (int k = 0; k <= N; k++)
            if (st[k] != 1) { printf("marked (%d rows): stage %d produced %d times\n", rows, k, st[k]); return 1; }
    }
    printf("ok %ld %ld\n", rows_plain, rows_retire);
    return 0;
}
