// Host harness of csrc/fleet_world.hpp (tests/test_pf_fleet.py): the header's functions, compiled with the host compiler.  All files hold
// doubles.
//   fleet_world_harness gather B S n_fixed radius ticks in.bin out.bin
//       in.bin: per tick x0 [B][14].  The world lists start as 7.0 everywhere (what a gather must leave alone in the fixed entries), the
//       bookkeeping as after a reset; per tick every instance is gathered as the kernel usv_pf_fleet_gather does (usvmpc.hip).
//       out.bin, per tick: world [B][n_fixed + S - 1][3] | wvel [B][n_fixed + S - 1][2] | min_separation [B] | separation_tick [B]
//   fleet_world_harness map B S out.bin                    out.bin: fleet_vessel(i, e, S) as [B][S - 1]
//   fleet_world_harness relayout n0_fixed f0 moving has_fixed n1_fixed f1 in.bin out.bin
//       in.bin: w0 [n0][3] | v0 [n0][2] | fixed [n1_fixed][3]   (n0 = n0_fixed + f0)      out.bin: w1 [n1][3] | v1 [n1][2]
//   fleet_world_harness refuse n in.bin out.bin            in.bin: n rows (B, S, n_fixed, radius)
//       out.bin: n rows (fleet_on, fleet_slots, fleet_scene_ok, fleet_fits, fleet_radius_ok)
#include "fleet_world.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace usv;

static bool load(const char *path, std::vector<double> &v)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = v.empty() || std::fread(v.data(), sizeof(double), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

static bool store(const char *path, const std::vector<double> &v)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = v.empty() || std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage\n"); return 2; }
    std::vector<double> out;
    const char *dst = argv[argc - 1];
    if (!std::strcmp(argv[1], "gather") && argc == 9) {
        const long B = std::atol(argv[2]);
        const int S = std::atoi(argv[3]), n_fixed = std::atoi(argv[4]), T = std::atoi(argv[6]);
        const double radius = std::atof(argv[5]);
        if (!fleet_scene_ok(B, S) || !fleet_on(S) || !fleet_fits(n_fixed, S)) { std::fprintf(stderr, "refused\n"); return 5; }
        const int nworld = n_fixed + fleet_slots(S);
        std::vector<double> in((size_t)T * B * FLEET_NX);
        if (!load(argv[7], in)) { std::fprintf(stderr, "short input\n"); return 3; }
        std::vector<double> world((size_t)B * nworld * 3, 7.0), wvel((size_t)B * nworld * 2, 7.0), min_sep(B, 1e300);
        std::vector<int> sep_tick(B, -1);
        for (int t = 0; t < T; t++) {
            const double *x0 = in.data() + (size_t)t * B * FLEET_NX;
            for (long i = 0; i < B; i++)
                fleet_gather(x0, i, S, n_fixed, radius, t, &world[(size_t)i * nworld * 3], &wvel[(size_t)i * nworld * 2], min_sep[i], sep_tick[i]);
            out.insert(out.end(), world.begin(), world.end());
            out.insert(out.end(), wvel.begin(), wvel.end());
            out.insert(out.end(), min_sep.begin(), min_sep.end());
            out.insert(out.end(), sep_tick.begin(), sep_tick.end());
        }
    } else if (!std::strcmp(argv[1], "map") && argc == 5) {
        const long B = std::atol(argv[2]);
        const int S = std::atoi(argv[3]);
        for (long i = 0; i < B; i++)
            for (int e = 0; e < S - 1; e++) out.push_back((double)fleet_vessel(i, e, S));
    } else if (!std::strcmp(argv[1], "relayout") && argc == 10) {
        const int n0_fixed = std::atoi(argv[2]), f0 = std::atoi(argv[3]), moving = std::atoi(argv[4]), has_fixed = std::atoi(argv[5]);
        const int n1_fixed = std::atoi(argv[6]), f1 = std::atoi(argv[7]), n0 = n0_fixed + f0, n1 = n1_fixed + f1;
        std::vector<double> in((size_t)n0 * 5 + (size_t)n1_fixed * 3);
        if (!load(argv[8], in)) { std::fprintf(stderr, "short input\n"); return 3; }
        out.assign((size_t)n1 * 5, -1.0);
        fleet_relayout(in.data(), moving ? in.data() + (size_t)n0 * 3 : nullptr, n0_fixed, f0, has_fixed ? in.data() + (size_t)n0 * 5 : nullptr,
                       n1_fixed, f1, out.data(), out.data() + (size_t)n1 * 3);
    } else if (!std::strcmp(argv[1], "refuse") && argc == 5) {
        const int n = std::atoi(argv[2]);
        std::vector<double> in((size_t)n * 4);
        if (!load(argv[3], in)) { std::fprintf(stderr, "short input\n"); return 3; }
        for (int r = 0; r < n; r++) {
            const long B = (long)in[4 * r];
            const int S = (int)in[4 * r + 1], n_fixed = (int)in[4 * r + 2];
            const double rows[5] = {(double)fleet_on(S), (double)fleet_slots(S), (double)fleet_scene_ok(B, S), (double)fleet_fits(n_fixed, S),
                                    (double)fleet_radius_ok(in[4 * r + 3])};
            out.insert(out.end(), rows, rows + 5);
        }
    } else {
        std::fprintf(stderr, "usage\n");
        return 2;
    }
    if (!store(dst, out)) { std::fprintf(stderr, "write failed\n"); return 4; }
    std::printf("ok\n");
    return 0;
}
