// Host harness of csrc/ca_fleet_world.hpp (tests/test_ca_fleet.py): the header's functions, compiled with the host compiler.  All files
// hold doubles.
//   ca_fleet_world_harness gather B S n_fixed radius ticks in.bin out.bin
//       in.bin: per tick x0 [B][8].  The world lists start as 7.0 everywhere (what a gather must leave alone in the fixed entries), the
//       bookkeeping as after a reset; per tick every instance is gathered as the kernel usv_guidance_fleet_gather does (usvmpc.hip).
//       out.bin, per tick: world [B][n_fixed + S - 1][3] | wvel [B][n_fixed + S - 1][2] | min_separation [B] | separation_tick [B]
//   ca_fleet_world_harness map B S out.bin                 out.bin: fleet_vessel(i, e, S) as [B][S - 1] (fleet_world.hpp's, reused)
#include "ca_fleet_world.hpp"

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
        if (B < 1 || T < 0 || !fleet_scene_ok(B, S) || !fleet_on(S) || !fleet_fits(n_fixed, S)) { std::fprintf(stderr, "refused\n"); return 5; }
        const int nworld = n_fixed + fleet_slots(S);
        std::vector<double> in((size_t)T * B * CA_FLEET_NX);
        if (!load(argv[7], in)) { std::fprintf(stderr, "short input\n"); return 3; }
        std::vector<double> world((size_t)B * nworld * 3, 7.0), wvel((size_t)B * nworld * 2, 7.0), min_sep(B, 1e300);
        std::vector<int> sep_tick(B, -1);
        for (int t = 0; t < T; t++) {
            const double *x0 = in.data() + (size_t)t * B * CA_FLEET_NX;
            for (long i = 0; i < B; i++)
                ca_fleet_gather(x0, i, S, n_fixed, radius, t, &world[(size_t)i * nworld * 3], &wvel[(size_t)i * nworld * 2], min_sep[i], sep_tick[i]);
            out.insert(out.end(), world.begin(), world.end());
            out.insert(out.end(), wvel.begin(), wvel.end());
            out.insert(out.end(), min_sep.begin(), min_sep.end());
            out.insert(out.end(), sep_tick.begin(), sep_tick.end());
        }
    } else if (!std::strcmp(argv[1], "map") && argc == 5) {
        const long B = std::atol(argv[2]);
        const int S = std::atoi(argv[3]);
        if (B < 1 || !fleet_on(S)) { std::fprintf(stderr, "refused\n"); return 5; }
        for (long i = 0; i < B; i++)
            for (int e = 0; e < S - 1; e++) out.push_back((double)fleet_vessel(i, e, S));
    } else {
        std::fprintf(stderr, "usage\n");
        return 2;
    }
    if (!store(dst, out)) { std::fprintf(stderr, "write failed\n"); return 4; }
    std::printf("ok\n");
    return 0;
}
