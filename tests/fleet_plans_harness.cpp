// Command-line driver of csrc/fleet_plan.hpp (tests/test_fleet_plans.py): exchanged plans - the stages 1 .. N of a slot that holds a
// scene-mate follow the mate's planned path - compiled with the host compiler only (-ffp-contract=off), against the numpy restatement
// scenario.fleet_plan_stages, bit for bit.  Also a stand-alone program under AddressSanitizer and UBSan.
//   fleet_plans_harness <model: pf | ca> <B> <S> <n_fixed> <N> <K> <in.bin> <out.bin>
// in.bin, doubles:   x [B][N+1][NX] | status [B] | finish_tick [B] | chosen [B][K] | pv [B][K][4] | p [B][N+1][2K]
// out.bin, doubles:  p [B][N+1][2K] | source [B][K] | fed (1)
// The integers travel as doubles (exact: all far below 2^53).
#include "fleet_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace usv;

template <class Fleet>
static int run(long B, int S, int n_fixed, int N, int K, const char *fin, const char *fout)
{
    const size_t nx = (size_t)B * (N + 1) * Fleet::NX, nk = (size_t)B * K, np = (size_t)B * (N + 1) * 2 * K;
    const size_t need = nx + 2 * (size_t)B + nk + 4 * nk + np;
    std::vector<double> in(need);
    FILE *f = std::fopen(fin, "rb");
    if (!f || std::fread(in.data(), sizeof(double), need, f) != need) { std::printf("short input\n"); return 1; }
    std::fclose(f);
    const double *x = in.data(), *dst = x + nx, *dft = dst + B, *dch = dft + B, *pv = dch + nk, *p0 = pv + 4 * nk;
    std::vector<int> status(B), finish(B), chosen(nk ? nk : 1), source(nk ? nk : 1, -1);
    for (long b = 0; b < B; b++) { status[b] = (int)dst[b]; finish[b] = (int)dft[b]; }
    for (size_t e = 0; e < nk; e++) chosen[e] = (int)dch[e];
    std::vector<double> p(p0, p0 + np);
    long fed = 0;
    for (long i = 0; i < B; i++)
        fed += fleet_plan_instance<Fleet>(x, status.data(), finish.data(), i, S, n_fixed, N, K, chosen.data() + (size_t)i * K,
                                          pv + (size_t)i * K * 4, p.data() + (size_t)i * (N + 1) * 2 * K, source.data() + (size_t)i * K);
    std::vector<double> out(p);
    for (size_t e = 0; e < nk; e++) out.push_back((double)source[e]);
    out.push_back((double)fed);
    f = std::fopen(fout, "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { std::printf("cannot write\n"); return 1; }
    std::fclose(f);
    std::printf("ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 9) { std::printf("usage: fleet_plans_harness <pf|ca> B S n_fixed N K in.bin out.bin\n"); return 2; }
    const long B = std::strtol(argv[2], nullptr, 0);
    const int S = std::atoi(argv[3]), n_fixed = std::atoi(argv[4]), N = std::atoi(argv[5]), K = std::atoi(argv[6]);
    if (B < 1 || S < 2 || B % S || n_fixed < 0 || N < 2 || K < 0) { std::printf("bad sizes\n"); return 2; }
    if (std::strcmp(argv[1], "pf") == 0) return run<PfFleet>(B, S, n_fixed, N, K, argv[7], argv[8]);
    if (std::strcmp(argv[1], "ca") == 0) return run<CaFleet>(B, S, n_fixed, N, K, argv[7], argv[8]);
    std::printf("unknown model %s\n", argv[1]);
    return 2;
}
