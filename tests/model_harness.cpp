// Host harness of csrc/models.hpp (tests/test_model_edges.py): the three models exactly as the lineariser and the integrator call them -
// ModelCall<M>::prepare at the start of an interval, ModelCall<M>::fjvp at a point inside it, one tangent column per call - compiled
// with the host compiler against the CPU lane emulator's lanes.hpp (-Itests/emu: frsqrt and frcp are exact there, so what is measured
// is the header's logic, not the device's estimates), driven over records of doubles.
//   model_harness MODEL in.bin out.bin                      (MODEL 0, 1, 2; the number of cases follows from the size of in.bin)
//   in: x_start [nx], x [nx], u [nu]                        out: f [nx], J [nx][nu + nx] with respect to z = [u; x]
// (linearize.hpp's kernels name the launch geometry; nothing here calls them)
struct HarnessDim3 { unsigned x, y, z; };
static const HarnessDim3 blockIdx = {0, 0, 0}, blockDim = {1, 1, 1}, threadIdx = {0, 0, 0};

#include "models.hpp"
#include "linearize.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace usv;

template <class M>
static void eval(const double *r, double *o)
{
    constexpr int NX = M::NX, NU = M::NU, NZ = NX + NU;
    using MC = ModelCall<M>;
    const double *xs = r, *x = r + NX, *u = r + 2 * NX;
    const typename MC::Pre pre = MC::prepare(xs);
    for (int c = 0; c < NZ; c++) {
        double s[NX], su[NU], f[NX], js[NX];
        for (int j = 0; j < NX; j++) s[j] = (c == NU + j) ? 1.0 : 0.0;
        for (int j = 0; j < NU; j++) su[j] = (c == j) ? 1.0 : 0.0;
        MC::fjvp(pre, x, u, s, su, f, js);
        for (int j = 0; j < NX; j++) {
            o[NX + j * NZ + c] = js[j];
            if (c == 0) o[j] = f[j];
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: model_harness MODEL in.bin out.bin\n"); return 2; }
    const int model = std::atoi(argv[1]);
    int nx, nu;
    if (model == 0) { nx = ModelM0::NX; nu = ModelM0::NU; }
    else if (model == 1) { nx = ModelM1::NX; nu = ModelM1::NU; }
    else if (model == 2) { nx = ModelM2::NX; nu = ModelM2::NU; }
    else { std::fprintf(stderr, "unknown model %s\n", argv[1]); return 2; }
    const int nin = 2 * nx + nu, nout = nx + nx * (nx + nu);
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) { std::perror(argv[2]); return 1; }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes % (long)(nin * sizeof(double))) { std::fprintf(stderr, "record size mismatch\n"); return 1; }
    const long n = bytes / (long)(nin * sizeof(double));
    std::vector<double> in((size_t)n * nin), out((size_t)n * nout);
    if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) { std::fprintf(stderr, "short read\n"); return 1; }
    std::fclose(f);
    for (long i = 0; i < n; i++) {
        const double *r = &in[(size_t)i * nin];
        double *o = &out[(size_t)i * nout];
        if (model == 0) eval<ModelM0>(r, o);
        else if (model == 1) eval<ModelM1>(r, o);
        else eval<ModelM2>(r, o);
    }
    f = std::fopen(argv[3], "wb");
    if (!f) { std::perror(argv[3]); return 1; }
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    std::printf("ok %ld\n", n);
    return 0;
}
