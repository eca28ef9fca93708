// Host harness of csrc/cascade.hpp (tests/test_cascade.py): the header's functions, compiled with the host compiler against the CPU lane
// emulator's lanes.hpp (-Itests/emu: the plant period is sim.hpp's erk_period, unmodified), driven over records of doubles.
//   cascade_harness MODE in.bin out.bin                     (the number of cases follows from the size of in.bin)
// MODE and the records:
//   inputs    in: s [6], past [2], psi_des, u_des             out: x0 [8], yref row [10]
//   outputs   in: x1 [8], psi_des, u_des, psi, u              out: thr [2], past [2], e_u, e_psi
//   plant     in: s [6], thr [2], c, T, steps                 out: s [6]
//   changed   in: last [2], psi_des, u_des                    out: changed (last = (-1, -1): "nothing written yet", cas_never)
//   ticks     in: tick, ratio                                 out: guidance tick, hands over
// (sim.hpp's batched entry point names the launch geometry; nothing here calls it)
struct HarnessDim3 { unsigned x, y, z; };
static const HarnessDim3 blockIdx = {0, 0, 0}, blockDim = {1, 1, 1}, threadIdx = {0, 0, 0};

#include "cascade.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace usv;

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: cascade_harness MODE in.bin out.bin\n"); return 2; }
    const std::string mode = argv[1];
    int nin, nout;
    if (mode == "inputs") { nin = 10; nout = CAS_NX + CAS_NY; }
    else if (mode == "outputs") { nin = 12; nout = 6; }
    else if (mode == "plant") { nin = 11; nout = CAS_NS; }
    else if (mode == "changed") { nin = 4; nout = 1; }
    else if (mode == "ticks") { nin = 2; nout = 2; }
    else { std::fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
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
        if (mode == "inputs") {
            cas_ll_x0(r, r + 6, o);
            const CasRef ref = cas_ref(r[8], r[9]);
            for (int j = 0; j < CAS_NY; j++) o[CAS_NX + j] = cas_yref_entry(j, ref);
        } else if (mode == "outputs") {
            float e_u, e_psi;
            cas_ll_outputs(r, r[8], r[9], r[10], cas_fix_u(r[11]), o, o + 2, e_u, e_psi);
            o[4] = (double)e_u; o[5] = (double)e_psi;
        } else if (mode == "plant") {
            std::memcpy(o, r, CAS_NS * sizeof(double));
            cas_plant_period(o, r + 6, r[8], r[9], (int)r[10]);
        } else if (mode == "changed") {
            double last[2] = {r[0], r[1]};
            if (r[0] == -1.0 && r[1] == -1.0) last[0] = last[1] = cas_never();
            o[0] = cas_ref_changed(last, r[2], r[3]) ? 1.0 : 0.0;
        } else {
            o[0] = cas_guidance_tick((long long)r[0], (int)r[1]) ? 1.0 : 0.0;
            o[1] = cas_hands_over((long long)r[0], (int)r[1]) ? 1.0 : 0.0;
        }
    }
    f = std::fopen(argv[3], "wb");
    if (!f) { std::perror(argv[3]); return 1; }
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    std::printf("ok %ld\n", n);
    return 0;
}
