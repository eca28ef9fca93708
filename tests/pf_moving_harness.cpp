// Host harness of the moving-world part of csrc/pf_guidance.hpp (tests/test_pf_moving.py): the header's functions, compiled with the host
// compiler, driven over a scripted tick sequence with the sequencing of the kernels usv_pf_prepare (decide, then stream) and
// usv_pf_world_step (usvmpc.hip), host-fed mode: every tick a prepare, then a world step of dt.
//   pf_moving_harness B npts L K N ticks max_radius margin dt in.bin out.bin
// in.bin (doubles): wp [B][2 npts] | world [B][L][3] | wvel [B][L][2] | per tick: vel [B][3], pose [B][3]
// out.bin (doubles), per tick and instance one record:
//   phase, chosen [K], min_clearance, p [N+1][2K], lh [N][K], world after the step [L][3]
#include "pf_guidance.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace usv;

int main(int argc, char **argv)
{
    if (argc != 12) { std::fprintf(stderr, "usage\n"); return 2; }
    const int B = std::atoi(argv[1]), npts = std::atoi(argv[2]), L = std::atoi(argv[3]), K = std::atoi(argv[4]), N = std::atoi(argv[5]);
    const int T = std::atoi(argv[6]);
    const double max_radius = std::atof(argv[7]), margin = std::atof(argv[8]), dt = std::atof(argv[9]);
    const size_t n_in = (size_t)B * 2 * npts + (size_t)B * L * 5 + (size_t)T * B * 6;
    std::vector<double> in(n_in);
    FILE *f = std::fopen(argv[10], "rb");
    if (!f || std::fread(in.data(), sizeof(double), n_in, f) != n_in) { std::fprintf(stderr, "short input\n"); return 3; }
    std::fclose(f);
    const double *wp = in.data(), *wvel = wp + (size_t)B * 2 * npts + (size_t)B * L * 3, *ticks = wvel + (size_t)B * L * 2;
    std::vector<double> world(wp + (size_t)B * 2 * npts, wp + (size_t)B * 2 * npts + (size_t)B * L * 3);
    std::vector<int> k(B, 1), chosen((size_t)B * K, -1);
    std::vector<double> minc(B, 1e300), pv((size_t)B * K * 4, 0.0), lh0((size_t)B * K, 0.0), d(L ? L : 1);
    const size_t np = (size_t)(N + 1) * 2 * K, nl = (size_t)N * K;
    std::vector<double> p(B * np, 0.0), lh(B * nl, 0.0), rec;
    std::vector<int> phase(B, PF_SWITCH);
    for (int t = 0; t < T; t++) {
        const double *vel = ticks + (size_t)t * B * 6, *pose = vel + (size_t)B * 3;
        (void)vel;
        for (int b = 0; b < B; b++) {
            const double nedx = pose[3 * b], nedy = pose[3 * b + 1];
            PfSegment seg;
            const int ph = pf_waypoint(wp + (size_t)b * 2 * npts, npts, k[b], nedx, nedy, seg);
            phase[b] = ph;
            if (ph == PF_SWITCH) k[b]++;
            if (ph == PF_OVER) continue; // (p, lh and the tracks keep what they hold)
            // decide: the slot tracks
            const double dmin = pf_select_tracks(&world[(size_t)b * L * 3], wvel + (size_t)b * L * 2, L, K, nedx, nedy, max_radius, margin, d.data(), 1,
                                                 &pv[(size_t)b * K * 4], &lh0[(size_t)b * K], &chosen[(size_t)b * K]);
            if (dmin < minc[b]) minc[b] = dmin;
            // stream: every stage from the tracks
            for (int kk = 0; kk <= N; kk++)
                for (int s = 0; s < K; s++)
                    for (int c = 0; c < 2; c++) p[b * np + (size_t)kk * 2 * K + 2 * s + c] = pf_stage(&pv[((size_t)b * K + s) * 4], c, kk, dt);
            for (int kk = 0; kk < N; kk++)
                for (int s = 0; s < K; s++) lh[b * nl + (size_t)kk * K + s] = lh0[(size_t)b * K + s];
        }
        for (size_t i = 0; i < (size_t)B * L; i++) pf_world_step(&world[3 * i], wvel + 2 * i, dt);
        for (int b = 0; b < B; b++) {
            rec.push_back(phase[b]);
            for (int s = 0; s < K; s++) rec.push_back(chosen[(size_t)b * K + s]);
            rec.push_back(minc[b]);
            rec.insert(rec.end(), p.begin() + b * np, p.begin() + (b + 1) * np);
            rec.insert(rec.end(), lh.begin() + b * nl, lh.begin() + (b + 1) * nl);
            rec.insert(rec.end(), world.begin() + (size_t)b * L * 3, world.begin() + (size_t)(b + 1) * L * 3);
        }
    }
    f = std::fopen(argv[11], "wb");
    if (!f || std::fwrite(rec.data(), sizeof(double), rec.size(), f) != rec.size()) { std::fprintf(stderr, "write failed\n"); return 4; }
    std::fclose(f);
    std::printf("ok %d\n", B);
    return 0;
}
