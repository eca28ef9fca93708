// Host harness of csrc/pf_guidance.hpp (tests/test_pf_frontend.py): the header's functions, compiled with the host compiler, driven over a
// scripted tick sequence with the sequencing of the kernels usv_pf_prepare / usv_pf_publish (usvmpc.hip), host-fed mode.
//   pf_frontend_harness B npts L K ticks max_radius margin stale_tick in.bin out.bin
// in.bin (doubles): wp [B][2 npts] | world [B][L][3] | per tick: vel [B][3], pose [B][3], x1 thrust [B][2]
// out.bin (doubles), per tick and instance one record:
//   k, phase, finish_tick, wrote, x0 [14], last [3], p [2K], lh [K], chosen [K], min_clearance, thr_port, thr_stbd, Tx, Tz, speed, e_u, e_ye, active
// stale_tick: the tick at which the caller "has written yref" (-1: never); tick 0 is stale as after a reset.
#include "pf_guidance.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace usv;

int main(int argc, char **argv)
{
    if (argc != 11) { std::fprintf(stderr, "usage\n"); return 2; }
    const int B = std::atoi(argv[1]), npts = std::atoi(argv[2]), L = std::atoi(argv[3]), K = std::atoi(argv[4]), T = std::atoi(argv[5]);
    const double max_radius = std::atof(argv[6]), margin = std::atof(argv[7]);
    const int stale_tick = std::atoi(argv[8]);
    const size_t n_in = (size_t)B * 2 * npts + (size_t)B * L * 3 + (size_t)T * B * 8;
    std::vector<double> in(n_in);
    FILE *f = std::fopen(argv[9], "rb");
    if (!f || std::fread(in.data(), sizeof(double), n_in, f) != n_in) { std::fprintf(stderr, "short input\n"); return 3; }
    std::fclose(f);
    const double *wp = in.data(), *world = wp + (size_t)B * 2 * npts, *ticks = world + (size_t)B * L * 3;
    // front-end state as usv_pf_reset leaves it
    std::vector<int> k(B, 1), phase(B, PF_SWITCH), finish(B, -1), chosen((size_t)B * (K ? K : 1), -1);
    std::vector<double> past(2 * B, 0.0), last(3 * B, __builtin_nan("")), u(B, 0.0), ye(B, 0.0), minc(B, 1e300), x0((size_t)B * PF_NX, 0.0);
    std::vector<double> p((size_t)B * 2 * (K ? K : 1), 0.0), lh((size_t)B * (K ? K : 1), 0.0), d(L ? L : 1);
    std::vector<PfOutputs> out(B);
    for (auto &o : out) o = PfOutputs{0, 0, 0, 0, 0, 0.0f, 0.0f};
    std::vector<int> active(B, 0);
    std::vector<double> rec;
    for (int t = 0; t < T; t++) {
        const double *vel = ticks + (size_t)t * B * 8, *pose = vel + (size_t)B * 3, *thr = pose + (size_t)B * 3;
        const bool stale = t == 0 || t == stale_tick;
        for (int b = 0; b < B; b++) {
            // ---- prepare
            const double uu = pf_fix_u(vel[3 * b]), v = vel[3 * b + 1], r = vel[3 * b + 2];
            const double nedx = pose[3 * b], nedy = pose[3 * b + 1], psi = pose[3 * b + 2];
            PfSegment seg;
            const int ph = pf_waypoint(wp + (size_t)b * 2 * npts, npts, k[b], nedx, nedy, seg);
            phase[b] = ph;
            if (ph == PF_SWITCH) k[b]++;
            if (ph == PF_OVER && finish[b] < 0) finish[b] = t;
            if (ph != PF_OVER) {
                const double dmin = pf_select(world + (size_t)b * L * 3, L, K, nedx, nedy, max_radius, margin, d.data(), 1, &p[(size_t)b * 2 * K],
                                              &lh[(size_t)b * K], &chosen[(size_t)b * K]);
                if (dmin < minc[b]) minc[b] = dmin;
            }
            if (ph == PF_ACTIVE) {
                pf_x0(psi, uu, v, r, seg, nedx, nedy, past[2 * b], past[2 * b + 1], &x0[(size_t)b * PF_NX]);
                u[b] = uu; ye[b] = seg.ye;
            }
            const bool wrote = pf_yref_write(ph, stale, &last[3 * b], seg);
            if (wrote) { last[3 * b] = seg.sin_ak; last[3 * b + 1] = seg.cos_ak; last[3 * b + 2] = seg.u_des; }
            else if (stale) last[3 * b] = last[3 * b + 1] = last[3 * b + 2] = __builtin_nan("");
            // ---- publish (the "solve" is the scripted x_1 thrust)
            active[b] = ph == PF_ACTIVE ? 1 : 0;
            if (ph == PF_ACTIVE) {
                pf_publish(thr[2 * b], thr[2 * b + 1], PF_SPEED, u[b], ye[b], out[b]);
                past[2 * b] = out[b].thr_port; past[2 * b + 1] = out[b].thr_stbd;
            } else if (ph == PF_OVER) {
                out[b].thr_port = 0.0; out[b].thr_stbd = 0.0; out[b].speed = 0.0;
            }
            rec.push_back(k[b]); rec.push_back(ph); rec.push_back(finish[b]); rec.push_back(wrote ? 1.0 : 0.0);
            for (int j = 0; j < PF_NX; j++) rec.push_back(x0[(size_t)b * PF_NX + j]);
            for (int j = 0; j < 3; j++) rec.push_back(last[3 * b + j]);
            for (int j = 0; j < 2 * K; j++) rec.push_back(p[(size_t)b * 2 * K + j]);
            for (int j = 0; j < K; j++) rec.push_back(lh[(size_t)b * K + j]);
            for (int j = 0; j < K; j++) rec.push_back(chosen[(size_t)b * K + j]);
            rec.push_back(minc[b]);
            rec.push_back(out[b].thr_port); rec.push_back(out[b].thr_stbd); rec.push_back(out[b].Tx); rec.push_back(out[b].Tz);
            rec.push_back(out[b].speed); rec.push_back((double)out[b].e_u); rec.push_back((double)out[b].e_ye); rec.push_back(active[b]);
        }
    }
    f = std::fopen(argv[10], "wb");
    if (!f || std::fwrite(rec.data(), sizeof(double), rec.size(), f) != rec.size()) { std::fprintf(stderr, "write failed\n"); return 4; }
    std::fclose(f);
    std::printf("ok %d\n", B);
    return 0;
}
