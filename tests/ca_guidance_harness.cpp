// Host harness of csrc/ca_guidance.hpp (tests/test_ca_guidance.py): the header's functions, compiled with the host compiler, driven over
// records of doubles.
//   ca_guidance_harness MODE K N dt in.bin out.bin          (the number of cases follows from the size of in.bin)
// MODE and the records (LM = 64 list entries, W = 4 waypoints at most):
//   reset     in: wp [4], psi                                   out: k, past_psied
//   sim       in: pose [3], max_radius, nw, world [LM][3]       out: n, obstacles [LM][3]
//   obstacles in: psi, nedx, nedy, n, obs [LM][3]               out: p [2K], lh [K], chosen [K]
//   prepare   in: vel [2], pose [3], k, past_psied, npts, wp [2W], n, obs [LM][3]
//             out: active, k, past_psied, ak, ye, x0 [8], p [2K], lh [K]                    (usv_guidance_pre's sequence)
//   publish   in: x1_psied, u0, ak                              out: heading, r, speed, past_psied
//   tick      in: x0 [8], k, past_psied, npts, wp [2W], L, max_radius, predict, min_clear, finish_tick, tick, world [LM][3], wvel [LM][2],
//                 p [(N+1)][2K], lh [N][K]  (what the arrays held before)
//             out: x0 [8], k, past_psied, active, ak, ye, min_clear, finish_tick, chosen [K], p [(N+1)][2K], lh [N][K]
//                                                                                            (usv_guidance_tick's sequence, one instance)
#include "ca_guidance.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace usv;

static const int LM = GUIDANCE_LMAX, W = 4;

// one instance of usv_guidance_tick (usvmpc.hip): the decide step, then the rows the stream step stores
static void tick(const double *in, double *out, int K, int N, double dt)
{
    double x0[CA_NX];
    std::memcpy(x0, in, sizeof x0);
    int k = (int)in[8];
    float pp = (float)in[9];
    const int npts = (int)in[10];
    const double *wp = in + 11;
    const int L = (int)in[11 + 2 * W];
    const double max_radius = in[12 + 2 * W];
    const bool predict = in[13 + 2 * W] != 0.0;
    double min_clear = in[14 + 2 * W];
    int finish = (int)in[15 + 2 * W];
    const int tk = (int)in[16 + 2 * W];
    const double *world = in + 17 + 2 * W, *wvel = world + 3 * LM, *p_in = wvel + 2 * LM, *lh_in = p_in + (size_t)(N + 1) * 2 * K;
    std::vector<double> p(p_in, p_in + (size_t)(N + 1) * 2 * K), lh(lh_in, lh_in + (size_t)N * K), d(LM), pv(4 * (K ? K : 1)), tl(K ? K : 1);
    std::vector<int> chosen(K ? K : 1, -1);
    int active = 0;
    double ak = 0.0, ye = 0.0;
    if (k >= npts) {
        if (finish < 0) finish = tk;
    } else {
        const double u_cb = ca_fix_u(x0[0]), v_cb = x0[1], nedx = x0[5], nedy = x0[6], psi = x0[7];
        if (predict) {
            ca_select_tracks(world, wvel, L, K, psi, nedx, nedy, max_radius, d.data(), 1, pv.data(), tl.data(), chosen.data());
            for (int s = 0; s <= N; s++)
                for (int i = 0; i < K; i++) {
                    p[((size_t)s * K + i) * 2] = ca_stage(&pv[4 * i], 0, s, dt);
                    p[((size_t)s * K + i) * 2 + 1] = ca_stage(&pv[4 * i], 1, s, dt);
                }
            for (int s = 0; s < N; s++)
                for (int i = 0; i < K; i++) lh[(size_t)s * K + i] = tl[i];
        } else {
            ca_select_world(world, L, K, psi, nedx, nedy, max_radius, d.data(), 1, p.data(), lh.data(), chosen.data());
        }
        const double c = ca_min_clearance(world, L, nedx, nedy, d.data(), 1);
        if (c < min_clear) min_clear = c;
        ca_waypoint(wp, npts, nedx, nedy, k, pp, active, ak, ye);
        if (active) ca_x0(u_cb, v_cb, ye, psi, ak, pp, nedx, nedy, x0);
        else if (finish < 0) finish = tk;
        if (!active) pp = (float)in[9]; // (the kernel stores past_psied for an active tick only)
    }
    std::memcpy(out, x0, sizeof x0);
    out[8] = k; out[9] = (double)pp; out[10] = active; out[11] = ak; out[12] = ye; out[13] = min_clear; out[14] = finish;
    for (int i = 0; i < K; i++) out[15 + i] = chosen[i];
    std::memcpy(out + 15 + K, p.data(), p.size() * sizeof(double));
    std::memcpy(out + 15 + K + p.size(), lh.data(), lh.size() * sizeof(double));
}

int main(int argc, char **argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: ca_guidance_harness MODE K N dt in.bin out.bin\n"); return 2; }
    const std::string mode = argv[1];
    const int K = std::atoi(argv[2]), N = std::atoi(argv[3]);
    const double dt = std::atof(argv[4]);
    if (K < 0 || K > 32 || N < 1 || N > 1000) { std::fprintf(stderr, "bad sizes\n"); return 2; }
    size_t nin = 0, nout = 0;
    if (mode == "reset") { nin = 5; nout = 2; }
    else if (mode == "sim") { nin = 5 + 3 * LM; nout = 1 + 3 * LM; }
    else if (mode == "obstacles") { nin = 4 + 3 * LM; nout = 4 * (size_t)K; }
    else if (mode == "prepare") { nin = 9 + 2 * W + 3 * LM; nout = 13 + 3 * (size_t)K; }
    else if (mode == "publish") { nin = 3; nout = 4; }
    else if (mode == "tick") { nin = 17 + 2 * W + 5 * LM + (size_t)(N + 1) * 2 * K + (size_t)N * K; nout = 15 + K + (size_t)(N + 1) * 2 * K + (size_t)N * K; }
    else { std::fprintf(stderr, "unknown mode\n"); return 2; }
    FILE *f = std::fopen(argv[5], "rb");
    if (!f) { std::fprintf(stderr, "no input\n"); return 3; }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || (size_t)bytes % (nin * sizeof(double)) != 0) { std::fprintf(stderr, "input is not whole records\n"); std::fclose(f); return 3; }
    const size_t cases = (size_t)bytes / (nin * sizeof(double));
    std::vector<double> in(cases * nin + 1), out(cases * nout + 1, 0.0), d(LM);
    if (std::fread(in.data(), sizeof(double), cases * nin, f) != cases * nin) { std::fprintf(stderr, "short input\n"); std::fclose(f); return 3; }
    std::fclose(f);
    for (size_t c = 0; c < cases; c++) {
        const double *a = &in[c * nin];
        double *o = &out[c * nout];
        if (mode == "reset") {
            int k; float pp;
            ca_reset(a, a[4], k, pp);
            o[0] = k; o[1] = (double)pp;
        } else if (mode == "sim") {
            int nw = (int)a[4];
            nw = nw < 0 ? 0 : (nw > LM ? LM : nw);
            o[0] = ca_sense_list(a[0], a[1], a[2], a + 5, nw, a[3], o + 1, LM);
        } else if (mode == "obstacles") {
            int n = (int)a[3];
            n = n < 0 ? 0 : (n > LM ? LM : n);
            std::vector<int> ch(K ? K : 1);
            ca_select_body(a + 4, n, K, a[0], a[1], a[2], d.data(), 1, o, o + 2 * K, ch.data());
            for (int i = 0; i < K; i++) o[3 * K + i] = ch[i];
        } else if (mode == "prepare") {
            const double u_cb = ca_fix_u(a[0]), v_cb = a[1], nedx = a[2], nedy = a[3], psi = a[4];
            int k = (int)a[5];
            float pp = (float)a[6];
            const int npts = (int)a[7];
            int n = (int)a[8 + 2 * W];
            n = n < 0 ? 0 : (n > LM ? LM : n);
            ca_select_body(a + 9 + 2 * W, n, K, psi, nedx, nedy, d.data(), 1, o + 13, o + 13 + 2 * K, nullptr);
            int active;
            double ak, ye;
            ca_waypoint(a + 8, npts, nedx, nedy, k, pp, active, ak, ye);
            if (active) ca_x0(u_cb, v_cb, ye, psi, ak, pp, nedx, nedy, o + 5);
            o[0] = active; o[1] = k; o[2] = (double)pp; o[3] = ak; o[4] = ye;
        } else if (mode == "publish") {
            float pp;
            ca_publish(a[0], a[2], a[1], pp, o[0], o[1], o[2]);
            o[3] = (double)pp;
        } else {
            tick(a, o, K, N, dt);
        }
    }
    f = std::fopen(argv[6], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), cases * nout, f) != cases * nout) { std::fprintf(stderr, "write failed\n"); return 4; }
    std::fclose(f);
    std::printf("ok %zu\n", cases);
    return 0;
}
