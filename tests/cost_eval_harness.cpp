// The arithmetic of the objective value (csrc/cost_eval.hpp) on the host: tables, one evaluation of a batch and the tracked sum, from a binary
// file to a binary file (the comparison is bit for bit: no number passes through text).
//   cost_eval_harness IN OUT
// IN : int32 B N nx nu ny ny_e K T, then doubles: dt, Vu [ny][nu], Vx [ny][nx], W [ny][ny], Vx_e [ny_e][nx], W_e [ny_e][ny_e], zl zu Zl Zu [K]
//      each, x [B][N+1][nx], u [B][N][nu], yref [B][N][ny], yref_e [B][ny_e], sl su [B][N][K] each, and T hand-overs of
//      x0 [B][nx], u0 [B][nu], yref0 [B][ny], sl0 su0 [B][K] each.
// OUT: doubles c [B][N+1], cost [B], parts [B][3], tracked [B] (the sum after T hand-overs, from 0.0).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cost_eval.hpp"

using namespace usv;

static std::vector<double> take(FILE *f, size_t n)
{
    std::vector<double> v(n ? n : 1, 0.0);
    if (n && fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: cost_eval_harness IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int32_t h[8];
    if (fread(h, sizeof(int32_t), 8, f) != 8) { fprintf(stderr, "short header\n"); return 2; }
    const int B = h[0], N = h[1], nx = h[2], nu = h[3], ny = h[4], ny_e = h[5], K = h[6], T = h[7];
    if (B < 1 || N < 1 || nx < 1 || nu < 0 || nx + nu > COST_LANES || ny < 1 || ny > COST_LANES || ny_e < 1 || ny_e > COST_LANES || K < 0 ||
        K > COST_KMAX || T < 0) {
        fprintf(stderr, "sizes out of range\n");
        return 2;
    }
    const size_t zB = (size_t)B, zN = (size_t)N;
    const double dt = take(f, 1)[0];
    const std::vector<double> Vu = take(f, (size_t)ny * nu), Vx = take(f, (size_t)ny * nx), W = take(f, (size_t)ny * ny),
                              Vx_e = take(f, (size_t)ny_e * nx), W_e = take(f, (size_t)ny_e * ny_e);
    const std::vector<double> zl = take(f, K), zu = take(f, K), Zl = take(f, K), Zu = take(f, K);
    const std::vector<double> x = take(f, zB * (zN + 1) * nx), u = take(f, zB * zN * nu), yref = take(f, zB * zN * ny), yref_e = take(f, zB * ny_e);
    const std::vector<double> sl = take(f, zB * zN * K), su = take(f, zB * zN * K);

    CostTab tab;
    cost_fill_tab(tab, nx, nu, ny, ny_e, K, Vu.data(), Vx.data(), W.data(), Vx_e.data(), W_e.data(), zl.data(), zu.data(), Zl.data(), Zu.data());

    std::vector<double> c(zB * (zN + 1)), cost(zB), parts(zB * 3), tracked(zB, 0.0);
    for (size_t b = 0; b < zB; b++)
        cost_instance(tab, dt, N, nx, nu, ny, ny_e, K, K, &x[b * (zN + 1) * nx], &u[b * zN * nu], &yref[b * zN * ny], &yref_e[b * ny_e], &sl[b * zN * K],
                      &su[b * zN * K], &c[b * (zN + 1)], &cost[b], &parts[b * 3]);
    for (int t = 0; t < T; t++) {
        const std::vector<double> x0 = take(f, zB * nx), u0 = take(f, zB * nu), y0 = take(f, zB * ny), sl0 = take(f, zB * K), su0 = take(f, zB * K);
        for (size_t b = 0; b < zB; b++) {
            double ls, slack;
            const double c0 = cost_stage(tab, dt, &u0[b * nu], &x0[b * nx], &y0[b * ny], &sl0[b * K], &su0[b * K], nx, nu, ny, K, &ls, &slack);
            tracked[b] = cost_add(tracked[b], c0);
        }
    }
    fclose(f);

    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const std::vector<double> *outs[] = {&c, &cost, &parts, &tracked};
    for (const std::vector<double> *v : outs)
        if (fwrite(v->data(), sizeof(double), v->size(), o) != v->size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(o);
    return 0;
}
