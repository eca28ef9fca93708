// cost_eval.hpp — the arithmetic of the objective value (usvmpc.hip: usv_cost_eval, usv_cost_track; include/usvmpc.h: usvmpc_get "cost" /
// "cost_stage" / "cost_parts", usvmpc_eval_cost, usvmpc_cost_track), as pure functions: host + device, no dependency on the kernels
// (tests/cost_eval_harness.cpp).
//
// The conventions are the project's (oracle/usv_oracle.h, host_spec.hpp): stage weight dt W, terminal weight W_e unscaled,
// slack cost scaled by dt, z = [u; x], V = [Vu Vx], dt = Tf / N.  Every product, difference and sum is rounded on its own - NO fused
// multiply-add (the pragma, as in closed_loop_log.hpp) - so that the results are, bit for bit, what a sequential numpy loop makes.  The order
// of operations is part of the interface:
//
//   stage k < N, z = [u_k; x_k], nz = nu + nx, rows i = 0 .. ny-1:
//       y_i = 0.0;  for j = 0 .. nz-1:  y_i = y_i + V[i][j]*z_j
//       r_i = y_i - yref[k][i]
//       t_i = 0.0;  for j = 0 .. ny-1:  t_i = t_i + W[i][j]*r_j
//       q   = 0.0;  for i = 0 .. ny-1:  q = q + r_i*t_i
//       ls_k = (0.5*dt) * q
//       S   = 0.0;  for i = 0 .. K-1:   S = S + (((zl_i*sl_i + zu_i*su_i) + (0.5*Zl_i)*(sl_i*sl_i)) + (0.5*Zu_i)*(su_i*su_i))
//       slack_k = dt * S                                     (hard h rows: K = 0 here, slack_k = dt * 0.0 = 0.0)
//       c_k = ls_k + slack_k
//   stage N: the same r, t, q with Vx_e, W_e, yref_e and z = x_N;  c_N = 0.5*q
//   totals, each sequential from 0.0 in stage order:
//       cost  = sum over k = 0 .. N of c_k
//       parts = [sum over k < N of ls_k,  c_N,  sum over k < N of slack_k]
//   tracked sum (one step per hand-over, in hand-over order):  sum = sum + c_0, c_0 the stage function with z = [u_0; x0]
//
// Padding: the kernels run every loop to 16 (S: to 16 or 32) over tables and rows padded with 0.0.  A padded term is 0.0 * 0.0 = +0.0, and a
// sum that started from +0.0 is never -0.0, so adding it changes no bit: the results are those of the loops above for every finite input.
// No clamp anywhere: a negative slack enters as it is.  A NaN in an instance's data stays a NaN in that instance's results.
#pragma once

#include <cmath>
#include <cstdint>

#ifndef USV_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define USV_HD __host__ __device__ inline
#else
#define USV_HD inline
#endif
#endif

namespace usv {

constexpr int COST_LANES = 16; // rows / columns of the padded tables (ny, nz <= 16: include/usvmpc.h USVMPC_NY_MAX)
constexpr int COST_KMAX = 32;  // obstacle rows (USVMPC_K_MAX)

// ---- the primitives: one rounding each.  The kernels are made of these and of nothing else that rounds.
USV_HD double cost_mac(double acc, double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = a * b;
    return acc + p;
}
USV_HD double cost_add(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a + b;
}
USV_HD double cost_sub(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a - b;
}
USV_HD double cost_mul(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a * b;
}
// one row's share of S: ((zl sl + zu su) + (0.5 Zl)(sl sl)) + (0.5 Zu)(su su)
USV_HD double cost_slack_term(double zl, double zu, double Zl, double Zu, double sl, double su)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = zl * sl;
    const double b = zu * su;
    const double lin = a + b;
    const double hl = 0.5 * Zl;
    const double sl2 = sl * sl;
    const double ql = hl * sl2;
    const double hu = 0.5 * Zu;
    const double su2 = su * su;
    const double qu = hu * su2;
    const double s1 = lin + ql;
    return s1 + qu;
}
// ls_k = (0.5 dt) q;  slack_k = dt S;  c_N = 0.5 q
USV_HD double cost_ls(double dt, double q)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double w = 0.5 * dt;
    return w * q;
}

// ---- the tables the kernels read (made on the host on first use, one small device allocation): TRANSPOSED and zero-padded to 16 x 16, so
// that lane r of a 16-lane group reads row r of V and of W as 16 loads in which the group's lanes are contiguous.
struct CostTab {
    double Vt[COST_LANES * COST_LANES];  // Vt[j * 16 + i] = V[i][j], V = [Vu Vx]
    double Wt[COST_LANES * COST_LANES];  // Wt[j * 16 + i] = W[i][j]
    double Vte[COST_LANES * COST_LANES]; // Vx_e, likewise
    double Wte[COST_LANES * COST_LANES]; // W_e
    double zl[COST_KMAX], zu[COST_KMAX], Zl[COST_KMAX], Zu[COST_KMAX]; // the h rows' slack penalties as the caller gave them (not scaled by dt)
};

// Vu [ny][nu], Vx [ny][nx], W [ny][ny], Vx_e [ny_e][nx], W_e [ny_e][ny_e] row-major with their own dimensions (usvmpc_desc)
inline void cost_fill_tab(CostTab &T, int nx, int nu, int ny, int ny_e, int K, const double *Vu, const double *Vx, const double *W,
                          const double *Vx_e, const double *W_e, const double *zl, const double *zu, const double *Zl, const double *Zu)
{
    T = CostTab{};
    for (int i = 0; i < ny; i++) {
        for (int j = 0; j < nu; j++) T.Vt[j * COST_LANES + i] = Vu[i * nu + j];
        for (int j = 0; j < nx; j++) T.Vt[(nu + j) * COST_LANES + i] = Vx[i * nx + j];
        for (int j = 0; j < ny; j++) T.Wt[j * COST_LANES + i] = W[i * ny + j];
    }
    for (int i = 0; i < ny_e; i++) {
        for (int j = 0; j < nx; j++) T.Vte[j * COST_LANES + i] = Vx_e[i * nx + j];
        for (int j = 0; j < ny_e; j++) T.Wte[j * COST_LANES + i] = W_e[i * ny_e + j];
    }
    for (int i = 0; i < K; i++) { T.zl[i] = zl[i]; T.zu[i] = zu[i]; T.Zl[i] = Zl[i]; T.Zu[i] = Zu[i]; }
}

// ---- the sequential statement of one instance, over the same tables (the CPU harness; the kernels spread the rows over a group's lanes and
// take every sum in this order)
// q of a stage: Vt / Wt one of the table's pairs, z [nz], yref [ny]
USV_HD double cost_q(const double *Vt, const double *Wt, const double *z, const double *yref, int nz, int ny)
{
    double r[COST_LANES];
    for (int i = 0; i < ny; i++) {
        double y = 0.0;
        for (int j = 0; j < nz; j++) y = cost_mac(y, Vt[j * COST_LANES + i], z[j]);
        r[i] = cost_sub(y, yref[i]);
    }
    double q = 0.0;
    for (int i = 0; i < ny; i++) {
        double t = 0.0;
        for (int j = 0; j < ny; j++) t = cost_mac(t, Wt[j * COST_LANES + i], r[j]);
        q = cost_add(q, cost_mul(r[i], t));
    }
    return q;
}
// S of a stage over K soft rows
USV_HD double cost_S(const CostTab &T, const double *sl, const double *su, int K)
{
    double S = 0.0;
    for (int i = 0; i < K; i++) S = cost_add(S, cost_slack_term(T.zl[i], T.zu[i], T.Zl[i], T.Zu[i], sl[i], su[i]));
    return S;
}
// c_k of a stage k < N from u_k [nu], x_k [nx] (or x0: the tracked sum), yref [ny], sl / su [K]; *ls and *slack: its two shares
USV_HD double cost_stage(const CostTab &T, double dt, const double *u, const double *x, const double *yref, const double *sl, const double *su,
                         int nx, int nu, int ny, int K, double *ls, double *slack)
{
    double z[COST_LANES];
    for (int j = 0; j < nu; j++) z[j] = u[j];
    for (int j = 0; j < nx; j++) z[nu + j] = x[j];
    *ls = cost_ls(dt, cost_q(T.Vt, T.Wt, z, yref, nu + nx, ny));
    *slack = cost_mul(dt, cost_S(T, sl, su, K));
    return cost_add(*ls, *slack);
}
// c_N
USV_HD double cost_terminal(const CostTab &T, const double *xN, const double *yref_e, int nx, int ny_e)
{
    return cost_mul(0.5, cost_q(T.Vte, T.Wte, xN, yref_e, nx, ny_e));
}
// One instance: x [N+1][nx], u [N][nu], yref [N][ny], yref_e [ny_e], sl / su [N][Kstride] of which the first K enter (K = 0: hard rows) ->
// c [N+1], *cost, parts [3]
USV_HD void cost_instance(const CostTab &T, double dt, int N, int nx, int nu, int ny, int ny_e, int K, int Kstride, const double *x, const double *u,
                          const double *yref, const double *yref_e, const double *sl, const double *su, double *c, double *cost, double *parts)
{
    double total = 0.0, p_ls = 0.0, p_slack = 0.0;
    for (int k = 0; k < N; k++) {
        double ls, slack;
        c[k] = cost_stage(T, dt, u + (long)k * nu, x + (long)k * nx, yref + (long)k * ny, sl + (long)k * Kstride, su + (long)k * Kstride, nx, nu, ny, K, &ls,
                          &slack);
        total = cost_add(total, c[k]);
        p_ls = cost_add(p_ls, ls);
        p_slack = cost_add(p_slack, slack);
    }
    c[N] = cost_terminal(T, x + (long)N * nx, yref_e, nx, ny_e);
    *cost = cost_add(total, c[N]);
    parts[0] = p_ls; parts[1] = c[N]; parts[2] = p_slack;
}

// The arguments of usv_cost_eval / usv_cost_track (usvmpc.hip): pointers and sizes only - nothing in here is indexed at run time, the tables
// live in device memory - so that the kernels need no scratch.
struct CostArgs {
    const CostTab *tab;
    const double *x, *u, *yref, *yref_e, *sl, *su; // [B][N+1][nx], [B][N][nu], [B][N][ny], [B][ny_e], [B][N][K] twice
    const double *x0;                              // [B][nx] (usv_cost_track)
    double *cost_stage, *cost, *parts;             // [B][N+1], [B], [B][3] (usv_cost_eval)
    double *sum;                                   // [B] (usv_cost_track)
    long B;
    int N, nx, nu, ny, ny_e;
    int K;   // entries of a stage of sl / su
    int Ks;  // how many of them enter the cost: K for soft h rows, 0 for hard ones
    double dt;
};

} // namespace usv
