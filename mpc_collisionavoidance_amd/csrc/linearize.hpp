// linearize.hpp — preparation phase of one SQP-RTI iteration, one 16-lane group per
// (instance, stage) pair.  Replaces acados' sim_erk (+ generated *_expl_vde_forw),
// ocp_nlp_cost_ls evaluation (the bgh obstacle rows are evaluated in qp_ipm.hpp) for the reference's OCPs
// (/root/reference/catkin_ws/src/nmpc_ca/scripts/usv_guidance_ca1/acados_settings.py:83-194).
//
// Lane r (variable r of [u;x]) integrates ITS OWN column of the forward sensitivities
// S = [dx+/du | dx+/dx] through the 4 RK stages (the VDE is linear in S column by column), while
// every lane carries the nominal RK stage points.  The lane therefore ends up holding row r of
// [B A]' — exactly the operand layout of the Riccati recursion (qp_ipm.hpp) — with no transpose; the
// informative entries are then packed densely for HBM (MatPack, params.hpp).
#pragma once
#include "lanes.hpp"
#include "lin_order.hpp"
#include "params.hpp"
#include "sfor.hpp"

namespace usv {

// A model may prepare quantities that are constant over a shooting interval (they depend only on states whose
// right-hand side is zero): `struct Pre`, `prepare(x)`, `fjvp_pre(pre, ...)`.  Models without them are called through
// their plain fjvp.
template <class M, class = void>
struct ModelCall {
    struct Pre {};
    USV_DEV static Pre prepare(const double *) { return {}; }
    USV_DEV static void fjvp(const Pre &, const double *x, const double *U, const double *s, const double *su, double *f, double *js)
    {
        M::fjvp(x, U, s, su, f, js);
    }
};
template <class M>
struct ModelCall<M, std::void_t<typename M::Pre>> {
    using Pre = typename M::Pre;
    USV_DEV static Pre prepare(const double *x) { return M::prepare(x); }
    USV_DEV static void fjvp(const Pre &p, const double *x, const double *U, const double *s, const double *su, double *f, double *js)
    {
        M::fjvp_pre(p, x, U, s, su, f, js);
    }
};
// ... also handing out the integrands of the model's quadrature entries (PairQuad, params.hpp); a model without such entries: the plain call
template <class M, class = void>
struct ModelQuad {
    USV_DEV static void fjvp(const typename ModelCall<M>::Pre &p, const double *x, const double *U, const double *s, const double *su, double *f, double *js, double *)
    {
        ModelCall<M>::fjvp(p, x, U, s, su, f, js);
    }
};
template <class M>
struct ModelQuad<M, std::void_t<decltype(M::PAIR_NQUAD)>> {
    USV_DEV static void fjvp(const typename M::Pre &p, const double *x, const double *U, const double *s, const double *su, double *f, double *js, double *qd)
    {
        M::fjvp_quad(p, x, U, s, su, f, js, qd);
    }
};

// MULTI: more than one RK4 step per interval (the initial sensitivity column is then a carried variable
// instead of a lane pattern the compiler rematerialises for free: 28 more VGPRs for M2, hence a separate build)
// MODE 0: every (instance, stage) of the batch, between two launches of the QP kernel (the plain path).
// MODE 1: speculative, for the NEXT tick, while the QP launch of tick P.tick is still running (second stream, its workgroups fill the
//         compute units that launch vacates in its tail): a group goes ahead only if its instance's results of that tick are final
//         AND so are those of the instance that still owns the group's planes under the running launch's map; otherwise it marks the
//         instance for MODE 2.  The iterate is read with loads that bypass the non-coherent L2s (lanes::ld_shared).
// MODE 2: fix-up after that launch: only the instances MODE 1 marked.
// MODE 3: MODE 1 with its grid walked in the order the running launch retires its instances (run_item, lin_order.hpp), by one-wave
//         workgroups: one fits into the registers a single leaving QP wave frees.
// MODE 4: MODE 2 as one wave per group, which leaves at once when its instance has no mark (run_marked).
// (which pair a launch takes: usvmpc.hip launch_solve)
template <class M, int KCH, bool SOFT, bool MULTI = false, int MODE = 0>
struct Linearize {
    static constexpr int NX = M::NX, NU = M::NU, NZ = NX + NU;
    using WL = WsLayout<M, KCH, SOFT>;
    static constexpr bool SPEC = MODE == 1 || MODE == 3, FIXUP = MODE == 2 || MODE == 4;

    // gid = k * Bp + g  (groups of a wave share the stage k): the whole-batch order of MODE 0
    USV_DEV static void run(const DevPtrs &P, long gid)
    {
        const long Bp = lanes::uniform(P.spec->Bp);
        const int k = (int)(gid / Bp);
        run_at(P, k, gid - (long)k * Bp);
    }

    // MODE 3: work item -> (group, stage) in the order the running QP launch retires its instances (lin_order.hpp); the four groups of a
    // wave are neighbouring stages of one instance (two at an instance's end)
    USV_DEV static void run_item(const DevPtrs &P, long item)
    {
        const LinItem it = lin_item(item, P.spec->N, (long)P.spec->B, P.perm_cur, P.inv_next);
        run_at(P, it.k, it.g);
    }

    // MODE 4: group g's marked stages, row r of the wave taking the stages k = r, r + 4, ...  A wave whose instance has no mark - nearly
    // all of them - leaves after reading the instance's redo words once.
    USV_DEV static void run_marked(const DevPtrs &P, long g, int row)
    {
        const int N = lanes::uniform(P.spec->N);
        const long gi = lin_slot(g, (long)lanes::uniform(P.spec->B));
        const long b = P.perm ? (long)P.perm[gi] : gi;
        int any = 0;
        for (int w = 0; w < P.redo_words; w++) any |= P.redo[b * P.redo_words + w];
        if (any == 0) return;
        for (int k = row; k <= N; k += lanes::WAVE_ROWS) run_at(P, k, g);
    }

    // stage k of group g
    USV_DEV static void run_at(const DevPtrs &P, const int k, const long g)
    {
        const DevSpec &S = *P.spec;
        const int lane = lanes::lane();
        const int N = lanes::uniform(S.N), K = lanes::uniform(S.K);
        const long Bp = lanes::uniform(S.Bp);
        const long gi = lin_slot(g, (long)lanes::uniform(S.B)); // padded groups replay the last instance
        const long b = P.perm ? (long)P.perm[gi] : gi;
        if constexpr (SPEC) {
            const long owner = P.perm_cur ? (long)P.perm_cur[gi] : gi;
            const bool ready = lanes::observe(P.epoch + b) == P.tick && lanes::observe(P.epoch + owner) == P.tick;
            if (!ready) { // (the whole 16-lane group leaves: nothing below crosses groups)
                if (lane == 0) lanes::set_bits(P.redo + b * P.redo_words + (k >> 5), 1 << (k & 31)); // this stage of this instance: later
                return;
            }
        }
        if constexpr (FIXUP) {
            if (((P.redo[b * P.redo_words + (k >> 5)] >> (k & 31)) & 1) == 0) return;
        }
        auto ld = [](const double *q) { // the iterate: handed over by a kernel that may still be running (MODE 1, 3)
            if constexpr (SPEC) return lanes::ld_shared(q);
            else return *q;
        };
        // workspace: [stage][group][plane][16 lanes] (lanes::Planes)
        double *tile = P.ws + (((long)k * Bp + g) * lanes::uniform(S.npt)) * LANES + lane;
        const bool xlane = lane >= NU && lane < NZ;

        double x[NX], U[NU > 0 ? NU : 1];
        const double *xk = P.x + ((long)b * (N + 1) + k) * NX;
        sfor<0, NX>([&](auto i) { x[i] = ld(xk + i); });
        if (k < N) {
            const double *uk = P.u + ((long)b * N + k) * NU;
            sfor<0, NU>([&](auto i) { U[i] = ld(uk + i); });
        } else {
            sfor<0, NU>([&](auto i) { U[i] = 0.0; });
        }

        // ---- cost gradient, reference part: -Mc yref (stage) | -Me yref_e (terminal).  The QP kernel keeps its iterate in
        // absolute form (zbar + z), so the gradient at it is this plus H (zbar + z): the H zbar term is not formed here ----
        {
            const double *Mrow = (k < N ? S.Mc : S.Me) + lane * LANES;
            const double *yr = (k < N) ? P.yref + ((long)b * N + k) * S.ny : P.yref_e + (long)b * S.ny_e;
            const int ny = (k < N) ? S.ny : S.ny_e;
            double acc = 0.0;
            for (int y = 0; y < ny; y++) acc = fma(-Mrow[y], yr[y], acc);
            tile[WL::P_GQ * LANES] = acc;
        }
        if (k == N) return; // wave-uniform

        // ---- ERK4 + forward VDE for this lane's sensitivity column; sim_steps steps of size dt / sim_steps
        // (acados sim_method_num_steps; the reference leaves it at 1): the column is simply carried on ----
        const int nsteps = MULTI ? S.sim_steps : 1;
        const double dt = S.dt / (double)nsteps;
        double s0[NX], f[NX], js[NX], xs[NX], ss[NX], xa[NX], sa[NX], su[NU > 0 ? NU : 1];
        sfor<0, NU>([&](auto l) { su[l] = (lane == l) ? 1.0 : 0.0; });
        sfor<0, NX>([&](auto i) { s0[i] = (lane == NU + i) ? 1.0 : 0.0; });
        using MC = ModelCall<M>;
        const typename MC::Pre pre = MC::prepare(x);
        for (int step = 0; step < nsteps; step++) { // wave-uniform
            MC::fjvp(pre, x, U, s0, su, f, js);
            sfor<0, NX>([&](auto i) {
                xa[i] = f[i];
                sa[i] = js[i];
                xs[i] = fma(0.5 * dt, f[i], x[i]);
                ss[i] = fma(0.5 * dt, js[i], s0[i]);
            });
            MC::fjvp(pre, xs, U, ss, su, f, js);
            sfor<0, NX>([&](auto i) {
                xa[i] = fma(2.0, f[i], xa[i]);
                sa[i] = fma(2.0, js[i], sa[i]);
                xs[i] = fma(0.5 * dt, f[i], x[i]);
                ss[i] = fma(0.5 * dt, js[i], s0[i]);
            });
            MC::fjvp(pre, xs, U, ss, su, f, js);
            sfor<0, NX>([&](auto i) {
                xa[i] = fma(2.0, f[i], xa[i]);
                sa[i] = fma(2.0, js[i], sa[i]);
                xs[i] = fma(dt, f[i], x[i]);
                ss[i] = fma(dt, js[i], s0[i]);
            });
            MC::fjvp(pre, xs, U, ss, su, f, js);
            sfor<0, NX>([&](auto i) {
                x[i] = fma(dt / 6.0, xa[i] + f[i], x[i]);
                sa[i] = fma(dt / 6.0, sa[i] + js[i], s0[i]);
                if constexpr (MULTI) s0[i] = sa[i];
            });
        }
        const double *xn = P.x + ((long)b * (N + 1) + k + 1) * NX;
        double bres = 0.0;
        sfor<0, NX>([&](auto i) { bres = (lane == NU + i) ? x[i] - ld(xn + i) : bres; });
        // lane r now holds row r of [B A]' (sa[i] = d x+_i / d z_r).  The structurally informative entries (MatPack:
        // M::SENS) are packed into MatPack<M>::NPK planes: lane L of plane q stores entry number 16 q + L of the
        // stream, i.e. for the row j whose range contains it the value sa[j] held by the lane of its column - a lane
        // gather per row that the plane touches.
        using MP = MatPack<M>;
        sfor<0, MP::NPK>([&](auto q) {
            const int sidx = 16 * q + lane;
            double val = 0.0;
            sfor<0, NX>([&](auto j) {
                constexpr int s0 = MP::start(j), cnt = MP::count(j);
                if constexpr (cnt > 0 && s0 < 16 * q + 16 && s0 + cnt > 16 * q) {
                    const int within = sidx - s0;
                    int c_l = 0; // lane that owns this entry's column
                    sfor<0, cnt>([&](auto ci) { c_l = (within == ci) ? MP::nth(MP::row_mask(j), ci) : c_l; });
                    const double gth = lanes::gather(sa[j], c_l);
                    val = (within >= 0 && within < cnt) ? gth : val;
                }
            });
            tile[(WL::P_MAT + q) * LANES] = val;
        });
        tile[WL::P_RB0 * LANES] = xlane ? bres : 0.0;
        // (obstacle rows are linearised inside the QP kernel from the iterate and (p, lh): QpIpm::obs_geom)
    }

    // ------------------------------------------------------------------------------------------------------------------------------------
    // Two (instance, stage) pairs per 16-lane row, for models that say which at most 8 columns need integrating (PairCols, params.hpp):
    // lane L serves half L >> 3 of the row and integrates the column of slot L & 7 with exactly the arithmetic the lane of that column runs
    // in run_at; nothing crosses a row, every exchange is a gather among the 8 lanes of a half.  Each plane still has 16 entries, so a lane
    // stores two of them (entry e = slot and slot + 8).  Control flow is uniform over a ROW: a half with nothing to do (nothing there,
    // terminal stage, not ready, not marked) keeps its lanes going on valid addresses and stores nothing.  Same bits as run_at.
    using PC = PairCols<M>;
    static constexpr int HALF = LANES / 2;

    // MODE 0 / 1 / 2: the halves in stage-major order (lin_order.hpp); n = (N + 1) Bp pairs
    USV_DEV static void run_pair(const DevPtrs &P, long row)
    {
        const LinItem it = lin_pair_plain(row, lanes::lane() >> 3, P.spec->N, (long)P.spec->Bp);
        run_pair_at(P, it.k < 0 ? 0 : it.k, it.g, it.k >= 0);
    }

    // MODE 3: the retire order; the two halves of a row are neighbouring stages of ONE instance
    USV_DEV static void run_pair_item(const DevPtrs &P, long row)
    {
        const LinItem it = lin_pair_retire(row, lanes::lane() >> 3, P.spec->N, (long)P.spec->B, (long)P.spec->Bp, P.perm_cur, P.inv_next);
        run_pair_at(P, it.k < 0 ? 0 : it.k, it.g, it.k >= 0);
    }

    // MODE 4: group g's marked stages shared out over the 2 x WAVE_ROWS halves of its wave
    USV_DEV static void run_pair_marked(const DevPtrs &P, long g, int row)
    {
        const int N = lanes::uniform(P.spec->N);
        const long gi = lin_slot(g, (long)lanes::uniform(P.spec->B));
        const long b = P.perm ? (long)P.perm[gi] : gi;
        int any = 0;
        for (int w = 0; w < P.redo_words; w++) any |= P.redo[b * P.redo_words + w];
        if (any == 0) return;
        const int half = lanes::lane() >> 3;
        for (int t = 0; lin_pair_marked(t, row, 0, lanes::WAVE_ROWS) <= N; t++) { // (row-uniform: the first half's stage)
            const int k = lin_pair_marked(t, row, half, lanes::WAVE_ROWS);
            run_pair_at(P, k <= N ? k : N, g, k <= N);
        }
    }

    // stage k of group g in this lane's half of the row; !live: nothing there (k, g are then any valid pair)
    USV_DEV static void run_pair_at(const DevPtrs &P, const int k, const long g, const bool live)
    {
        const DevSpec &S = *P.spec;
#ifdef USV_LANES_OPAQUE // (run_pair_marked calls this in a loop: hoisted out of it, the lane patterns below - unit columns, entry selects - cost
                        // some 30 registers, which spill)
        const int lane = lanes::opaque(lanes::lane());
#else
        const int lane = lanes::lane();
#endif
        const int slot = lane & (HALF - 1), hb = lane & HALF;
        const int N = lanes::uniform(S.N);
        const long Bp = lanes::uniform(S.Bp);
        const long gi = lin_slot(g, (long)lanes::uniform(S.B));
        const long b = P.perm ? (long)P.perm[gi] : gi;
        bool act = live;
        if constexpr (SPEC) {
            const long owner = P.perm_cur ? (long)P.perm_cur[gi] : gi;
            const bool ready = lanes::observe(P.epoch + b) == P.tick && lanes::observe(P.epoch + owner) == P.tick;
            if (live && !ready && slot == 0) lanes::set_bits(P.redo + b * P.redo_words + (k >> 5), 1 << (k & 31)); // this stage of this instance: later
            act = live && ready;
        }
        if constexpr (FIXUP) act = act && ((P.redo[b * P.redo_words + (k >> 5)] >> (k & 31)) & 1) != 0;
        const bool integ = act && k < N;
        // the row leaves, or ends after the cost gradient, only as a whole: what the other half has to do
        const int mine = (act ? 1 : 0) | (integ ? 2 : 0);
        const int both = mine | (int)lanes::gather((double)mine, lane ^ HALF);
        if (both == 0) return;
        auto ld = [](const double *q) {
            if constexpr (SPEC) return lanes::ld_shared(q);
            else return *q;
        };
        double *tile = P.ws + (((long)k * Bp + g) * lanes::uniform(S.npt)) * LANES + slot; // entry `slot` of plane 0; entry slot + 8: + HALF
        const int ku = k < N ? k : N - 1; // (a half at the terminal stage idles through the integration on the interval before it)

        double x[NX], U[NU > 0 ? NU : 1];
        const double *xk = P.x + ((long)b * (N + 1) + ku) * NX;
        sfor<0, NX>([&](auto i) { x[i] = ld(xk + i); });
        const double *uk = P.u + ((long)b * N + ku) * NU;
        sfor<0, NU>([&](auto i) { U[i] = ld(uk + i); });

        {   // cost gradient, reference part (run_at)
            const bool st = k < N;
            const double *yr = st ? P.yref + ((long)b * N + k) * S.ny : P.yref_e + (long)b * S.ny_e;
            const int ny = st ? S.ny : S.ny_e;
            sfor<0, 2>([&](auto h2) {
                const double *Mrow = (st ? S.Mc : S.Me) + (slot + HALF * h2) * LANES;
                double acc = 0.0;
                for (int y = 0; y < ny; y++) acc = fma(-Mrow[y], yr[y], acc);
                if (act) tile[WL::P_GQ * LANES + HALF * h2] = acc;
            });
        }
        if ((both & 2) == 0) return; // row-uniform

        // ---- ERK4 + forward VDE (run_at) for the column of this lane's slot; the quadrature entries accumulate beside it, in every lane,
        // by the operations the lane of the entry's column would perform on its sa[row] ----
        constexpr int NQ = PC::NQUAD;
        const int nsteps = MULTI ? S.sim_steps : 1;
        const double dt = S.dt / (double)nsteps;
        int col = -1;
        sfor<0, PC::NCOL>([&](auto c) {
            constexpr int var = PC::col(decltype(c)::value);
            col = (slot == c) ? var : col;
        });
        double s0[NX], f[NX], js[NX], xs[NX], ss[NX], xa[NX], sa[NX], su[NU > 0 ? NU : 1];
        double qd[NQ > 0 ? NQ : 1], qa[NQ > 0 ? NQ : 1], q0[NQ > 0 ? NQ : 1];
        sfor<0, NU>([&](auto l) { su[l] = (col == l) ? 1.0 : 0.0; });
        sfor<0, NX>([&](auto i) { s0[i] = (col == NU + i) ? 1.0 : 0.0; });
        sfor<0, NQ>([&](auto e) { q0[e] = 0.0; });
        using MC = ModelCall<M>;
        using MQ = ModelQuad<M>;
        const typename MC::Pre pre = MC::prepare(x);
        for (int step = 0; step < nsteps; step++) { // wave-uniform
            MQ::fjvp(pre, x, U, s0, su, f, js, qd);
            sfor<0, NX>([&](auto i) {
                xa[i] = f[i];
                sa[i] = js[i];
                xs[i] = fma(0.5 * dt, f[i], x[i]);
                ss[i] = fma(0.5 * dt, js[i], s0[i]);
            });
            sfor<0, NQ>([&](auto e) { qa[e] = qd[e]; });
            MQ::fjvp(pre, xs, U, ss, su, f, js, qd);
            sfor<0, NX>([&](auto i) {
                xa[i] = fma(2.0, f[i], xa[i]);
                sa[i] = fma(2.0, js[i], sa[i]);
                xs[i] = fma(0.5 * dt, f[i], x[i]);
                ss[i] = fma(0.5 * dt, js[i], s0[i]);
            });
            sfor<0, NQ>([&](auto e) { qa[e] = fma(2.0, qd[e], qa[e]); });
            MQ::fjvp(pre, xs, U, ss, su, f, js, qd);
            sfor<0, NX>([&](auto i) {
                xa[i] = fma(2.0, f[i], xa[i]);
                sa[i] = fma(2.0, js[i], sa[i]);
                xs[i] = fma(dt, f[i], x[i]);
                ss[i] = fma(dt, js[i], s0[i]);
            });
            sfor<0, NQ>([&](auto e) { qa[e] = fma(2.0, qd[e], qa[e]); });
            MQ::fjvp(pre, xs, U, ss, su, f, js, qd);
            sfor<0, NX>([&](auto i) {
                x[i] = fma(dt / 6.0, xa[i] + f[i], x[i]);
                sa[i] = fma(dt / 6.0, sa[i] + js[i], s0[i]);
                if constexpr (MULTI) s0[i] = sa[i];
            });
            sfor<0, NQ>([&](auto e) {
                qa[e] = fma(dt / 6.0, qa[e] + qd[e], q0[e]);
                if constexpr (MULTI) q0[e] = qa[e];
            });
        }
        const double *xn = P.x + ((long)b * (N + 1) + ku + 1) * NX;
        double bres[2] = {0.0, 0.0};
        // (the difference stays inside the conditional arm, as in run_at: the compiler then keeps what only x[i] needs of the last RK stage under
        // the same condition in both forms, and contracts the rest of that stage alike - with it hoisted out, single-step kernels differed in the
        // last place of [B A])
        sfor<0, NX>([&](auto i) {
            constexpr int e = NU + decltype(i)::value;
            if constexpr (e < HALF) bres[0] = (slot == e) ? x[i] - ld(xn + i) : bres[0];
            else bres[1] = (slot == e - HALF) ? x[i] - ld(xn + i) : bres[1];
        });
        // the MatPack stream (run_at): entry 16 q + e comes from the lane of ITS half that integrated the entry's column, or is a quadrature
        using MP = MatPack<M>;
        sfor<0, MP::NPK>([&](auto q) {
            sfor<0, 2>([&](auto h2) {
                const int sidx = 16 * q + slot + HALF * h2;
                double val = 0.0;
                sfor<0, NX>([&](auto j) {
                    constexpr int jj = decltype(j)::value, qq = decltype(q)::value;
                    constexpr int st0 = MP::start(jj), cnt = MP::count(jj);
                    if constexpr (cnt > 0 && st0 < 16 * qq + 16 && st0 + cnt > 16 * qq) {
                        const int within = sidx - st0;
                        int c_l = 0; // slot that owns this entry's column
                        sfor<0, cnt>([&](auto ci) {
                            constexpr int c = MP::nth(MP::row_mask(jj), decltype(ci)::value);
                            constexpr int sl = PC::slot_of(c);
                            if constexpr (PC::quad_of(jj, c) < 0) c_l = (within == decltype(ci)::value) ? sl : c_l;
                        });
                        const double gth = lanes::gather(sa[jj], hb | c_l);
                        val = (within >= 0 && within < cnt) ? gth : val;
                        sfor<0, cnt>([&](auto ci) {
                            constexpr int c = MP::nth(MP::row_mask(jj), decltype(ci)::value);
                            constexpr int qe = PC::quad_of(jj, c);
                            if constexpr (qe >= 0) val = (within == decltype(ci)::value) ? qa[qe] : val;
                        });
                    }
                });
                if (integ) tile[(WL::P_MAT + q) * LANES + HALF * h2] = val;
            });
        });
        if (integ) {
            tile[WL::P_RB0 * LANES] = bres[0];
            tile[WL::P_RB0 * LANES + HALF] = bres[1];
        }
    }
};

} // namespace usv
