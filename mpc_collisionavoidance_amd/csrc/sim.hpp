// sim.hpp — the batched integrator: acados' sim_erk (AcadosSimSolver) and the closed-loop plant step.
//
// `num_steps` RK4 steps of size T / num_steps over one sampling period, through the same ModelCall<M> prepare / fjvp calls the
// lineariser makes (linearize.hpp): prepare once at the start of the period, four fjvp per step.  Two mappings:
//   SENS = false  one lane per instance (64 instances per wave).  fjvp is called with a zero tangent, so a generated model needs
//                 nothing beyond the interface it already has; the tangent arithmetic is dead and the compiler drops it.
//   SENS = true   one 16-lane group per instance.  Lane c integrates column c of the forward sensitivities alongside the nominal
//                 state, as the lineariser's lane r does (the variational equation is linear in S, column by column); every lane
//                 carries the same nominal stage points, so x_next is the same bits in both mappings.
// Output layout: x_next [B][nx] and S_forw [B][nx][nx + nu] = [Sx | Su] row-major, i.e. lane c < nx holds d x+ / d x_c and lane
// nx + l holds d x+ / d u_l.  That is acados_template's S_forw (AcadosSimSolver.get("S_forw"), "Sx", "Su") AS RECALLED: the acados
// sources are not part of this tree.  Lanes beyond nx + nu and instances beyond B store nothing.
#pragma once
#include "lanes.hpp"
#include "linearize.hpp"
#include "sfor.hpp"

namespace usv {

// A copy of v the compiler cannot see through: it keeps the tangent evaluation's expression DAG apart from the nominal one's
USV_DEV double opaque(double v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// f and the tangent J (s, su) at the stage point xs.  The nominal f is evaluated with a zero tangent, exactly as when SENS is off;
// the tangent comes from a second evaluation on opaque copies of the point.  (Evaluated together, the two share products, and the
// backend's choice of which product of a sum to fuse into a multiply-add follows use counts: f - and x_next - would then differ in
// the last bits between the two mappings.)
template <class M, bool SENS>
USV_DEV void stage_eval(const typename ModelCall<M>::Pre &pre, const double *xs_start, const double *xs, const double *U, const double *ss,
                        const double *su, double *f, double *js)
{
    constexpr int NX = M::NX, NU = M::NU;
    using MC = ModelCall<M>;
    double z[NX], zu[NU > 0 ? NU : 1], junk[NX];
    sfor<0, NX>([&](auto i) { z[i] = 0.0; });
    sfor<0, NU>([&](auto l) { zu[l] = 0.0; });
    MC::fjvp(pre, xs, U, z, zu, f, junk);
    if constexpr (SENS) {
        double xo[NX], x0o[NX], Uo[NU > 0 ? NU : 1];
        sfor<0, NX>([&](auto i) { xo[i] = opaque(xs[i]); x0o[i] = opaque(xs_start[i]); });
        sfor<0, NU>([&](auto l) { Uo[l] = opaque(U[l]); });
        const typename MC::Pre pre_o = MC::prepare(x0o);
        MC::fjvp(pre_o, xo, Uo, ss, su, junk, js);
    }
}

// One period of `steps` RK4 steps from x (in place) under the constant input U, carrying the tangent column (s, su) when SENS.
// The x arithmetic is the lineariser's statement for statement and does not depend on SENS.
template <class M, bool SENS>
USV_DEV void erk_period(double *x, const double *U, double *s, const double *su, double T, int steps)
{
    constexpr int NX = M::NX;
    using MC = ModelCall<M>;
    const double dt = T / (double)steps;
    double x0[NX];
    sfor<0, NX>([&](auto i) { x0[i] = x[i]; });
    const typename MC::Pre pre = MC::prepare(x0);
    double f[NX], js[NX], xs[NX], ss[NX], xa[NX], sa[NX];
    for (int step = 0; step < steps; step++) {
        stage_eval<M, SENS>(pre, x0, x, U, s, su, f, js);
        sfor<0, NX>([&](auto i) {
            xa[i] = f[i];
            xs[i] = fma(0.5 * dt, f[i], x[i]);
            if constexpr (SENS) { sa[i] = js[i]; ss[i] = fma(0.5 * dt, js[i], s[i]); } else ss[i] = s[i];
        });
        stage_eval<M, SENS>(pre, x0, xs, U, ss, su, f, js);
        sfor<0, NX>([&](auto i) {
            xa[i] = fma(2.0, f[i], xa[i]);
            xs[i] = fma(0.5 * dt, f[i], x[i]);
            if constexpr (SENS) { sa[i] = fma(2.0, js[i], sa[i]); ss[i] = fma(0.5 * dt, js[i], s[i]); }
        });
        stage_eval<M, SENS>(pre, x0, xs, U, ss, su, f, js);
        sfor<0, NX>([&](auto i) {
            xa[i] = fma(2.0, f[i], xa[i]);
            xs[i] = fma(dt, f[i], x[i]);
            if constexpr (SENS) { sa[i] = fma(2.0, js[i], sa[i]); ss[i] = fma(dt, js[i], s[i]); }
        });
        stage_eval<M, SENS>(pre, x0, xs, U, ss, su, f, js);
        sfor<0, NX>([&](auto i) {
            x[i] = fma(dt / 6.0, xa[i] + f[i], x[i]);
            if constexpr (SENS) s[i] = fma(dt / 6.0, sa[i] + js[i], s[i]);
        });
    }
}

// x [B][nx], u [B][nu] -> xn [B][nx] (and S [B][nx][nx + nu] when SENS).  SENS: thread t serves instance t / 16, column t % 16.
template <class M, bool SENS>
USV_DEV void sim_run(const double *xin, const double *uin, double *xn, double *S, long B, double T, int steps)
{
    constexpr int NX = M::NX, NU = M::NU, NZ = NX + NU;
    static_assert(NZ <= LANES, "one sensitivity column per lane of a 16-lane group");
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long b = SENS ? t / LANES : t;
    const int c = SENS ? (int)(t % LANES) : 0;
    if (b >= B) return;
    double x[NX], U[NU > 0 ? NU : 1], s[NX], su[NU > 0 ? NU : 1];
    sfor<0, NX>([&](auto i) { x[i] = xin[b * NX + i]; s[i] = (SENS && c == i) ? 1.0 : 0.0; });
    sfor<0, NU>([&](auto l) { U[l] = uin[b * NU + l]; su[l] = (SENS && c == NX + l) ? 1.0 : 0.0; });
    erk_period<M, SENS>(x, U, s, su, T, steps);
    if constexpr (SENS) {
        if (c >= NZ) return;
        double xc = 0.0;
        sfor<0, NX>([&](auto i) {
            xc = (c == i) ? x[i] : xc;
            S[(b * NX + i) * NZ + c] = s[i];
        });
        if (c < NX) xn[b * NX + c] = xc;
    } else {
        sfor<0, NX>([&](auto i) { xn[b * NX + i] = x[i]; });
    }
}

} // namespace usv
