// fleet_plan.hpp — vessel encounters with exchanged plans (usvmpc_pf_fleet_plans / usvmpc_guidance_fleet_plans): a scene-mate is itself a
// vessel of this batch, and its own NMPC has just solved where it will go.  With plans on, the stages 1 .. N of a slot that holds a
// scene-mate follow the mate's planned path x[j][1 .. N] instead of the straight line pos + (k dt) vel.  Pure functions, host + device, no
// dependency on the kernels (usvmpc.hip: fleet_plan_body, usv_pf_fleet_plans, usv_guidance_fleet_plans; tests/fleet_plans_harness.cpp).
//     instance i, slot s, list index c = chosen[i][s] (the decide step's choice; -1: parked, or i does not stream this tick)
//     source vessel     j = fleet_vessel(i, c - n_fixed, S) when c >= n_fixed, else none (a fixed entry or a parked slot)
//     P_k               the position pair of x[j][k]: states Fleet::PX, Fleet::PY (10, 11 for usv_model_pf_ca; 5, 6 for usv_model_guidance_ca1)
//     q                 the slot's stage-0 position as the decide step left it in trk_pv (the guidance model's is float32-rounded, as ever)
//     e                 = q - P_1: the mate's iterate is one hand-over old, so its stage 1 is now; what the plant and the disturbance did to
//                       the mate since is carried along the whole plan
//     p[i][0][s]        stays q
//     p[i][k][s]        = P_{k+1} + e                        k = 1 .. N - 1
//     p[i][N][s]        = (P_N + (P_N - P_{N-1})) + e        the plan's last step once more
//     lh                untouched
// A plan is used only when the handle's plan state says the iterate is exactly one hand-over old (world_plan.hpp: PLAN_SHIFTED; the host
// launches the kernel then and only then), instance i streams this tick, mate j's mission is not over (finish_tick[j] < 0 after this
// prepare) and status[j] of the last solve is 0.  Every other slot keeps the constant-velocity bits the prepare wrote.
// Sums and differences only, each rounded on its own (no product: nothing a compiler could contract; the pragma is kept as in
// fleet_world.hpp), so numpy gives the same bits (scenario.fleet_plan_stages).  N >= 2 (the entry points refuse N = 1).
#pragma once

#include "ca_fleet_world.hpp"
#include "fleet_world.hpp"

namespace usv {

// the vessel whose plan feeds a slot that holds list index c of instance i; -1: none
USV_HD long fleet_plan_vessel(long i, int c, int n_fixed, int S)
{
    return (c >= n_fixed && c - n_fixed < S - 1) ? fleet_vessel(i, c - n_fixed, S) : -1;
}

// ... and whether that plan may be used: the mate's mission is not over and its last solve succeeded
USV_HD long fleet_plan_source(long i, int c, int n_fixed, int S, const int *finish_tick, const int *status)
{
    const long j = fleet_plan_vessel(i, c, n_fixed, S);
    return (j >= 0 && finish_tick[j] < 0 && status[j] == 0) ? j : -1;
}

// stage k (1 <= k <= N) of a slot fed by the plan xj ([N + 1][Fleet::NX]) whose stage-0 position is q
template <class Fleet>
USV_HD void fleet_plan_pair(const double *xj, int N, int k, double qx, double qy, double &ox, double &oy)
{
    USV_FLEET_NOFMA
    const double *P1 = xj + Fleet::NX;
    const double ex = qx - P1[Fleet::PX], ey = qy - P1[Fleet::PY];
    if (k < N) {
        const double *P = xj + (long)(k + 1) * Fleet::NX;
        ox = P[Fleet::PX] + ex;
        oy = P[Fleet::PY] + ey;
    } else {
        const double *PN = xj + (long)N * Fleet::NX, *PM = PN - Fleet::NX;
        ox = (PN[Fleet::PX] + (PN[Fleet::PX] - PM[Fleet::PX])) + ex;
        oy = (PN[Fleet::PY] + (PN[Fleet::PY] - PM[Fleet::PY])) + ey;
    }
}

// One instance, as the kernel's threads do it between them.  x [B][N + 1][NX], status [B], finish_tick [B]: the whole batch's; chosen [K]
// (all -1 when the instance does not stream), pv [K][4] the slot tracks (X, Y, vX, vY), p [N + 1][2K] the instance's stages as the prepare
// left them, source [K] out.  -> the number of plan-fed slots
template <class Fleet>
USV_HD int fleet_plan_instance(const double *x, const int *status, const int *finish_tick, long i, int S, int n_fixed, int N, int K,
                               const int *chosen, const double *pv, double *p, int *source)
{
    int fed = 0;
    for (int s = 0; s < K; s++) {
        const long j = fleet_plan_source(i, chosen[s], n_fixed, S, finish_tick, status);
        source[s] = (int)j;
        if (j < 0) continue;
        fed++;
        const double *xj = x + j * (long)(N + 1) * Fleet::NX;
        for (int k = 1; k <= N; k++)
            fleet_plan_pair<Fleet>(xj, N, k, pv[4 * s], pv[4 * s + 1], p[(long)k * 2 * K + 2 * s], p[(long)k * 2 * K + 2 * s + 1]);
    }
    return fed;
}

} // namespace usv
