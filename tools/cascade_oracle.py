#!/usr/bin/env python3
"""The two-layer control stack of guidance.Cascade in closed loop ON THE CPU: for the guidance layer the reference node's arithmetic from
the CPU oracle (oracle.binding.obstacle_sim / guidance_prepare / guidance_publish, per instance) and the oracle's SQP-RTI step on
usv_model_guidance_ca1; for the low-level layer the oracle's SQP-RTI step on usv_model_low_level through its generated-model hook
(codegen.emit_oracle_c -> register_generated -> spec_from_ocp) between numpy's restatement of the coupling (scenario.cascade_ll_inputs /
cascade_ll_outputs) and of the vessel (scenario.cascade_plant_step).  The loop guidance.Cascade runs on the device, restated without one.
No GPU, no solver library.

Prints, for scenario.make_ca_missions, finish ticks, minimum clearance and failed solves per layer - and beside them the same missions
closed on the guidance model's own kinematic prediction (x0 <- x_1, what advance does).  It is the yardstick the device's cascade is held
against (profiles/cascade_oracle.txt; tests/test_gpu_cascade.py runs `run` itself).

    python tools/cascade_oracle.py --batch 64 --ticks 900 --write
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_collisionavoidance_amd import codegen, scenario, usv_models  # noqa: E402
from oracle import binding as oracle  # noqa: E402

MODEL_GUIDANCE_CA1 = 1
WORK = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc", "gen")


def low_level_spec(N, dt):
    """The oracle's spec of usv_model_low_level (model id MGEN: registered from the generated plain-C model)"""
    ocp = usv_models.make_ocp("usv_model_low_level", N * dt, N)
    os.makedirs(WORK, exist_ok=True)
    oracle.register_generated(codegen.emit_oracle_c(codegen.analyse(ocp.model)), WORK)
    return oracle.spec_from_ocp(ocp, oracle.MGEN)


def _clearance(pose, world, max_radius):
    r = np.sqrt((pose[0] - world[:, 0]) ** 2 + (pose[1] - world[:, 1]) ** 2)
    vis = r < max_radius
    return (r[vis] - (world[vis, 2] + 0.5)).min() if vis.any() else 1e300


def run(m, gticks, N=100, K=8, dt=0.05, ll_N=100, ratio=5, num_steps=1, c=scenario.CASCADE_C, max_radius=100.0, threads=1, cascade=True,
        record=False):
    """m: scenario.make_ca_missions(...).  gticks guidance ticks (gticks * ratio low-level ticks).  cascade=False: the same missions closed on
    the guidance model's kinematic prediction.  Returns dict(finish_tick [B] (guidance ticks, -1: not finished), min_clearance [B],
    guidance_failures, low_level_failures, max_qp_iter, state [B,6] (the vessel at the end); record: also states [gticks * ratio + 1, B, 6])."""
    B = m["pose"].shape[0]
    wps = np.tile(np.asarray(m["waypoints"], dtype=float)[None], (B, 1, 1)) if np.ndim(m["waypoints"]) == 2 else np.asarray(m["waypoints"], dtype=float)
    npts = wps.shape[1]
    world = np.asarray(m["world"], dtype=float)
    T = dt / ratio
    gspec = oracle.spec(MODEL_GUIDANCE_CA1, N, N * dt, K)
    st = [oracle.guidance_reset(wps[b].ravel(), m["pose"][b, 2]) for b in range(B)]
    k, pp = np.array([s[0] for s in st]), np.array([s[1] for s in st], dtype=np.float32)
    S = np.column_stack([m["pose"], m["vel"], np.zeros(B)])                  # the vessel (nedx, nedy, psi, u, v, r)
    X0 = np.zeros((B, 8))                                                    # the guidance solver's x0 as the device holds it
    X0[:, 0:2], X0[:, 5:8] = S[:, 3:5], S[:, 0:3]
    gx = np.ascontiguousarray(np.tile(np.zeros(8)[None, None], (B, N + 1, 1)))   # (acados_create: x_k = constraints.x0 = 0, u = 0)
    gu = np.zeros((B, N, 1))
    p, lh = np.tile(100.0 * np.ones(2 * K), (B, N + 1, 1)), np.tile(1.5 * np.ones(K), (B, N, 1))
    gyref, gyref_e = np.zeros((B, N, 9)), np.zeros((B, 8))
    heading, speed = np.zeros(B), np.zeros(B)
    active = np.zeros(B, dtype=int)
    ak = np.zeros(B)
    finish, min_clear = np.full(B, -1), np.full(B, 1e300)
    gfail = lfail = 0
    max_it = 0
    if cascade:
        lspec = low_level_spec(ll_N, T)
        past = np.zeros((B, 2))
        lx0, _ = scenario.cascade_ll_inputs(S, past, np.zeros(B), np.zeros(B))
        lx = np.ascontiguousarray(np.tile(lx0[:, None, :], (1, ll_N + 1, 1)))
        lu = np.zeros((B, ll_N, 2))
        lp, llh = np.zeros((B, ll_N + 1, 0)), np.zeros((B, ll_N, 0))
    states = [S.copy()]
    for g in range(gticks):
        # ---- the guidance layer: usv_guidance_tick -> solve -> usv_guidance_post
        for b in range(B):
            if k[b] >= npts:
                if finish[b] < 0:
                    finish[b] = g
                continue
            pose = X0[b, 5:8]
            body, n = oracle.obstacle_sim(pose, world[b], max_radius)
            r = oracle.guidance_prepare(K, X0[b, 0:2], pose, wps[b].ravel(), body, k[b], pp[b])
            min_clear[b] = min(min_clear[b], _clearance(pose, world[b], max_radius))
            p[b, 0], lh[b, 0] = r["p_obs"], r["r_obs"]
            p[b, 1:], lh[b, 1:] = r["p_obs"][None], r["r_obs"][None]       # (a world at rest: "static_obstacles", stage 0 serves every stage)
            k[b], active[b] = r["k"], r["active"]
            if r["active"]:
                X0[b], pp[b], ak[b] = r["x0"], r["past_psied"], r["ak"]
            else:
                finish[b] = g
        status, its = oracle.rti_batch(gspec, gx, gu, X0, gyref, gyref_e, p, lh, threads=threads)
        gfail += int((status != 0).sum())
        max_it = max(max_it, int(its.max()))
        for b in range(B):
            if active[b]:
                o = oracle.guidance_publish(gx[b, 1, 4], gu[b, 0, 0], ak[b], pp[b])
                heading[b], speed[b], pp[b] = o["heading"], o["speed"], o["past_psied"]
            else:
                heading[b], speed[b] = 0.0, 0.0
        if not cascade:
            X0[:] = gx[:, 1]                                                 # advance: the plant is the controller's prediction
            S[:, 0:3], S[:, 3:5] = X0[:, 5:8], X0[:, 0:2]
            states.append(S.copy())
            continue
        # ---- `ratio` low-level ticks: usv_cascade_refs -> solve -> usv_cascade_step
        for i in range(ratio):
            lx0, row = scenario.cascade_ll_inputs(S, past, heading, speed)
            lyref, lyref_e = np.ascontiguousarray(np.tile(row[:, None, :], (1, ll_N, 1))), np.ascontiguousarray(row[:, :8])
            status, its = oracle.rti_batch(lspec, lx, lu, lx0, lyref, lyref_e, lp, llh, threads=threads)
            lfail += int((status != 0).sum())
            max_it = max(max_it, int(its.max()))
            thr, past, _, _ = scenario.cascade_ll_outputs(lx[:, 1], heading, speed, S)
            S = scenario.cascade_plant_step(S, thr, T, num_steps, c)
            states.append(S.copy())
        X0[:, 0:2], X0[:, 5:8] = S[:, 3:5], S[:, 0:3]                        # the hand-over: x0[0, 1, 5, 6, 7]
    out = dict(finish_tick=finish, min_clearance=min_clear, guidance_failures=gfail, low_level_failures=lfail, max_qp_iter=max_it, state=S)
    if record:
        out["states"] = np.array(states)
    return out


def report(name, r, B):
    fin = r["finish_tick"] >= 0
    return ["%s:" % name,
            "  finished %d of %d%s" % (fin.sum(), B, ", at guidance ticks %d .. %d (median %d)" % (
                r["finish_tick"][fin].min(), r["finish_tick"][fin].max(), int(np.median(r["finish_tick"][fin]))) if fin.any() else ""),
            "  smallest min_clearance %.4f m (median %.4f, largest %.4f)" % (r["min_clearance"].min(), np.median(r["min_clearance"]), r["min_clearance"].max()),
            "  failed solves: guidance %d, low level %d; at most %d IPM iterations" % (r["guidance_failures"], r["low_level_failures"], r["max_qp_iter"])]


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--obstacles", type=int, default=6)
    ap.add_argument("--ticks", type=int, default=900, help="guidance ticks")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--ll-horizon", type=int, default=100)
    ap.add_argument("--ll-dt", type=float, default=0.01)
    ap.add_argument("--ratio", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--write", action="store_true", help="also write profiles/cascade_oracle.txt")
    a = ap.parse_args()
    m = scenario.make_ca_missions(a.batch, a.obstacles, seed=a.seed)
    kw = dict(N=a.horizon, ll_N=a.ll_horizon, ratio=a.ratio, dt=a.ratio * a.ll_dt, threads=a.threads)
    text = ["# tools/cascade_oracle.py --batch %d --obstacles %d --ticks %d --seed %d --horizon %d --ll-horizon %d --ll-dt %g --ratio %d" % (
        a.batch, a.obstacles, a.ticks, a.seed, a.horizon, a.ll_horizon, a.ll_dt, a.ratio),
        "# scenario.make_ca_missions on the CPU oracle: the yardstick of tests/test_gpu_cascade.py"]
    text += report("cascade (guidance -> low-level NMPC -> 3-DOF vessel)", run(m, a.ticks, cascade=True, **kw), a.batch)
    text += report("kinematic loop (x0 <- x_1 of the guidance model)", run(m, a.ticks, cascade=False, **kw), a.batch)
    print("\n".join(text), flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "cascade_oracle.txt"), "w") as f:
            f.write("\n".join(text) + "\n")
