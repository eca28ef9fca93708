#!/usr/bin/env python3
"""The path-following missions of scenario.make_pf_missions in closed loop ON THE CPU: the numpy front end (tests/pf_frontend_ref.PfRef,
device-resident mode; scenario.predict_world for a moving world) in front of the CPU oracle's SQP-RTI step, the plant being the controller's
prediction x_1 - the loop examples/pf_mission_sweep.py runs on the device, restated without one.  No GPU, no solver library.

Prints finish ticks, clearances and failure counts.  It is the yardstick the device's missions are held against
(profiles/pf_moving_oracle.txt) and the place where the generator's velocity law was settled (--drift-along / --drift-across override
scenario.PF_DRIFT_ALONG / PF_DRIFT_ACROSS).

    python tools/pf_mission_oracle.py --batch 64 --ticks 560                  # a world at rest
    python tools/pf_mission_oracle.py --batch 64 --ticks 700 --moving         # the moving world, predicted per stage
    python tools/pf_mission_oracle.py --batch 64 --ticks 700 --moving --no-predict
    python tools/pf_mission_oracle.py --parity-starts --batch 32 --ticks 25 --moving   # the window of the parity test
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_collisionavoidance_amd import scenario  # noqa: E402
from oracle import binding as oracle  # noqa: E402
from tests import pf_frontend_ref as R  # noqa: E402

MODEL_PF_CA = 2


def run(B, ticks, seed=0, moving=False, predict=True, threads=16, drift=None, parity_starts=False, quiet=False):
    cfg = scenario.PF_MISSION_OCP
    N, K, dt = cfg["N"], cfg["K"], cfg["dt"]
    if drift is not None:
        scenario.PF_DRIFT_ALONG, scenario.PF_DRIFT_ACROSS = drift
    m = scenario.make_pf_missions(B, seed, moving=moving)
    x0 = m["x0"].copy()
    if parity_starts:                    # tests/test_gpu_pf_moving.pf_parity_starts
        rng = np.random.default_rng(1000 + seed)
        first = np.minimum(m["world"][:, 0, 1], m["world"][:, 2, 1])
        x0[:, 0], x0[:, 1], x0[:, 2], x0[:, 3], x0[:, 10] = np.pi / 2, 1.0, 0.0, 0.7, 4.0
        x0[:, 11] = first - rng.uniform(1.0, 3.0, B)
    world = m["world"].copy()
    wvel = m["world_vel"] if moving else np.zeros((B, world.shape[1], 2))
    spec = oracle.spec(MODEL_PF_CA, N, N * dt, K, sim_steps=cfg["sim_steps"])
    fe = R.PfRef(B, N, K, cfg["margin"])
    fe.reset(m["waypoints"])
    fe.set_world(world, cfg["max_radius"])
    fe.x0[:] = x0
    x = np.ascontiguousarray(np.tile(x0[:, None, :], (1, N + 1, 1)))
    u = np.zeros((B, N, 2))
    p, lh = np.zeros((B, N + 1, 2 * K)), np.zeros((B, N, K))
    fails, both_ok, active_rows = np.zeros(ticks, dtype=int), np.zeros(ticks), np.zeros(ticks, dtype=int)
    status = np.zeros(B, dtype=np.int32)
    for t in range(ticks):
        fe.world = world
        fe.prepare()
        live = fe.phase != R.OVER
        if moving and predict:
            pp, ll = scenario.predict_world(world, wvel, fe.chosen, N, dt, margin=cfg["margin"])
        else:
            pp, ll = np.tile(fe.p0[:, None], (1, N + 1, 1)), np.tile(fe.lh0[:, None], (1, N, 1))
        p[live], lh[live] = pp[live], ll[live]
        status, its = oracle.rti_batch(spec, x, u, fe.x0, fe.yref, fe.yref_e, p, lh, threads=threads)
        fails[t] = int((status != 0).sum())
        both_ok[t] = ((status == 0) & (its < spec.opts.qp_iter_max)).mean()
        if parity_starts:                # instances with an obstacle row at its bound somewhere in the horizon
            for b in range(B):
                gap = min((oracle.model_h(MODEL_PF_CA, x[b, k], p[b, k])[0] - lh[b, k]).min() for k in range(1, N))
                active_rows[t] += int(gap < 1e-3)
        fe.publish(x[:, 1])
        fe.x0[:] = x[:, 1]               # the hand-over: the plant is the controller's prediction, no trajectory shift
        if moving:
            world[:, :, :2] = world[:, :, :2] + dt * wvel
    fe.world = world
    res = dict(finish_tick=fe.finish_tick.copy(), min_clearance=fe.min_clearance.copy(), failures_per_tick=fails, final_status=status,
               waypoint_index=fe.k.copy(), converged_per_tick=both_ok, active_rows_per_tick=active_rows, yref_writes=fe.yref_writes)
    if not quiet:
        ft, mc = res["finish_tick"], res["min_clearance"]
        fin = ft >= 0
        print("seeds %d .. %d, %d ticks, %s" % (seed, seed + B - 1, ticks, ("moving world (drift %.3g / %.3g m/s), %s" % (
            scenario.PF_DRIFT_ALONG, scenario.PF_DRIFT_ACROSS, "predicted per stage" if predict else "held still inside the horizon"))
            if moving else "world at rest"))
        print("finished %d of %d%s" % (fin.sum(), B, ", at ticks %d .. %d" % (ft[fin].min(), ft[fin].max()) if fin.any() else ""))
        print("finish ticks %s" % ft.tolist())
        print("smallest clearance %.4f m (median %.4f); per mission %s" % (mc.min(), np.median(mc), np.round(mc, 4).tolist()))
        print("failed solves %d over all ticks (%d ticks with at least one); final status %s" % (fails.sum(), (fails > 0).sum(), status.tolist()))
        print("not finished: seeds %s, waypoint index %s" % ((seed + np.nonzero(~fin)[0]).tolist(), fe.k[~fin].tolist()))
        if parity_starts:
            print("converged per tick: min %.3f; instance-ticks with an obstacle row at its bound: %d (per tick %s)"
                  % (both_ok.min(), active_rows.sum(), active_rows.tolist()))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ticks", type=int, default=560)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--moving", action="store_true")
    ap.add_argument("--no-predict", action="store_true", help="the moving world held still inside the horizon (option \"pf_predict\" 0)")
    ap.add_argument("--drift-along", type=float, default=None)
    ap.add_argument("--drift-across", type=float, default=None)
    ap.add_argument("--parity-starts", action="store_true", help="the starts of the parity test instead of the generator's")
    a = ap.parse_args()
    drift = None
    if a.drift_along is not None or a.drift_across is not None:
        drift = (scenario.PF_DRIFT_ALONG if a.drift_along is None else a.drift_along,
                 scenario.PF_DRIFT_ACROSS if a.drift_across is None else a.drift_across)
    run(a.batch, a.ticks, seed=a.seed, moving=a.moving, predict=not a.no_predict, threads=a.threads, drift=drift,
        parity_starts=a.parity_starts)
