#!/usr/bin/env python3
"""A scenario sweep through the two-layer control stack the reference deploys (guidance.Cascade): B LiDAR scenarios of
scenario.make_ca_missions, each flown by the guidance NMPC (usv_model_guidance_ca1, 20 Hz) above the low-level NMPC (usv_model_low_level,
100 Hz) on a 3-DOF vessel - every tick on the device, no host array in the loop.  Prints how many missions finish, at which guidance
ticks, and the smallest clearance kept; tools/cascade_oracle.py is the same loop on the CPU.  --log-every n keeps every n-th low-level
tick's state, thrusts, set-points and status in the cascade's log on the device and prints the span of the logged track for a few
instances; --cost tracks the realised cost of both layers and prints its mean.

    python examples/cascade_sweep.py --batch 4096 --ticks 900 --log-every 25 --cost
"""
import argparse
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the solver library: one HIP runtime for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_collisionavoidance_amd import BatchOcpSolver, scenario, usv_models  # noqa: E402
from mpc_collisionavoidance_amd.guidance import Cascade, GuidanceFrontEnd  # noqa: E402


def run(B, gticks, L=6, seed=0, N=100, K=8, dt=0.05, ll_N=100, ratio=5, sigma=0.0, log_every=0, cost=False):
    m = scenario.make_ca_missions(B, L, seed=seed)
    g = BatchOcpSolver(usv_models.make_ocp("usv_model_guidance_ca1", N * dt, N, K), B)
    fe = GuidanceFrontEnd(g)
    ll = BatchOcpSolver(usv_models.make_ocp("usv_model_low_level", ll_N * dt / ratio, ll_N), B)
    fe.reset(m["waypoints"], m["pose"][:, 2])
    fe.set_world(m["world"])
    cas = Cascade(fe, ll, ratio=ratio)
    cas.reset(m["pose"], np.column_stack([m["vel"], np.zeros(B)]))
    if log_every > 0:                                            # (one record per log_every ticks; nothing below waits for it)
        cas.start_log((gticks * ratio + log_every - 1) // log_every, every=log_every)
    if cost:
        cas.track_cost()
    t0 = time.perf_counter()
    for t in range(gticks * ratio):
        cas.tick(sigma, t)
    st = cas.state()                                             # (waits for the stream)
    wall = time.perf_counter() - t0
    ms = fe.mission_state()
    out = dict(finish_tick=ms["finish_tick"], min_clearance=ms["min_clearance"], state=st["state"], err_sums=st["err_sums"],
               ms_per_low_level_tick=1e3 * wall / (gticks * ratio))
    if log_every > 0:
        out["log"], out["log_info"] = cas.read_log(instances=(0, min(B, 4))), cas.log_info()
    if cost:
        out["cost"] = cas.tracked_cost()
    cas.close(); ll.close(); g.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=900, help="guidance ticks (x ratio low-level ticks)")
    ap.add_argument("--obstacles", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sigma", type=float, default=0.0, help="disturbance on (u, v, r) per low-level tick")
    ap.add_argument("--log-every", type=int, default=0, metavar="n", help="log every n-th low-level tick on the device (0: no log)")
    ap.add_argument("--cost", action="store_true", help="track the realised cost of both layers on the device")
    a = ap.parse_args()
    r = run(a.batch, a.ticks, L=a.obstacles, seed=a.seed, sigma=a.sigma, log_every=a.log_every, cost=a.cost)
    fin = r["finish_tick"] >= 0
    print("finished %d of %d%s" % (fin.sum(), a.batch, ", at guidance ticks %d .. %d" % (r["finish_tick"][fin].min(), r["finish_tick"][fin].max())
                                   if fin.any() else ""))
    print("smallest min_clearance %.4f m (median %.4f)" % (r["min_clearance"].min(), np.median(r["min_clearance"])))
    print("mean |e_u| %.4f m/s, mean |e_psi| %.4f rad per low-level tick" % (r["err_sums"][:, 0].mean() / (a.ticks * 5), r["err_sums"][:, 1].mean() / (a.ticks * 5)))
    print("%.3f ms per low-level tick (%d instances)" % (r["ms_per_low_level_tick"], a.batch))
    if a.log_every > 0:
        lg, info = r["log"], r["log_info"]
        print("log: %d records of %d ticks (%d missed), every %d-th tick" % (info["records"], info["ticks"], info["missed"], a.log_every))
        for b in range(lg["state"].shape[0]):
            x, y = lg["state"][b, :, 0], lg["state"][b, :, 1]
            print("  instance %d: nedx %.2f .. %.2f m, nedy %.2f .. %.2f m over ticks %d .. %d; largest |thrust| %.2f; low-level failures %d" % (
                b, x.min(), x.max(), y.min(), y.max(), lg["tick"][0], lg["tick"][-1], np.abs(lg["thrust"][b]).max(), (lg["ll_status"][b] != 0).sum()))
    if a.cost:
        for layer in ("guidance", "low_level"):
            total, count = r["cost"][layer]
            print("realised cost, %s: mean %.5g per instance over %d solves (%.5g per solve)" % (layer, total.mean(), count, total.mean() / max(count, 1)))
