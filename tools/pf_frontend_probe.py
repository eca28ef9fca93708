#!/usr/bin/env python3
"""What the path-following front end of usv_model_pf_ca costs per closed-loop tick, three ways (needs an MI355X), on the missions of
scenario.make_pf_missions (N = 40, K = 4, 5 RK4 steps):

  plain     solve_async + advance on the instances' first-tick inputs: no front end after the first prepare (at 16 384 instances and more the
            pipelined lineariser runs: nothing invalidates it)
  resident  prepare() -> solve_async -> publish(fetch=False) -> advance: the device-resident front end (a prepare counts as a caller write
            of yref, so the lineariser runs inside the solve)
  hostfed   x0 read back, prepare(vel, pose) from it, solve_async, publish(fetch=False), advance: the host-fed front end

Median over --ticks timed ticks after --warmup warm-up ticks (a host clock around the tick and a final sync), `--runs` alternating runs, one
JSON line each, with the lineariser's and the QP launch's kernel times of the same ticks (HIP events) and the bytes a full yref rewrite
streams.

    python tools/pf_frontend_probe.py --batch 65536
    rocprofv3 --kernel-trace --stats -- python tools/pf_frontend_probe.py --batch 65536 --modes resident --runs 1 --ticks 4 --warmup 1
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (before the solver library: one HIP runtime for both)
from mpc_collisionavoidance_amd import BatchOcpSolver, scenario, usv_models  # noqa: E402
from mpc_collisionavoidance_amd.guidance import PathFollowingFrontEnd  # noqa: E402

MODES = ("plain", "resident", "hostfed")
_missions = {}


def run(mode, B, ticks, warmup, seed=0):
    cfg = scenario.PF_MISSION_OCP
    N, K, dt = cfg["N"], cfg["K"], cfg["dt"]
    if (B, seed) not in _missions:
        _missions[(B, seed)] = scenario.make_pf_missions(B, seed)
    m = _missions[(B, seed)]
    ocp = usv_models.make_ocp("usv_model_pf_ca", N * dt, N, K)
    ocp.solver_options.sim_method_num_steps = cfg["sim_steps"]
    s = BatchOcpSolver(ocp, B)
    fe = PathFollowingFrontEnd(s)
    s.set("x0", 0, m["x0"])
    s.set_all("x", np.tile(m["x0"][:, None, :], (1, N + 1, 1)))
    s.set_all("u", np.zeros((B, N, 2)))
    fe.reset(m["waypoints"])
    fe.set_world(m["world"], max_radius=cfg["max_radius"], margin=cfg["margin"])
    if mode == "plain":
        fe.prepare()                      # the first tick's inputs, once
    s.sync()
    times = []
    for t in range(warmup + ticks):
        t0 = time.perf_counter()
        if mode == "resident":
            fe.prepare()
        elif mode == "hostfed":
            x0 = s.get("x0", 0)
            fe.prepare(x0[:, 3:6], x0[:, [10, 11, 0]])
        s.solve_async()
        if mode != "plain":
            fe.publish(fetch=False)
        s.advance()
        s.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    timed = times[warmup:]
    lin, qp = s.kernel_ms(ticks)
    used, discarded = s.pipeline_stats()
    st = fe.state()
    out = dict(mode=mode, batch=B, N=N, K=K, ticks=ticks, warmup=warmup, tick_ms_median=statistics.median(timed), tick_ms_min=min(timed),
               tick_ms_max=max(timed), linearize_ms_median=float(np.median(lin)), qp_ms_median=float(np.median(qp)),
               pipelined_linearisations_used=int(used), yref_writes=st["yref_writes"], yref_full_rewrite_bytes=B * (N * 16 + 14) * 8,
               failed_last_tick=int(s.fail_counts(1)[0]))
    s.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default=",".join(MODES))
    a = ap.parse_args()
    for r in range(a.runs):
        for mode in a.modes.split(","):
            line = run(mode, a.batch, a.ticks, a.warmup)
            line["run"] = r
            print(json.dumps(line), flush=True)
