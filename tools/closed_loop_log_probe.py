#!/usr/bin/env python3
"""What keeping the closed-loop trajectory costs per tick of a device-resident path-following mission (needs an MI355X): the resident loop
of tools/pf_frontend_probe.py - prepare() -> solve_async -> publish(fetch=False) -> advance, scenario.make_pf_missions, N = 40, K = 4, 5 RK4
steps - in four modes:

  off       no log
  pose      start_log of (psi, nedx, nedy) = states 0, 10, 11, every tick                (what examples/pf_mission_sweep.py --log-every 1 keeps)
  all       start_log of all 14 states + u + status, every tick, with the three error channels of scripts/usv_pf_ca/main.py
  readback  no log; the host reads x0 and u[:, 0] back every tick, just before the hand-over - what the log replaces

Median over --ticks timed ticks after --warmup warm-up ticks (a host clock around the tick and a final sync), `--runs` alternating runs, one
JSON line each.  tick_net_ms_median is the median of (tick - QP launch) per tick, the QP launch's time from HIP events of the same ticks.

With --moving the world moves (scenario.make_pf_missions(moving=True)), so that a kernel trace also holds usv_pf_world_step, a launch-bound
kernel to compare usv_log_record with.

    python tools/closed_loop_log_probe.py --batch 65536
    rocprofv3 --kernel-trace --stats -- python tools/closed_loop_log_probe.py --batch 65536 --moving --modes all --runs 1 --ticks 4 --warmup 1
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

MODES = ("off", "pose", "all", "readback")
ERRORS = [(0, 9), (3, 0.7), (6, 0.0)]
_missions = {}


def run(mode, B, ticks, warmup, seed=0, moving=False):
    cfg = scenario.PF_MISSION_OCP
    N, K, dt = cfg["N"], cfg["K"], cfg["dt"]
    if (B, seed) not in _missions:
        _missions[(B, seed)] = scenario.make_pf_missions(B, seed, moving=True)   # (every other field is the same with either value)
    m = _missions[(B, seed)]
    ocp = usv_models.make_ocp("usv_model_pf_ca", N * dt, N, K)
    ocp.solver_options.sim_method_num_steps = cfg["sim_steps"]
    s = BatchOcpSolver(ocp, B)
    fe = PathFollowingFrontEnd(s)
    s.set("x0", 0, m["x0"])
    s.set_all("x", np.tile(m["x0"][:, None, :], (1, N + 1, 1)))
    s.set_all("u", np.zeros((B, N, 2)))
    fe.reset(m["waypoints"])
    fe.set_world(m["world"], max_radius=cfg["max_radius"], margin=cfg["margin"], vel=m["world_vel"] if moving else None)
    base = s.device_bytes()
    if mode == "pose":
        s.start_log(warmup + ticks, states=[0, 10, 11], u=False, status=False)
    elif mode == "all":
        s.start_log(warmup + ticks, errors=ERRORS)
    log_bytes = s.device_bytes() - base
    s.sync()
    times = []
    for t in range(warmup + ticks):
        t0 = time.perf_counter()
        fe.prepare()
        s.solve_async()
        fe.publish(fetch=False)
        if mode == "readback":
            s.get("x0", 0), s.get("u", 0)
        s.advance()
        s.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    timed = np.array(times[warmup:])
    lin, qp = s.kernel_ms(ticks)
    info = s.log_info() if mode in ("pose", "all") else dict(records=0, missed=0)
    out = dict(mode=mode, batch=B, moving=bool(moving), N=N, K=K, ticks=ticks, warmup=warmup, tick_ms_median=statistics.median(timed.tolist()),
               tick_ms_min=float(timed.min()), tick_ms_max=float(timed.max()), qp_ms_median=float(np.median(qp)),
               linearize_ms_median=float(np.median(lin)), tick_net_ms_median=float(np.median(timed - qp)),
               log_bytes=int(log_bytes), record_bytes=int(log_bytes // (warmup + ticks)) if log_bytes else 0,
               records=info["records"], missed=info["missed"], failed_last_tick=int(s.fail_counts(1)[0]))
    s.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--moving", action="store_true", help="the world moves (every stage of p / lh per tick, usv_pf_world_step per hand-over)")
    a = ap.parse_args()
    for r in range(a.runs):
        for mode in a.modes.split(","):
            line = run(mode, a.batch, a.ticks, a.warmup, moving=a.moving)
            line["run"] = r
            print(json.dumps(line), flush=True)
