#!/usr/bin/env python3
"""What the objective value costs per closed-loop tick of a device-resident loop (needs an MI355X): the resident loop of
tools/pf_frontend_probe.py - prepare() -> solve_async -> publish(fetch=False) -> advance on the missions of scenario.make_pf_missions
(usv_model_pf_ca, N = 40, 5 RK4 steps; --K obstacle rows) - in four modes:

  none    no cost call
  eval    eval_cost() behind every solve_async (kernel usv_cost_eval; the results stay on the device)
  track   track_cost(True) once: every advance first enqueues usv_cost_track
  both    eval and track
  host    what the two replace: the host reads x, u and yref back every tick (get_all: a synchronisation and 10 KB per instance) and
          evaluates the objective in numpy (vectorised - the fastest the host can do, not the operation-by-operation restatement of the tests)

Median over --ticks timed ticks after --warmup warm-up ticks (a host clock around the tick and a final sync), `--runs` alternating runs, one
JSON line each, with the QP launch's kernel time of the same ticks (HIP events) and the tick net of it.

    python tools/cost_probe.py --batch 65536 --K 10
    rocprofv3 --kernel-trace --stats -- python tools/cost_probe.py --batch 65536 --K 10 --modes both --runs 1 --ticks 4 --warmup 1
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

MODES = ("none", "eval", "track", "host")   # and "both"
_missions = {}


def host_cost(ocp, dt, x, u, yref, yref_e):
    """the objective of a handle with hard obstacle rows on the host, vectorised: [B]"""
    co = ocp.cost
    V = np.concatenate([np.asarray(co.Vu, dtype=float), np.asarray(co.Vx, dtype=float)], axis=1)
    r = np.concatenate([u, x[:, :-1]], axis=2) @ V.T - yref
    stage = 0.5 * dt * np.einsum("bki,ij,bkj->b", r, np.asarray(co.W, dtype=float), r)
    re = x[:, -1] @ np.asarray(co.Vx_e, dtype=float).T - yref_e
    return stage + 0.5 * np.einsum("bi,ij,bj->b", re, np.asarray(co.W_e, dtype=float), re)


def run(mode, B, ticks, warmup, K, seed=0):
    cfg = scenario.PF_MISSION_OCP
    N, dt = cfg["N"], cfg["dt"]
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
    if mode in ("track", "both"):
        s.track_cost(True)
    s.sync()
    times, last = [], None
    for t in range(warmup + ticks):
        t0 = time.perf_counter()
        fe.prepare()
        s.solve_async()
        if mode in ("eval", "both"):
            s.eval_cost()
        elif mode == "host":
            last = host_cost(ocp, s.dt, s.get_all("x"), s.get_all("u"), s.get_all("yref"), s.get("yref", N))
        fe.publish(fetch=False)
        s.advance()
        s.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    timed = times[warmup:]
    _, qp = s.kernel_ms(ticks)
    if mode in ("eval", "both"):
        last = s.get_cost()          # (after the advance: the same iterate, evaluated once more)
    out = dict(mode=mode, batch=B, N=N, K=K, ticks=ticks, warmup=warmup, tick_ms_median=statistics.median(timed), tick_ms_min=min(timed),
               tick_ms_max=max(timed), qp_ms_median=float(np.median(qp)), net_ms_median=statistics.median(timed) - float(np.median(qp)),
               cost_median=None if last is None else float(np.median(last)),
               tracked_median=float(np.median(s.tracked_cost()[0])) if mode in ("track", "both") else None,
               eval_read_bytes=B * ((N + 1) * 14 + N * 2 + N * 16 + 14) * 8, eval_written_bytes=B * (N + 1 + 4) * 8,
               failed_last_tick=int(s.fail_counts(1)[0]), device_bytes=s.device_bytes())
    s.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--K", type=int, default=scenario.PF_MISSION_OCP["K"])
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default=",".join(MODES))
    a = ap.parse_args()
    for r in range(a.runs):
        for mode in a.modes.split(","):
            line = run(mode, a.batch, a.ticks, a.warmup, a.K)
            line["run"] = r
            print(json.dumps(line), flush=True)
