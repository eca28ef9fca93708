#!/usr/bin/env python3
"""What a closed loop against moving obstacles costs per tick, three ways (needs an MI355X):

  rewind   today's loop: p written once, never updated - the world starts again from tick 0 every tick (it solves OTHER problems than
           the two below from tick 1 on: printed for the record, not as a bound)
  tracks   option "obstacle_tracks": p derived on the device from the tracks, the world stepped by the hand-over
  host     the host rebuilds p with scenario.predict_tracks and pushes it with set_all("p") every tick (the same problems as `tracks`,
           bit for bit: tests/test_gpu_obstacle_tracks.py)

Median over --ticks timed ticks after --warmup warm-up ticks (a host clock around solve_async + advance + sync; `host` includes its numpy
rebuild and the upload), `--runs` alternating runs, one JSON line each, plus the bytes usv_obstacle_predict writes per tick.

    python tools/obstacle_tracks_probe.py --model usv_model_pf_ca --horizon 80 --obstacles 20 --batch 8192
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

MODES = ("rewind", "tracks", "host")


def run(mode, name, N, K, B, ticks, warmup, seed=1234, sigma=1e-3):
    wl = scenario.make_bench_batch(name, N, K, B, seed=seed, moving=True)
    ocp = usv_models.make_ocp(name, N * scenario.BENCH_DT, N, K)
    ocp.solver_options.sim_method_num_steps = scenario.BENCH_SIM_STEPS[name]
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, wl)
    s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
    if mode == "tracks":
        scenario.load_tracks(s, wl)
    pos, vel = wl["obs_pos"].copy(), wl["obs_vel"]
    times = []
    total0 = 0
    for t in range(warmup + ticks):
        if t == warmup:
            s.sync()
            total0 = s.unconverged_total()
        t0 = time.perf_counter()
        if mode == "host":
            s.set_all("p", scenario.predict_tracks(pos, vel, N, s.dt))
            pos = pos + s.dt * vel
        s.solve_async()
        s.advance(sigma, seed=t)
        s.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    timed = times[warmup:]
    unconv = s.unconverged_total() - total0
    out = dict(mode=mode, model=name, N=N, K=K, batch=B, ticks=ticks, warmup=warmup,
               tick_ms_median=statistics.median(timed), tick_ms_min=min(timed), tick_ms_max=max(timed),
               converged_solves_per_s=(B * ticks - unconv) / (sum(timed) * 1e-3), unconverged=int(unconv),
               predict_bytes_per_tick=B * (N + 1) * 2 * K * 8 if mode == "tracks" else 0,
               host_p_bytes_per_tick=B * (N + 1) * 2 * K * 8 if mode == "host" else 0)
    if mode == "tracks":
        out["clearance_min_worst"] = float(s.get("clearance_min", 0).min())
    s.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="usv_model_pf_ca")
    ap.add_argument("--horizon", type=int, default=80)
    ap.add_argument("--obstacles", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default=",".join(MODES))
    a = ap.parse_args()
    for r in range(a.runs):
        for mode in a.modes.split(","):
            line = run(mode, a.model, a.horizon, a.obstacles, a.batch, a.ticks, a.warmup)
            line["run"] = r
            print(json.dumps(line), flush=True)
