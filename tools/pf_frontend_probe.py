#!/usr/bin/env python3
"""What the path-following front end of usv_model_pf_ca costs per closed-loop tick, three ways (needs an MI355X), on the missions of
scenario.make_pf_missions (N = 40, K = 4, 5 RK4 steps):

  plain     solve_async + advance on the instances' first-tick inputs: no front end after the first prepare (at 16 384 instances and more the
            pipelined lineariser runs: nothing invalidates it)
  resident  prepare() -> solve_async -> publish(fetch=False) -> advance: the device-resident front end (a prepare counts as a caller write
            of yref, so the lineariser runs inside the solve)
  hostfed   x0 read back, prepare(vel, pose) from it, solve_async, publish(fetch=False), advance: the host-fed front end

With --moving the world of `resident` and `hostfed` moves (scenario.make_pf_missions(moving=True)): prepare writes p / lh of every stage and
advance steps the world; the extra mode `held` is `resident` with option "pf_predict" 0 (the world moves between ticks, stage 0 only) and `static` is `resident` over
a world at rest whatever --moving says, so that one invocation alternates the three.

With --fleet S the batch is cut into scenes of S vessels that are each other's moving obstacles (PathFollowingFrontEnd.set_fleet; every
vessel's route, start and four fixed obstacles are moved 4 a metres east for vessel a of a scene, so that scene-mates sail side by side),
the world of every mode moves, and two more modes exist: `fleet` is `resident` with the fleet on - prepare() gathers the scene-mates on the
device ahead of its own kernel -, and `fleethost` is the loop a handle without the fleet needs for the same scenes: synchronise, read x0 and
the world back, rebuild the S - 1 trailing entries and velocities in numpy (scenario.fleet_world), upload, then the same four calls.  The
JSON lines also go to --out (default profiles/pf_fleet_probe.txt).  --plans switches exchanged plans on in mode `fleet` (set_fleet(plans=True):
one more kernel behind the prepare, csrc/fleet_plan.hpp), and the mode `planhost` is the loop a handle without them needs: synchronise, read
x, status and the front-end state back, prepare, read p back, rebuild it in numpy (scenario.fleet_plan_stages), upload [B][N+1][2K].  --root
imports the package of another checkout (one whose library has no plans runs `fleet` without the switch).

Median over --ticks timed ticks after --warmup warm-up ticks (a host clock around the tick and a final sync), `--runs` alternating runs, one
JSON line each, with the lineariser's and the QP launch's kernel times of the same ticks (HIP events) and the bytes a full yref rewrite
streams.

    python tools/pf_frontend_probe.py --batch 65536
    python tools/pf_frontend_probe.py --batch 65536 --moving --modes static,resident,held
    python tools/pf_frontend_probe.py --batch 65536 --fleet 4 --modes resident,fleet,fleethost
    rocprofv3 --kernel-trace --stats -- python tools/pf_frontend_probe.py --batch 65536 --modes resident --runs 1 --ticks 4 --warmup 1
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv[:-1] else HERE   # (ahead of the imports below)
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (before the solver library: one HIP runtime for both)
from mpc_collisionavoidance_amd import BatchOcpSolver, scenario, usv_models  # noqa: E402
from mpc_collisionavoidance_amd.guidance import PathFollowingFrontEnd  # noqa: E402

MODES = ("plain", "resident", "hostfed")   # and "held", "static" (see above)
_missions = {}


def fleet_missions(m, S):
    """make_pf_missions' batch with vessel a of every scene moved 4 a metres east: route, start and fixed obstacles"""
    east = 4.0 * (np.arange(m["x0"].shape[0]) % S)
    out = {k: v.copy() for k, v in m.items()}
    out["waypoints"][:, :, 0] += east[:, None]
    out["world"][:, :, 0] += east[:, None]
    out["x0"][:, 10] += east
    return out


def run(mode, B, ticks, warmup, seed=0, moving=False, fleet=0, radius=0.5, plans=False):
    cfg = scenario.PF_MISSION_OCP
    N, K, dt = cfg["N"], cfg["K"], cfg["dt"]
    if (B, seed, fleet) not in _missions:
        m = scenario.make_pf_missions(B, seed, moving=True)   # (every other field is the same with either value)
        _missions[(B, seed, fleet)] = fleet_missions(m, fleet) if fleet else m
    m = _missions[(B, seed, fleet)]
    ocp = usv_models.make_ocp("usv_model_pf_ca", N * dt, N, K)
    ocp.solver_options.sim_method_num_steps = cfg["sim_steps"]
    s = BatchOcpSolver(ocp, B)
    fe = PathFollowingFrontEnd(s)
    s.set("x0", 0, m["x0"])
    s.set_all("x", np.tile(m["x0"][:, None, :], (1, N + 1, 1)))
    s.set_all("u", np.zeros((B, N, 2)))
    fe.reset(m["waypoints"])
    if mode == "held":
        s.set_option("pf_predict", 0)
    moves = mode == "held" or mode in ("fleet", "fleethost", "planhost") or (moving and mode in ("resident", "hostfed"))
    fe.set_world(m["world"], max_radius=cfg["max_radius"], margin=cfg["margin"], vel=m["world_vel"] if moves else None)
    n_fixed = m["world"].shape[1]
    if mode == "fleet" and plans:
        fe.set_fleet(fleet, radius, plans=True)
    elif mode in ("fleet", "planhost"):
        fe.set_fleet(fleet, radius)
    elif mode == "fleethost":             # the same list, the trailing S - 1 entries the host's to fill
        far = np.tile([1000.0, 1000.0, 0.0], (B, fleet - 1, 1))
        fe.set_world(np.concatenate([m["world"], far], axis=1), max_radius=cfg["max_radius"],
                     vel=np.concatenate([m["world_vel"], np.zeros((B, fleet - 1, 2))], axis=1))
    if mode == "plain":
        fe.prepare()                      # the first tick's inputs, once
    s.sync()
    times = []
    for t in range(warmup + ticks):
        t0 = time.perf_counter()
        if mode in ("resident", "held", "static", "fleet"):
            fe.prepare()
        elif mode == "fleethost":
            x0 = s.get("x0", 0)
            w, v = fe.world()
            w[:, n_fixed:], v[:, n_fixed:], _ = scenario.fleet_world(x0, fleet, radius)
            fe.set_world(w, max_radius=cfg["max_radius"], vel=v)
            fe.prepare()
        elif mode == "planhost":
            x, status = s.get_all("x"), s.get_int("status")          # (synchronises)
            fe.prepare()
            if t >= 1:
                p, fin = s.get_all("p"), fe.state()["finish_tick"]
                w = fe.world()[0]
                slots = p[:, 0].reshape(B, K, 2)
                hit = (slots[:, :, None, :] == w[:, None, :, :2]).all(axis=3)
                chosen = np.where(hit.any(axis=2) & (fin < 0)[:, None], hit.argmax(axis=2), -1)
                s.set_all("p", scenario.fleet_plan_stages(p, x, chosen, fleet, n_fixed, status, fin)[0])
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
               tick_ms_max=max(timed), tick_net_of_qp_ms_median=statistics.median(timed) - float(np.median(qp)), fleet=fleet, plans=bool(plans and mode == "fleet"),
               root="this tree" if ROOT == HERE else "another checkout",
               linearize_ms_median=float(np.median(lin)), qp_ms_median=float(np.median(qp)),
               pipelined_linearisations_used=int(used), yref_writes=st["yref_writes"], yref_full_rewrite_bytes=B * (N * 16 + 14) * 8,
               failed_last_tick=int(s.fail_counts(1)[0]), moving=bool(moves),
               p_lh_full_rewrite_bytes=B * ((N + 1) * 2 * K + N * K) * 8 if moves and mode != "held" else 0)
    s.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--moving", action="store_true", help="the world of the front-end modes moves (every stage of p / lh per tick)")
    ap.add_argument("--fleet", type=int, default=0, help="scenes of this many vessels (modes fleet, fleethost); the world of every mode moves")
    ap.add_argument("--out", default=None, help="with --fleet: where the JSON lines are also written (default profiles/pf_fleet_probe.txt)")
    ap.add_argument("--plans", action="store_true", help="mode fleet: exchanged plans on (set_fleet(plans=True))")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is imported (default: this one)")
    a = ap.parse_args()
    lines = []
    for r in range(a.runs):
        for mode in a.modes.split(","):
            line = run(mode, a.batch, a.ticks, a.warmup, moving=a.moving or a.fleet > 0, fleet=a.fleet, plans=a.plans)
            line["run"] = r
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    if a.fleet:
        with open(a.out or os.path.join(HERE, "profiles", "pf_fleet_probe.txt"), "a") as f:
            f.write("# tools/pf_frontend_probe.py --batch %d --fleet %d --modes %s --ticks %d --warmup %d --runs %d%s\n" % (
                a.batch, a.fleet, a.modes, a.ticks, a.warmup, a.runs, " --plans" if a.plans else ""))
            f.write("\n".join(lines) + "\n")
