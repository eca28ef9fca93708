#!/usr/bin/env python3
"""What a closed-loop tick of the guidance front end (usv_model_guidance_ca1, N = 100, K = 8, the scenarios of scenario.make_ca_missions)
costs, three ways (needs an MI355X):

  hostfed   sense(pose, world) -> prepare(vel, pose) -> solve -> publish -> x1 = get("x", 1) -> numpy clearance: the loop of
            examples/scenario_sweep.py as it stands without --resident (five synchronisations and the world list through the host per tick)
  resident  prepare() -> solve_async -> publish(fetch=False) -> advance: the device-resident loop over a world at rest
  moving    the same over a moving world that is predicted: prepare() writes p / lh of every stage
  held      the moving world held still inside the horizon (predict = 0): stage 0 only

With --fleet S the batch is cut into scenes of S vessels that are each other's moving obstacles (GuidanceFrontEnd.set_fleet; vessel a of a
scene starts 2 a metres to the side), the world of every resident mode moves, and two more modes exist: `fleet` is `moving` with the fleet
on - prepare() gathers the scene-mates on the device ahead of usv_guidance_tick -, and `fleethost` is the loop a handle without the fleet
needs for the same scenes: synchronise, read x0 and the world back, rebuild the S - 1 trailing entries and velocities in numpy
(scenario.ca_fleet_world), upload, then the same four calls.  tick_net_of_qp_ms_median is the tick without the QP launch.  The JSON lines
also go to --out (default with --fleet: profiles/guidance_fleet_probe.txt).  --plans switches exchanged plans on in mode `fleet`
(set_fleet(plans=True): one more kernel behind the tick, csrc/fleet_plan.hpp); the mode `planhost` is the loop a handle without them needs:
synchronise, read x, status and the mission state back, prepare, read p back, rebuild it in numpy (scenario.fleet_plan_stages), upload it.

Per run one JSON line: the median tick (a host clock around the loop's body, ending in a synchronisation for the resident modes), and for the
resident modes the HIP-event time of the prepare's kernel (usv_guidance_tick: events on the solver's stream either side of it), the bytes a
predicted tick streams divided by that time, usvmpc_pipeline_stats, and how many missions kept their clearance.  --runs alternating runs.

--root DIR imports the package from another checkout (mode hostfed only needs calls every revision has): that is how the record's
host-fed figures were taken at the commit before the resident mode existed.

    python tools/guidance_mission_probe.py --batch 8192
    python tools/guidance_mission_probe.py --batch 65536 --modes resident,moving,held
    python tools/guidance_mission_probe.py --batch 65536 --fleet 4 --entries 4 --modes moving,fleet,fleethost
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def missions(B, L, seed):
    """scenario.make_ca_missions, restated so that --root may name a revision that has no such generator (the same draws)"""
    rng = np.random.default_rng(seed)
    y = -1.0 + (np.arange(L)[None, :] + rng.uniform(0.2, 0.8, (B, L))) * (25.0 / L)
    x = 4.0 + rng.uniform(-1.5, 1.5, (B, L))
    r = rng.uniform(0.3, 0.8, (B, L))
    world = np.stack([x, y, r], axis=2)
    pose = np.column_stack([4.0 + rng.uniform(-1, 1, B), np.full(B, -5.0), np.full(B, np.pi / 2) + rng.uniform(-0.3, 0.3, B)])
    rv = np.random.default_rng([seed, 1])
    wvel = np.stack([rv.uniform(-0.3, 0.3, (B, L)), np.zeros((B, L))], axis=2)
    return dict(waypoints=np.array([[4.0, -5.0], [4.0, 25.0], [10.0, 30.0]]), pose=pose, vel=np.column_stack([np.full(B, 0.7), np.zeros(B)]),
                world=world, world_vel=wvel)


def run(mode, B, ticks, warmup, N=100, K=8, L=5, seed=0, fleet=0, radius=0.5, plans=False):
    import torch
    from mpc_collisionavoidance_amd import BatchOcpSolver, scenario, usv_models
    from mpc_collisionavoidance_amd.guidance import GuidanceFrontEnd
    dt = 0.05
    m = missions(B, L, seed)
    s = BatchOcpSolver(usv_models.make_ocp("usv_model_guidance_ca1", N * dt, N, K), B)
    fe = GuidanceFrontEnd(s)
    world, pose, vel = m["world"], m["pose"], m["vel"]
    fe.reset(m["waypoints"], pose[:, 2])
    times, tick_ms = [], []
    out = dict(mode=mode, batch=B, N=N, K=K, L=L, ticks=ticks, warmup=warmup, fleet=fleet, plans=bool(plans and mode == "fleet"))
    if mode in ("fleet", "fleethost", "planhost") and fleet < 2:
        raise SystemExit("modes fleet and fleethost need --fleet S with S >= 2")
    if mode == "hostfed":
        min_clear = np.full(B, np.inf)
        for t in range(warmup + ticks):
            t0 = time.perf_counter()
            fe.sense(pose, world, max_radius=100.0)
            fe.prepare(vel, pose)
            s.solve()
            fe.publish()
            x1 = s.get("x", 1)
            vel, pose = x1[:, 0:2].copy(), x1[:, 5:8].copy()
            d = np.sqrt((pose[:, None, 0] - world[:, :, 0]) ** 2 + (pose[:, None, 1] - world[:, :, 1]) ** 2) - (world[:, :, 2] + 0.5)
            min_clear = np.minimum(min_clear, d.min(axis=1))
            times.append((time.perf_counter() - t0) * 1e3)
    else:
        x0 = np.zeros((B, 8))
        x0[:, 0:2], x0[:, 5:8] = vel, pose
        if fleet:
            x0[:, 5] += 2.0 * (np.arange(B) % fleet)
        s.set("x0", 0, x0)
        if mode == "fleethost":            # the same list, the trailing S - 1 entries the host's to fill
            fe.set_world(np.concatenate([world, np.tile([1000.0, 1000.0, 0.0], (B, fleet - 1, 1))], axis=1), max_radius=100.0,
                         vel=np.concatenate([m["world_vel"], np.zeros((B, fleet - 1, 2))], axis=1))
        else:
            fe.set_world(world, max_radius=100.0, vel=m["world_vel"] if mode in ("moving", "held", "fleet", "planhost") or fleet else None,
                         predict=mode != "held")
        if mode == "fleet" and plans:
            fe.set_fleet(fleet, radius, plans=True)
        elif mode in ("fleet", "planhost"):
            fe.set_fleet(fleet, radius)
        s.sync()
        for t in range(warmup + ticks):
            t0 = time.perf_counter()
            if mode == "fleethost":
                xr = s.get("x0", 0)         # (synchronises)
                w, v = fe.world()
                w[:, L:], v[:, L:], _ = scenario.ca_fleet_world(xr, fleet, radius)
                fe.set_world(w, max_radius=100.0, vel=v)
            if mode == "planhost":          # what a handle without exchanged plans needs: x, status and the mission state back, p back and up
                xs, status, before = s.get_all("x"), s.get_int("status"), fe.mission_state()["finish_tick"]
            fe.prepare()
            if mode == "planhost" and t >= 1:
                p, fin = s.get_all("p"), fe.mission_state()["finish_tick"]
                w = fe.world()[0]
                hit = np.abs(p[:, 0].reshape(B, K, 1, 2) - w[:, None, :, :2]).max(axis=3) <= 1e-4
                chosen = np.where(hit.any(axis=2) & (before < 0)[:, None], hit.argmax(axis=2), -1)
                s.set_all("p", scenario.fleet_plan_stages(p, xs, chosen, fleet, L, status, fin, pos=scenario.FLEET_PLAN_POS["usv_model_guidance_ca1"])[0])
            s.solve_async()
            fe.publish(fetch=False)
            s.advance(0.0, t)
            s.sync()
            times.append((time.perf_counter() - t0) * 1e3)
        lin, qp = s.kernel_ms(ticks)
        used, discarded = s.pipeline_stats()
        # the kernel's own time, in a pass of its own AFTER the timed ticks: events need the solver on a stream of torch's, and a handle on a
        # caller's stream no longer pipelines its lineariser (usvmpc_set_stream)
        stream = torch.cuda.Stream()
        s.set_stream(stream.cuda_stream)
        for t in range(0 if mode in ("fleethost", "planhost") else warmup + ticks):   # (fleethost: the kernels are those of `moving`)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fe.prepare()
            e1.record(stream)
            s.solve_async()
            fe.publish(fetch=False)
            s.advance(0.0, warmup + ticks + t)
            s.sync()
            tick_ms.append(e0.elapsed_time(e1))
        st = fe.mission_state()
        min_clear = st["min_clearance"]
        k_ms = statistics.median(tick_ms[warmup:]) if tick_ms else 0.0
        tick_ms = tick_ms or [0.0] * (warmup + 1)
        nbytes = B * ((N + 1) * 2 * K + N * K) * 8 if mode in ("moving", "fleet") else 0
        out.update(guidance_tick_ms_median=k_ms, guidance_tick_ms_min=min(tick_ms[warmup:]), streamed_bytes=nbytes,
                   stream_TB_per_s=(nbytes / (k_ms * 1e-3) / 1e12) if nbytes and k_ms else 0.0, pipelined_linearisations_used=int(used),
                   pipelined_linearisations_discarded=int(discarded))
    timed = times[warmup:]
    if mode == "hostfed":
        lin, qp = s.kernel_ms(ticks)
    out.update(tick_ms_median=statistics.median(timed), tick_ms_min=min(timed), tick_ms_max=max(timed), linearize_ms_median=float(np.median(lin)),
               qp_ms_median=float(np.median(qp)), tick_net_of_qp_ms_median=statistics.median(timed) - float(np.median(qp)), failed_last_tick=int(s.fail_counts(1)[0]),
               missions_clear_of_keepout=int((min_clear > 0.0).sum()), min_clearance_worst=float(min_clear.min()))
    s.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default="hostfed,resident,moving")
    ap.add_argument("--fleet", type=int, default=0, help="scenes of this many vessels (modes fleet, fleethost); the world of every resident mode moves")
    ap.add_argument("--plans", action="store_true", help="mode fleet: exchanged plans on (set_fleet(plans=True)); the mode planhost is the host loop they replace")
    ap.add_argument("--entries", type=int, default=5, help="world entries per instance (with --fleet: the fixed ones)")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is imported (default: this one)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well (the record: profiles/guidance_mission_probe.txt)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch  # noqa: F401  (before the solver library: one HIP runtime for both)
    if a.fleet and not a.out:
        a.out = os.path.join(HERE, "profiles", "guidance_fleet_probe.txt")
    if a.fleet:
        with open(a.out, "a") as f:
            f.write("# tools/guidance_mission_probe.py --batch %d --fleet %d --entries %d --modes %s --ticks %d --warmup %d --runs %d%s\n" % (
                a.batch, a.fleet, a.entries, a.modes, a.ticks, a.warmup, a.runs, " --plans" if a.plans else ""))
    for r in range(a.runs):
        for mode in a.modes.split(","):
            line = run(mode, a.batch, a.ticks, a.warmup, L=a.entries, fleet=a.fleet, plans=a.plans)
            line["run"] = r
            line["root"] = "this tree" if os.path.abspath(a.root) == HERE else "another checkout"
            print(json.dumps(line), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
