#!/usr/bin/env python3
"""Vessel encounters with the model the reference deploys (usv_model_guidance_ca1: nmpc_guidance_ca1.cpp behind obstacle_sim_node.py, N = 100,
K = 8, soft obstacle rows), the whole tick on the device: scenes of S vessels, each running this NMPC behind the guidance front end and each
the others' moving obstacle (scenario.make_ca_encounters: side by side, crossing or head-on).  A tick is

    prepare() -> solve_async() -> publish(fetch=False) -> advance()

with no host array and no stream synchronisation in it: ahead of the front end's own kernel, prepare() gathers every vessel's scene-mates -
position, hull radius, velocity (u, v) turned by psi, from the states the plant left in x0 - into the fleet entries of its world list
(guidance.GuidanceFrontEnd.set_fleet; csrc/ca_fleet_world.hpp), and the front end then senses them, selects the nearest K and writes the
predicted obstacle set of every stage as it does for any moving world; the lineariser keeps running a tick ahead.  The plant is the
controller's prediction x_1; with --plant-steps K an RK4 integrator of its own (advance_sim).

    python examples/ca_encounter_sweep.py --scenes 4096 --scene-size 2 --ticks 300 --kind crossing [--plant-steps 10] [--no-predict] [--plans]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (before the solver library: one HIP runtime for both)
from mpc_collisionavoidance_amd import AcadosSim, BatchOcpSolver, BatchSimSolver, scenario, usv_models  # noqa: E402
from mpc_collisionavoidance_amd.guidance import GuidanceFrontEnd  # noqa: E402

RING = 64   # solves whose failure counts the library keeps


def run(scenes, S, ticks, kind="crossing", N=None, K=None, seed=0, radius=0.5, plant_steps=None, predict=True, quiet=False, plans=False):
    cfg = scenario.CA_ENC_OCP
    N, K, dt = N or cfg["N"], K or cfg["K"], cfg["dt"]
    B = scenes * S
    m = scenario.make_ca_encounters(scenes, S, seed, kind)
    ocp = usv_models.make_ocp("usv_model_guidance_ca1", N * dt, N, K)
    s = BatchOcpSolver(ocp, B)
    plant = None
    if plant_steps:
        sim = AcadosSim()
        sim.model = ocp.model
        sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = dt, int(plant_steps), False
        plant = BatchSimSolver(sim, B)
    fe = GuidanceFrontEnd(s)
    s.set("x0", 0, m["x0"])
    s.set_all("x", np.tile(m["x0"][:, None, :], (1, N + 1, 1)))        # acados' own initial iterate: x_k = x0, u = 0
    s.set_all("u", np.zeros((B, N, 1)))
    fe.reset(m["waypoints"], m["pose"][:, 2])
    fe.set_world(m["world"], max_radius=cfg["max_radius"])
    fe.set_fleet(S, radius, plans=plans)      # plans: a scene-mate's slot follows the mate's own solved path (csrc/fleet_plan.hpp)
    if not predict:                                                     # (the fleet is on: these are the fixed entries, and the choice holds)
        fe.set_world(m["world"], max_radius=cfg["max_radius"], predict=False)
    fails = np.zeros(ticks, dtype=int)
    s.sync()
    t0 = time.perf_counter()
    for i in range(ticks):
        fe.prepare()
        s.solve_async()
        fe.publish(fetch=False)
        if plant is None:
            s.advance()
        else:
            s.advance_sim(plant)
        if (i + 1) % RING == 0 or i == ticks - 1:                         # the device counts the failed solves: fetched once per RING ticks
            n = (i % RING) + 1
            fails[i + 1 - n:i + 1] = s.fail_counts(n)
    s.sync()
    el = time.perf_counter() - t0
    st, fl, pl = fe.mission_state(), fe.fleet_state(), fe.fleet_plan_state()
    res = dict(ticks_per_s=ticks / el, finish_tick=st["finish_tick"], min_clearance=st["min_clearance"], min_separation=fl["min_separation"],
               separation_tick=fl["separation_tick"], waypoint_index=st["wp_index"], failures_per_tick=fails, final_status=s.get_int("status"),
               final_pose=s.get("x0", 0)[:, 5:8].copy(), plan_fed=pl["plan_fed"], plan_launches=pl["plan_launches"])
    if not quiet:
        fin = st["finish_tick"] >= 0
        ms, mc = res["min_separation"], res["min_clearance"]
        print("%s: %d scenes of %d x %d ticks in %.2f s (%.1f ticks/s, %.0f vessel-ticks/s)" % (kind, scenes, S, ticks, el, ticks / el, B * ticks / el))
        if fin.any():
            print("finished: %d of %d, at ticks %d .. %d" % (fin.sum(), B, st["finish_tick"][fin].min(), st["finish_tick"][fin].max()))
        else:
            print("finished: 0 of %d" % B)
        print("smallest separation between two vessels of a scene: %.4f m (median %.4f m), met at tick %d; hulls of %.2f m touch at %.2f m"
              % (ms.min(), np.median(ms), res["separation_tick"][ms.argmin()], radius, 2 * radius))
        print("minimum clearance to the keep-out circle (R + 0.5 m): worst %.4f m, median %.4f m" % (mc.min(), np.median(mc)))
        if plans:
            print("exchanged plans: %d launches of the plan kernel, %d plan-fed (vessel, slot) pairs" % (pl["plan_launches"], pl["plan_fed"]))
        print("failed solves: %d over all ticks (%d ticks with at least one)" % (fails.sum(), (fails > 0).sum()))
    s.close()
    if plant is not None:
        plant.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=512)
    ap.add_argument("--scene-size", type=int, default=2)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--kind", default="crossing", choices=scenario.CA_ENC_KINDS)
    ap.add_argument("--horizon", type=int, default=None, help="default: the reference's N = 100 (Tf = 5 s)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--radius", type=float, default=0.5, help="hull radius of a vessel as its scene-mates see it")
    ap.add_argument("--plant-steps", type=int, default=None,
                    help="integrate the plant in this many RK4 steps per tick (default: the plant is the controller's prediction x_1)")
    ap.add_argument("--no-predict", action="store_true", help="the scene is held still inside the horizon (set_world(..., predict=False))")
    ap.add_argument("--plans", action="store_true", help="scene-mates are predicted along their own solved paths, not along straight lines")
    a = ap.parse_args()
    run(a.scenes, a.scene_size, a.ticks, kind=a.kind, N=a.horizon, seed=a.seed, radius=a.radius, plant_steps=a.plant_steps,
        predict=not a.no_predict, plans=a.plans)
