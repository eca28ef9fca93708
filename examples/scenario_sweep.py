#!/usr/bin/env python3
"""A batched LiDAR-scenario sweep with the whole tick on the device: the ROS pipeline of the reference
(obstacle simulator -> NMPC node callbacks / waypoint manager -> acados_solve -> published set-points,
catkin_ws/src/simulation/scripts/obstacle_sim_node.py + catkin_ws/src/nmpc_ca/src/nmpc_guidance_ca1.cpp) run for B
random obstacle fields at once.  As in the reference's own main.py the plant is the model prediction: the next
pose / velocity are read from x_1 of the solution.  With --plant-steps K the plant is an integrator of its own instead
(BatchSimSolver: the same model over the same 0.05 s in K RK4 steps, from x_0 under u_0), i.e. a plant that differs from
the controller's one-step prediction by its discretisation error.

With --log-every n the device-resident loop also keeps its closed-loop trajectory (the reference's simX: scripts/usv_guidance_ca1/
main.py:147-148) without a host array in the tick: start_log() records (xned, yned, psi) of every n-th tick on the device and sums |e| and
e e of this model's tracking errors, the states ye and chie (scripts/usv_pf_ca/main.py prints the same statistics for its own); read once
at the end.

    python examples/scenario_sweep.py --batch 4096 --ticks 300 [--plant-steps 10] [--resident [--log-every 4]]
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


def make_worlds(B, L, rng):
    """scenario.make_ca_worlds: L obstacles per scenario along the first leg (4,-5) -> (4,25)."""
    return scenario.make_ca_worlds(B, L, rng)


ERRORS = (("ye", (2, 0.0)), ("chie", (3, 0.0)))   # the tracking errors of usv_model_guidance_ca1 are states: (state, constant)


def run(B=1024, ticks=600, N=100, K=8, L=5, seed=0, quiet=False, plant_steps=None, resident=False, moving=False, predict=True, log_every=None,
        cost=False):
    """resident=False: the host-fed loop (the ROS nodes' callbacks, arrays through the host every tick).  resident=True: the whole mission
    on the device - the world is uploaded once, a tick is prepare() -> solve_async -> publish(fetch=False) -> advance, and the host reads
    once at the end.  moving=True (resident only): the obstacles cross the first leg and the horizon sees where they will be (predict)."""
    dt = 0.05
    ocp = usv_models.make_ocp("usv_model_guidance_ca1", N * dt, N, K)
    s = BatchOcpSolver(ocp, B)
    plant = None
    if plant_steps:
        sim = AcadosSim()
        sim.model = ocp.model
        sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = dt, int(plant_steps), False
        plant = BatchSimSolver(sim, B)
    fe = GuidanceFrontEnd(s)
    m = scenario.make_ca_missions(B, L, seed, moving=moving)
    wps, world, pose, vel = m["waypoints"], m["world"], m["pose"], m["vel"]
    fe.reset(wps, pose[:, 2])
    if moving and not resident:
        raise Exception("a moving world needs the device-resident loop (resident=True)")
    if log_every and not resident:
        raise Exception("the log replaces the host arrays of the device-resident loop (resident=True); the host-fed loop has them anyway")
    if cost and not resident:
        raise Exception("the tracked cost replaces the read-backs of the device-resident loop (resident=True)")
    if resident:
        res = _run_resident(s, fe, plant, m, ticks, predict, log_every, cost)
    else:
        min_clear = np.full(B, np.inf)
        bad = np.zeros(B, dtype=bool)
        t0 = time.perf_counter()
        for i in range(ticks):
            fe.sense(pose, world, max_radius=100.0)      # obstacle_sim_node.simulate()
            fe.prepare(vel, pose)                        # obstaclesCallback + waypoint_manager + control() inputs
            st = s.solve()                               # acados_solve()
            out = fe.publish()                           # desired heading / r / speed
            bad |= (st != 0) & (out["active"] != 0)
            if plant is None:
                x1 = s.get("x", 1)
            else:
                plant.set("x", s.get("x", 0))
                plant.set("u", s.get("u", 0))
                plant.solve()
                x1 = plant.get("x")
            vel, pose = x1[:, 0:2].copy(), x1[:, 5:8].copy()
            d = np.sqrt((pose[:, None, 0] - world[:, :, 0]) ** 2 + (pose[:, None, 1] - world[:, :, 1]) ** 2) - (world[:, :, 2] + 0.5)
            min_clear = np.minimum(min_clear, d.min(axis=1))
        el = time.perf_counter() - t0
        k, _ = fe.state()
        res = dict(ticks_per_s=ticks / el, scenario_ticks_per_s=B * ticks / el, min_clearance=min_clear, solver_failures=bad,
                   waypoint_index=k, final_pose=pose)
    if not quiet:
        el = ticks / res["ticks_per_s"]
        min_clear, bad, k = res["min_clearance"], res["solver_failures"], res["waypoint_index"]
        print("%d scenarios x %d ticks in %.2f s (%.0f scenario-ticks/s)" % (B, ticks, el, B * ticks / el))
        print("minimum clearance to the keep-out circle (R + 0.5 m): worst %.3f m, 1st percentile %.3f m, median %.3f m"
              % (min_clear.min(), np.percentile(min_clear, 1), np.median(min_clear)))
        print("scenarios with a solver failure: %d; reached the second leg: %d" % (bad.sum(), (k >= 2).sum()))
        if cost:
            tc = res["tracked_cost"][res["finish_tick"] >= 0]
            if tc.size:
                print("realised closed-loop cost over %d hand-overs, finished missions: min %.4f, median %.4f, max %.4f"
                      % (res["tracked_count"], tc.min(), np.median(tc), tc.max()))
            else:
                print("realised closed-loop cost over %d hand-overs: no mission has finished" % res["tracked_count"])
        if log_every:
            print("logged %d records of (xned, yned, psi) per scenario, one every %d ticks; errors over %d ticks:"
                  % (len(res["log_tick"]), log_every, res["error_count"]))
            for c, (name, _) in enumerate(ERRORS):
                print("  %-5s mean absolute error %.6f, mean square error %.6f (means over the %d scenarios)"
                      % (name, res["mean_abs_error"][:, c].mean(), res["mean_sq_error"][:, c].mean(), B))
    s.close()
    if plant is not None:
        plant.close()
    return res


def _run_resident(s, fe, plant, m, ticks, predict, log_every=None, cost=False):
    """The device-resident loop.  min_clearance is the front end's: the minimum over the poses the ticks were PREPARED at (the start pose
    included, the pose after the last tick not), where the host-fed loop takes the poses after each tick.
    solver_failures: an instance's status after the last tick, missions that are over left out as in the host-fed loop; the ticks before
    are audited through the device-side failure counts (usvmpc_fail_counts: a ring of 64 solves, read once per 64 ticks and at the end) -
    a failure in an earlier tick, before any mission was over, marks EVERY instance, since the host does not know which one it was."""
    B = s.B
    x0 = np.zeros((B, 8))
    x0[:, 0:2], x0[:, 5:8] = m["vel"], m["pose"]
    s.set("x0", 0, x0)
    fe.set_world(m["world"], max_radius=100.0, vel=m.get("world_vel"), predict=predict)
    fails = []
    if log_every:
        s.start_log(-(-ticks // log_every), every=log_every, states=[5, 6, 7], u=False, status=False, errors=[c for _, c in ERRORS])
    if cost:
        s.track_cost(True)                           # the realised closed-loop cost: every hand-over adds c_0(x0, u_0) on the device
    t0 = time.perf_counter()
    for i in range(ticks):
        fe.prepare()                                 # sensor + callbacks + waypoint manager, from the solver's own x0
        s.solve_async()
        fe.publish(fetch=False)
        if plant is None:
            s.advance(0.0, i)
        else:
            s.advance_sim(plant, 0.0, i)
        if (i + 1) % 64 == 0 or i + 1 == ticks:
            fails.append(s.fail_counts((i % 64) + 1))
    s.sync()
    el = time.perf_counter() - t0
    st = fe.mission_state()
    fails = np.concatenate(fails) if fails else np.zeros(0, dtype=int)
    over = st["finish_tick"] >= 0
    bad = (s.get_int("status") != 0) & ~over
    audited = min(ticks - 1, int(st["finish_tick"][over].min())) if over.any() else ticks - 1
    if ticks and fails[:max(audited, 0)].any():
        bad[:] = True
    res = dict(ticks_per_s=ticks / el, scenario_ticks_per_s=B * ticks / el, min_clearance=st["min_clearance"], solver_failures=bad,
               waypoint_index=st["wp_index"], final_pose=s.get("x0", 0)[:, 5:8].copy(), finish_tick=st["finish_tick"], fail_counts=fails)
    if cost:
        res["tracked_cost"], res["tracked_count"] = s.tracked_cost()
    if log_every:
        log, err = s.read_log(), s.log_errors()
        # beside final_pose, in its order (xned, yned, psi): [B][records][3] and the tick of each record
        res.update(log_pose=log["x"].copy(), log_tick=log["tick"], error_count=err["count"],
                   mean_abs_error=err["sum_abs"] / max(err["count"], 1), mean_sq_error=err["sum_sq"] / max(err["count"], 1))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--horizon", type=int, default=100, help="the reference uses N = 100, Tf = 5 s; shorter horizons see the obstacles too late")
    ap.add_argument("--plant-steps", type=int, default=None,
                    help="integrate the plant in this many RK4 steps per tick (default: the plant is the controller's prediction x_1)")
    ap.add_argument("--resident", action="store_true", help="keep the whole mission on the device (no host array, no synchronisation per tick)")
    ap.add_argument("--moving", action="store_true", help="the obstacles cross the first leg at up to 0.3 m/s (device-resident loop)")
    ap.add_argument("--no-predict", action="store_true", help="with --moving: hold the world still inside the horizon")
    ap.add_argument("--log-every", type=int, default=None,
                    help="device-resident loop: keep (xned, yned, psi) of every n-th tick and the ye / chie error statistics on the device")
    ap.add_argument("--cost", action="store_true", help="device-resident loop: sum the realised closed-loop cost of every scenario on the device")
    a = ap.parse_args()
    run(a.batch, a.ticks, a.horizon, plant_steps=a.plant_steps, resident=a.resident or a.moving or bool(a.log_every), moving=a.moving,
        predict=not a.no_predict, log_every=a.log_every, cost=a.cost)
