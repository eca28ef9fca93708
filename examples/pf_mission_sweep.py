#!/usr/bin/env python3
"""Multi-leg path-following missions with the headline model, the whole tick on the device: the reference's path-following node
(catkin_ws/src/nmpc_ca/src/nmpc_pf.cpp: waypoint manager, x0 / reference assembly, published thrusts) around usv_model_pf_ca with hard
obstacle rows, for B random obstacle fields at once (scenario.make_pf_missions: two legs, four obstacles beside them).  A tick is

    prepare() -> solve_async() -> publish(fetch=False) -> advance()

with no host array and no stream synchronisation in it: the front end reads the vessel's state from the solver's own x0 and writes the solver
inputs in place (guidance.PathFollowingFrontEnd, device-resident mode).  The plant is the controller's prediction x_1, as in the reference's
own main.py; with --plant-steps K an RK4 integrator of its own (advance_sim: x0 <- sim(x0, u_0) in K steps).

With --moving the obstacles drift at constant velocities (scenario.make_pf_missions(moving=True)): prepare() then writes the predicted
obstacle set of every stage and advance() moves the world along - the tick is the same four calls.  --no-predict holds the moving world
still inside the horizon (option "pf_predict" 0), the baseline that shows what prediction buys.

With --log-every n the loop also keeps its closed-loop trajectory - the reference's simX and its printed statistics (scripts/usv_pf_ca/
main.py:153-176, 199-207) - without a host array or a synchronisation in the tick: start_log() records (nedx, nedy, psi) of every n-th tick on the
device and sums |e| and e e of psi - ak, u - 0.7 and ye over the ticks after 400 (every tick of a shorter run); read once at the end.

    python examples/pf_mission_sweep.py --batch 8192 --ticks 560 [--plant-steps 10] [--moving [--no-predict]] [--log-every 4]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (before the solver library: one HIP runtime for both)
from mpc_collisionavoidance_amd import AcadosSim, BatchOcpSolver, BatchSimSolver, scenario, usv_models  # noqa: E402
from mpc_collisionavoidance_amd.guidance import PathFollowingFrontEnd  # noqa: E402

RING = 64   # solves whose failure counts the library keeps
ERRORS = (("psi - ak", (0, 9)), ("u - u_ref", (3, 0.7)), ("ye", (6, 0.0)))   # main.py's three statistics as (state, state | constant)
ERRORS_FIRST = 401                                                          # ... over the ticks after 400


def run(B, ticks, N=40, K=4, seed=0, plant_steps=None, quiet=False, moving=False, predict=True, log_every=None, cost=False):
    cfg = scenario.PF_MISSION_OCP
    dt = cfg["dt"]
    m = scenario.make_pf_missions(B, seed, moving=moving)
    ocp = usv_models.make_ocp("usv_model_pf_ca", N * dt, N, K)
    ocp.solver_options.sim_method_num_steps = cfg["sim_steps"]
    s = BatchOcpSolver(ocp, B)
    plant = None
    if plant_steps:
        sim = AcadosSim()
        sim.model = ocp.model
        sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = dt, int(plant_steps), False
        plant = BatchSimSolver(sim, B)
    fe = PathFollowingFrontEnd(s)
    s.set("x0", 0, m["x0"])
    s.set_all("x", np.tile(m["x0"][:, None, :], (1, N + 1, 1)))        # acados' own initial iterate: x_k = x0, u = 0
    s.set_all("u", np.zeros((B, N, 2)))
    fe.reset(m["waypoints"])
    if moving and not predict:
        s.set_option("pf_predict", 0)
    fe.set_world(m["world"], max_radius=cfg["max_radius"], margin=cfg["margin"], vel=m["world_vel"] if moving else None)
    npts = m["waypoints"].shape[1]
    fails = np.zeros(ticks, dtype=int)
    active0 = None
    if log_every:
        s.start_log(-(-ticks // log_every), every=log_every, states=[0, 10, 11], u=False, status=False, errors=[c for _, c in ERRORS],
                    errors_first=ERRORS_FIRST if ticks > ERRORS_FIRST else 0)
    if cost:
        s.track_cost(True)      # the realised closed-loop cost: every hand-over adds c_0(x0, u_0) on the device
    s.sync()
    t0 = time.perf_counter()
    for i in range(ticks):
        fe.prepare()
        s.solve_async()
        if i == 0:
            active0 = fe.publish()["active"].copy()                      # (the one read-back inside the loop)
        else:
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
    st = fe.state()
    last_active = fe.publish()["active"]                                 # (publishes the last tick again: the same values)
    k = st["wp_index"]
    # yref rewrites the rule predicts: every instance active at tick 0, plus one per switch onto a further segment - a switch whose next tick
    # has not come yet (the run ended on the switch tick) and the last switch (mission over: nothing is written) do not count
    new_segments = np.minimum(k, npts - 1) - 1 - ((k > 1) & (k < npts) & (last_active == 0))
    res = dict(ticks_per_s=ticks / el, scenario_ticks_per_s=B * ticks / el, finish_tick=st["finish_tick"], min_clearance=st["min_clearance"],
               waypoint_index=k, switches=k - 1, new_segments=new_segments, active_at_tick_0=int(active0.sum()), yref_writes=st["yref_writes"],
               failures_per_tick=fails, final_status=s.get_int("status"), final_pose=s.get("x0", 0)[:, [10, 11, 0]])
    if log_every:
        log, err = s.read_log(), s.log_errors()
        # beside final_pose, in its order (nedx, nedy, psi): [B][records][3] and the tick of each record
        res.update(log_pose=log["x"][:, :, [1, 2, 0]].copy(), log_tick=log["tick"], error_count=err["count"],
                   mean_abs_error=err["sum_abs"] / max(err["count"], 1), mean_sq_error=err["sum_sq"] / max(err["count"], 1))
    if cost:
        res["tracked_cost"], res["tracked_count"] = s.tracked_cost()
        if not quiet:
            tc = res["tracked_cost"][st["finish_tick"] >= 0]
            if tc.size:
                print("realised closed-loop cost over %d hand-overs, finished missions: min %.4f, median %.4f, max %.4f"
                      % (res["tracked_count"], tc.min(), np.median(tc), tc.max()))
            else:
                print("realised closed-loop cost over %d hand-overs: no mission has finished" % res["tracked_count"])
    if not quiet and log_every:
        print("logged %d records of (nedx, nedy, psi) per mission, one every %d ticks; errors over %d ticks:"
              % (len(res["log_tick"]), log_every, res["error_count"]))
        for c, (name, _) in enumerate(ERRORS):
            print("  %-9s mean absolute error %.6f, mean square error %.6f (means over the %d missions)"
                  % (name, res["mean_abs_error"][:, c].mean(), res["mean_sq_error"][:, c].mean(), B))
    if not quiet:
        fin = st["finish_tick"] >= 0
        print("%d missions x %d ticks in %.2f s (%.1f ticks/s, %.0f mission-ticks/s)" % (B, ticks, el, ticks / el, B * ticks / el))
        if fin.any():
            print("finished: %d of %d, at ticks %d .. %d" % (fin.sum(), B, st["finish_tick"][fin].min(), st["finish_tick"][fin].max()))
        else:
            print("finished: 0 of %d" % B)
        mc = st["min_clearance"]
        print("minimum clearance to the keep-out circle (R + 0.5 m): worst %.4f m, median %.4f m" % (mc.min(), np.median(mc)))
        print("failed solves: %d over all ticks (%d ticks with at least one); yref rewrites: %d of %d instance-ticks"
              % (fails.sum(), (fails > 0).sum(), st["yref_writes"], B * ticks))
    s.close()
    if plant is not None:
        plant.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=560)
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--plant-steps", type=int, default=None,
                    help="integrate the plant in this many RK4 steps per tick (default: the plant is the controller's prediction x_1)")
    ap.add_argument("--moving", action="store_true", help="the obstacles drift at constant velocities")
    ap.add_argument("--no-predict", action="store_true", help="with --moving: the world is held still inside the horizon (option \"pf_predict\" 0)")
    ap.add_argument("--log-every", type=int, default=None,
                    help="keep (nedx, nedy, psi) of every n-th tick and main.py's error statistics on the device (start_log)")
    ap.add_argument("--cost", action="store_true", help="sum the realised closed-loop cost of every mission on the device (track_cost)")
    a = ap.parse_args()
    run(a.batch, a.ticks, N=a.horizon, seed=a.seed, plant_steps=a.plant_steps, moving=a.moving, predict=not a.no_predict, log_every=a.log_every,
        cost=a.cost)
