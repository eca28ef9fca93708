#!/usr/bin/env python3
"""A batched closed loop against MOVING obstacles with the whole tick on the device: the obstacles are tracks (position + constant
velocity per slot) held by the solver, which derives the per-stage obstacle sets itself before every solve and moves the world along
with every hand-over (option "obstacle_tracks", include/usvmpc.h).  Default: BASELINE configs[4]'s OCP (usv_model_pf_ca, N = 80,
20 moving obstacles); `--model usv_model_guidance_ca1` for the soft-row model.  With --plant-steps K the plant is an integrator of
its own (the same model over the same 0.05 s in K RK4 steps) instead of the controller's prediction x_1.  Nothing but the status comes
back per tick; the clearance actually kept is accumulated on the device.

    python examples/moving_obstacles.py --batch 8192 --ticks 100 [--plant-steps 10]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (before the solver library: one HIP runtime for both)
from mpc_collisionavoidance_amd import AcadosSim, BatchOcpSolver, BatchSimSolver, scenario, usv_models  # noqa: E402


def run(name="usv_model_pf_ca", B=8192, ticks=100, N=80, K=20, seed=1234, sigma=1e-3, plant_steps=None, quiet=False):
    dt = scenario.BENCH_DT
    wl = scenario.make_bench_batch(name, N, K, B, seed=seed, moving=True)
    ocp = usv_models.make_ocp(name, N * dt, N, K)
    ocp.solver_options.sim_method_num_steps = scenario.BENCH_SIM_STEPS[name]
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, wl)
    scenario.load_tracks(s, wl)                      # p is derived from here on; advance moves the world
    s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
    plant = None
    if plant_steps:
        sim = AcadosSim()
        sim.model = ocp.model
        sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = dt, int(plant_steps), False
        plant = BatchSimSolver(sim, B)
    bad = np.zeros(B, dtype=bool)
    t0 = time.perf_counter()
    for t in range(ticks):
        bad |= s.solve() != 0                        # the only per-tick device-to-host copy
        if plant is None:
            s.advance(sigma, seed=t)
        else:
            s.advance_sim(plant, sigma=sigma, seed=t)
    s.sync()
    el = time.perf_counter() - t0
    min_clear = s.get("clearance_min", 0)
    res = dict(scenario_ticks_per_s=B * ticks / el, min_clearance=min_clear, solver_failures=bad, unconverged=s.unconverged_total())
    if not quiet:
        print("%s, N = %d, %d moving obstacles: %d scenarios x %d ticks in %.2f s (%.0f scenario-ticks/s)" % (name, N, K, B, ticks, el, B * ticks / el))
        print("minimum clearance to a keep-out circle over the run: worst %.3f m, 1st percentile %.3f m, median %.3f m"
              % (min_clear.min(), np.percentile(min_clear, 1), np.median(min_clear)))
        print("scenarios with a solver failure: %d; QPs not converged to the IPM tolerances: %d of %d" % (bad.sum(), res["unconverged"], B * ticks))
    s.close()
    if plant is not None:
        plant.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="usv_model_pf_ca", choices=["usv_model_pf_ca", "usv_model_guidance_ca1"])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--horizon", type=int, default=80)
    ap.add_argument("--obstacles", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=1e-3, help="standard deviation of the disturbance added at the hand-over")
    ap.add_argument("--plant-steps", type=int, default=None,
                    help="integrate the plant in this many RK4 steps per tick (default: the plant is the controller's prediction x_1)")
    a = ap.parse_args()
    run(a.model, a.batch, a.ticks, a.horizon, a.obstacles, sigma=a.sigma, plant_steps=a.plant_steps)
