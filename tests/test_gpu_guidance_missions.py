"""Device-resident missions of the guidance front end (usv_model_guidance_ca1; kernel usv_guidance_tick, arithmetic csrc/ca_guidance.hpp):
the resident tick against the host-fed calls, the pipelined lineariser across resident ticks, the moving world's arithmetic and refusals,
and the closed loop of examples/scenario_sweep.py either way."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from mpc_collisionavoidance_amd import scenario, usv_models

pytestmark = pytest.mark.gpu

M1, DT = "usv_model_guidance_ca1", 0.05
E_ARG = -1
WPS = np.array([[4.0, -5.0], [4.0, 25.0], [10.0, 30.0]])


def _solver(B, N, K):
    from mpc_collisionavoidance_amd import BatchOcpSolver
    from mpc_collisionavoidance_amd.guidance import GuidanceFrontEnd
    s = BatchOcpSolver(usv_models.make_ocp(M1, N * DT, N, K), B)
    return s, GuidanceFrontEnd(s)


def _missions(B, L, rng):
    """Three-point lists.  Instances 1 mod 5 start within 1.5 m of the second point (they switch); instances 3 mod 5 fly a TWO-POINT mission
    and start 1.8 .. 2 m from its end (they finish).  A handle has one npts for all its instances, so the two-point list is written as a
    three-point one whose last leg is 0.3 m long and points back: on the tick after the switch the vessel is within 1 m of its end and the
    mission is over."""
    wps = np.tile(WPS[None], (B, 1, 1))
    pose = np.column_stack([4.0 + rng.uniform(-1, 1, B), rng.uniform(-4.0, 10.0, B), np.pi / 2 + rng.uniform(-0.3, 0.3, B)])
    sw = np.arange(B) % 5 == 1
    fin = np.arange(B) % 5 == 3
    pose[sw] = np.column_stack([4.0 + rng.uniform(-0.3, 0.3, sw.sum()), 25.0 - rng.uniform(0.6, 1.5, sw.sum()), np.full(sw.sum(), np.pi / 2)])
    wps[fin, 2] = [4.0, 24.7]
    pose[fin] = np.column_stack([np.full(fin.sum(), 4.0), 25.0 - rng.uniform(1.8, 2.0, fin.sum()), np.full(fin.sum(), np.pi / 2)])
    vel = np.column_stack([np.full(B, 0.7), rng.uniform(-0.02, 0.02, B)])
    vel[0, 0] = 0.0                                                              # u == 0 -> 0.001
    world = np.concatenate([4.0 + rng.uniform(-7, 7, (B, L, 1)), rng.uniform(-12.0, 42.0, (B, L, 1)), rng.uniform(0.2, 0.8, (B, L, 1))], axis=2)
    return wps, pose, vel, world, sw, fin


def _clearance(pose, world, max_radius):
    """numpy, per instance: min over the visible entries of sqrt(dx^2 + dy^2) - (R + 0.5) (examples/scenario_sweep.py); inf: none visible"""
    r = np.sqrt((pose[:, None, 0] - world[:, :, 0]) ** 2 + (pose[:, None, 1] - world[:, :, 1]) ** 2)
    d = np.where(r < max_radius, r - (world[:, :, 2] + 0.5), np.inf)
    return d.min(axis=1) if world.shape[1] else np.full(len(pose), np.inf)


@pytest.mark.parametrize("K,L", [(8, 12), (3, 64), (8, 0)])
def test_resident_equals_host_fed_bit_for_bit(K, L):
    """Solver A: sense(pose, world) -> prepare(vel, pose) -> solve -> publish -> x1 = get("x", 1).  Solver B: set_world once, x0 once, then
    prepare() -> solve_async -> publish -> advance(0, seed).  Compared on every tick, per instance:
      - up to the last ACTIVE tick: x0, stage 0 of p / lh, all of x and u, wp_index, past_psied, the published arrays;
      - on the tick that ENDS the mission (the first inactive one): stage 0 of p / lh, wp_index, past_psied and the published arrays.  x0, x
        and u cannot agree there: neither front end writes x0 on an inactive tick, so A solves from the x0 its last active prepare wrote
        and B from the x_1 advance left in its place.
    B's min_clearance against numpy on A's poses (visible entries, ticks up to the one that ends the mission)."""
    B, N, T, R = 70, 20, 40, 18.0
    rng = np.random.default_rng(31 + L)
    wps, pose, vel, world, sw, fin = _missions(B, L, rng)
    sA, feA = _solver(B, N, K)
    sB, feB = _solver(B, N, K)
    feA.reset(wps, pose[:, 2])
    feB.reset(wps, pose[:, 2])
    x0 = np.zeros((B, 8))
    x0[:, 0:2], x0[:, 5:8] = vel, pose
    sB.set("x0", 0, x0)
    feB.set_world(world, max_radius=R)
    st = feB.mission_state()
    assert (st["min_clearance"] == 1e300).all() and (st["finish_tick"] == -1).all() and (st["wp_index"] == 1).all()
    finish = np.full(B, -1)
    want_mc = np.full(B, np.inf)
    nvis = []
    for i in range(T):
        feA.sense(pose, world, max_radius=R)
        feA.prepare(vel, pose)
        sA.solve()
        outA = feA.publish()
        kA, ppA = feA.state()
        feB.prepare()
        sB.solve_async()
        outB = feB.publish()                                                      # (one fetched publish: it waits for the stream)
        stB = feB.mission_state()
        alive = finish < 0
        active = alive & (outA["active"] != 0)
        for f in ("x0", "x", "u"):
            a = sA.get("x0", 0) if f == "x0" else sA.get_all(f)
            b = sB.get("x0", 0) if f == "x0" else sB.get_all(f)
            assert a[active].tobytes() == b[active].tobytes(), (i, f)
        for f in ("p", "lh"):
            assert sA.get(f, 0)[alive].tobytes() == sB.get(f, 0)[alive].tobytes(), (i, f)
        assert np.array_equal(kA[alive], stB["wp_index"][alive]) and ppA[alive].tobytes() == stB["past_psied"][alive].tobytes(), i
        for f in ("heading", "r", "speed", "ye", "active"):
            assert outA[f][alive].tobytes() == outB[f][alive].tobytes(), (i, f)
        want_mc[alive] = np.minimum(want_mc[alive], _clearance(pose[alive], world[alive], R))
        if L:
            nvis.append((np.hypot(pose[:, None, 0] - world[:, :, 0], pose[:, None, 1] - world[:, :, 1]) < R).sum(axis=1))
        finish[alive & (outA["active"] == 0)] = i
        sB.advance(0.0, i)
        x1 = sA.get("x", 1)
        vel, pose = x1[:, 0:2].copy(), x1[:, 5:8].copy()
    st = feB.mission_state()
    assert np.array_equal(st["finish_tick"], finish)
    assert (finish[fin] >= 0).all() and (finish[~fin] == -1).all()
    assert (st["wp_index"][sw] == 2).all() and (st["wp_index"][fin] == 3).all()
    assert np.array_equal(st["min_clearance"], np.where(np.isinf(want_mc), 1e300, want_mc))
    if L:
        nvis = np.array(nvis)
        assert (nvis > K).any()                                                   # the ranked choice ...
        assert K < 8 or ((nvis <= K) & (nvis > 0)).any()                          # ... and, at L = 12, list order too
    sA.close(); sB.close()


def test_pipelined_lineariser_survives_resident_ticks():
    B, N, K, L, T = 16384, 20, 8, 5, 8
    m = scenario.make_ca_missions(B, L, seed=3)
    x0 = np.zeros((B, 8))
    x0[:, 0:2], x0[:, 5:8] = m["vel"], m["pose"]
    runs = {}
    for pipe in (1, 0):
        s, fe = _solver(B, N, K)
        s.set_option("pipeline_linearize", pipe)
        fe.reset(m["waypoints"], m["pose"][:, 2])
        s.set("x0", 0, x0)
        fe.set_world(m["world"])
        rec = []
        for i in range(T):
            fe.prepare()
            s.solve_async()
            fe.publish(fetch=False)
            s.advance(0.0, i)
            s.sync()
            rec.append((s.get_all("x"), s.get_all("u"), s.get("x0", 0)))
        runs[pipe] = (rec, s.pipeline_stats())
        s.close()
    for i in range(T):
        for a, b in zip(runs[1][0][i], runs[0][0][i]):
            assert a.tobytes() == b.tobytes(), i
    used, discarded = runs[1][1]
    assert used >= 5 and discarded == 0, (used, discarded)
    assert runs[0][1] == (0, 0)


def test_moving_world_arithmetic_and_refusals():
    B, N, K, L, R = 70, 20, 8, 12, 18.0
    rng = np.random.default_rng(9)
    wps, pose, vel, world, sw, fin = _missions(B, L, rng)
    wvel = rng.uniform(-0.3, 0.3, (B, L, 2))
    x0 = np.zeros((B, 8))
    x0[:, 0:2], x0[:, 5:8] = vel, pose
    dp = C.POINTER(C.c_double)

    def err(s):
        return s._lib.usvmpc_last_error(s._h).decode()

    # ---- refusals: another model, no reset, no world, not finite, the tracks either way round, one of vel_uv / pose
    from mpc_collisionavoidance_amd import BatchOcpSolver
    s0 = BatchOcpSolver(usv_models.make_ocp("usv_model_pf_ca", N * 0.01, N, 4), B)
    lib = s0._lib
    assert lib.usvmpc_guidance_world(s0._h, world.ctypes.data_as(dp), L, R) == E_ARG and M1 in err(s0)
    assert lib.usvmpc_guidance_world_vel(s0._h, wvel.ctypes.data_as(dp), 1) == E_ARG and M1 in err(s0)
    assert lib.usvmpc_guidance_world_step(s0._h, 0.05) == E_ARG and M1 in err(s0)
    assert lib.usvmpc_guidance_world_read(s0._h, None, None) == E_ARG and M1 in err(s0)
    assert lib.usvmpc_guidance_mission_state(s0._h, None, None, None, None) == E_ARG and M1 in err(s0)
    s0.close()
    s, fe = _solver(B, N, K)
    assert lib.usvmpc_guidance_world(s._h, world.ctypes.data_as(dp), L, R) == E_ARG and "usvmpc_guidance_reset" in err(s)
    fe.reset(wps, pose[:, 2])
    s.set("x0", 0, x0)
    assert lib.usvmpc_guidance_prepare(s._h, None, None, None, None, 0) == E_ARG and "world list" in err(s)
    assert lib.usvmpc_guidance_prepare(s._h, x0.ctypes.data_as(dp), None, None, None, 0) == E_ARG and "both" in err(s)
    with pytest.raises(Exception, match="both"):
        fe.prepare(vel)
    assert lib.usvmpc_guidance_world_vel(s._h, wvel.ctypes.data_as(dp), 1) == E_ARG and "no world list yet" in err(s)
    assert lib.usvmpc_guidance_world_read(s._h, None, None) == E_ARG and "no world list yet" in err(s)
    bad = world.copy()
    bad[5, 3, 1] = np.nan
    assert lib.usvmpc_guidance_world(s._h, bad.ctypes.data_as(dp), L, R) == E_ARG and "NaN" in err(s)
    assert lib.usvmpc_guidance_world(s._h, world.ctypes.data_as(dp), 65, R) == E_ARG and "0..64" in err(s)
    fe.set_world(world, max_radius=R)
    assert lib.usvmpc_guidance_world_step(s._h, 0.05) == E_ARG and "at rest" in err(s)
    for b in (np.nan, np.inf, -np.inf):
        v = wvel.copy()
        v[3, 2, 1] = b
        assert lib.usvmpc_guidance_world_vel(s._h, v.ctypes.data_as(dp), 1) == E_ARG and "not finite" in err(s)
    assert np.array_equal(fe.world()[0], world) and np.array_equal(fe.world()[1], np.zeros((B, L, 2)))   # nothing changed: still at rest
    s2, fe2 = _solver(B, N, K)
    fe2.reset(wps, pose[:, 2])
    s2.set_obstacle_tracks(np.zeros((B, K, 2)) + 50.0)
    assert lib.usvmpc_guidance_world(s2._h, world.ctypes.data_as(dp), L, R) == 0
    assert lib.usvmpc_guidance_world_vel(s2._h, wvel.ctypes.data_as(dp), 1) == E_ARG and "obstacle_tracks" in err(s2)
    s2.set_option("obstacle_tracks", 0)
    assert lib.usvmpc_guidance_world_vel(s2._h, wvel.ctypes.data_as(dp), 1) == 0
    with pytest.raises(Exception, match="world moves"):
        s2.set_option("obstacle_tracks", 1)
    s2.close()

    # ---- at rest: the reference for stage 0
    fe.prepare()
    p_rest, lh_rest, x0_rest = s.get_all("p"), s.get_all("lh"), s.get("x0", 0)
    # ---- predict = 1: every stage
    s.set("x0", 0, x0)
    fe.reset(wps, pose[:, 2])
    fe.set_world(world, max_radius=R, vel=wvel, predict=True)
    fe.prepare()
    p, lh = s.get_all("p"), s.get_all("lh")
    assert p[:, 0].tobytes() == p_rest[:, 0].tobytes() and lh[:, 0].tobytes() == lh_rest[:, 0].tobytes()
    assert s.get("x0", 0).tobytes() == x0_rest.tobytes()
    # which world entry sits behind a slot: the one whose float32-rounded NED position the slot holds (distinct random positions)
    P0 = p[:, 0].reshape(B, K, 2)
    parked = (P0[:, :, 0] == 1000.0) & (lh[:, 0] == 0.0)
    assert parked.any() and (~parked).any()
    dist = np.abs(P0[:, :, None, :] - world[:, None, :, :2]).max(axis=3)          # [B, K, L]
    idx = dist.argmin(axis=2)
    assert (dist.min(axis=2)[~parked] < 1e-5).all()
    v = np.take_along_axis(wvel, idx[:, :, None].repeat(2, axis=2), axis=1)      # [B, K, 2]
    v[parked] = 0.0
    kdt = (np.arange(N + 1, dtype=float) * DT)[None, :, None, None]
    want = (P0[:, None] + kdt * v[:, None]).reshape(B, N + 1, 2 * K)
    assert p.tobytes() == want.tobytes()
    assert (p.reshape(B, N + 1, K, 2)[np.nonzero(parked)[0], :, np.nonzero(parked)[1]] == 1000.0).all()
    assert lh.tobytes() == np.tile(lh[:, :1], (1, N, 1)).tobytes() and (lh.transpose(0, 2, 1)[parked] == 0.0).all()
    # ---- the world moves with advance and with step_world
    s.solve()
    s.advance()
    w1 = world.copy()
    w1[:, :, :2] = world[:, :, :2] + DT * wvel
    assert fe.world()[0].tobytes() == w1.tobytes() and fe.world()[1].tobytes() == wvel.tobytes()
    fe.step_world(0.37)
    w2 = w1.copy()
    w2[:, :, :2] = w1[:, :, :2] + 0.37 * wvel
    assert fe.world()[0].tobytes() == w2.tobytes()
    # the same n_world keeps the velocities, another one drops them
    fe.set_world(world, max_radius=R, vel=wvel, predict=True)
    assert lib.usvmpc_guidance_world(s._h, w2.ctypes.data_as(dp), L, R) == 0
    assert np.array_equal(fe.world()[0], w2) and np.array_equal(fe.world()[1], wvel)
    w3 = np.ascontiguousarray(world[:, :L - 1])
    assert lib.usvmpc_guidance_world(s._h, w3.ctypes.data_as(dp), L - 1, R) == 0
    fe._L = L - 1
    assert np.array_equal(fe.world()[0], w3) and np.array_equal(fe.world()[1], np.zeros((B, L - 1, 2)))
    assert lib.usvmpc_guidance_world_step(s._h, 0.05) == E_ARG and "at rest" in err(s)
    # ---- predict = 0: stage 0 only (sentinels stay), "static_obstacles" on: the solve equals one with stage 0 on every stage
    s.set("x0", 0, x0)
    fe.reset(wps, pose[:, 2])
    fe.set_world(world, max_radius=R, vel=wvel, predict=False)
    s.set_all("p", np.full((B, N + 1, 2 * K), -5.0))
    s.set_all("lh", np.full((B, N, K), -6.0))
    fe.prepare()
    p, lh = s.get_all("p"), s.get_all("lh")
    assert (p[:, 1:] == -5.0).all() and (lh[:, 1:] == -6.0).all()
    assert p[:, 0].tobytes() == p_rest[:, 0].tobytes() and lh[:, 0].tobytes() == lh_rest[:, 0].tobytes()
    xs, us = s.get_all("x"), s.get_all("u")                                       # (the iterate this solve starts from)
    s.solve()
    s3, _ = _solver(B, N, K)
    s3.set("x0", 0, s.get("x0", 0))
    s3.set_all("x", xs)
    s3.set_all("u", us)
    s3.set_all("p", np.tile(p[:, :1], (1, N + 1, 1)))
    s3.set_all("lh", np.tile(lh[:, :1], (1, N, 1)))
    s3.solve()
    assert s3.get_all("x").tobytes() == s.get_all("x").tobytes() and s3.get_all("u").tobytes() == s.get_all("u").tobytes()
    s.advance()                                                                   # held still inside the horizon, but it moves between ticks
    assert fe.world()[0].tobytes() == w1.tobytes()
    s3.close(); s.close()

    # ---- zero velocities with predict = 1: the same x / u bits over 10 ticks as the world at rest
    out = []
    for moving in (False, True):
        s, fe = _solver(B, N, K)
        fe.reset(wps, pose[:, 2])
        s.set("x0", 0, x0)
        fe.set_world(world, max_radius=R, vel=np.zeros((B, L, 2)) if moving else None, predict=True)
        rec = []
        for i in range(10):
            fe.prepare()
            s.solve_async()
            fe.publish(fetch=False)
            s.advance(0.0, i)
            s.sync()
            rec.append((s.get_all("x"), s.get_all("u")))
        out.append(rec)
        s.close()
    for i in range(10):
        assert out[0][i][0].tobytes() == out[1][i][0].tobytes() and out[0][i][1].tobytes() == out[1][i][1].tobytes(), i


def _sweep():
    spec = importlib.util.spec_from_file_location("scenario_sweep", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "scenario_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_closed_loop_resident_equals_host_fed():
    """examples/scenario_sweep.py, 96 scenarios, 200 ticks, N = 100.  The two loops define min_clearance one tick apart: the host-fed loop
    takes the poses AFTER each tick (pose_1 .. pose_200), the resident front end the poses its ticks were PREPARED at (pose_0 .. pose_199).
    Shifted by that tick they are the same numbers: min(resident, d(pose_200)) == min(host-fed, d(pose_0)), with d numpy's expression, pose_0
    the generator's start pose and pose_200 the final pose (which both loops report, and which must be the same bits)."""
    mod = _sweep()
    a = mod.run(B=96, ticks=200, N=100, quiet=True)
    b = mod.run(B=96, ticks=200, N=100, quiet=True, resident=True)
    assert set(a) <= set(b)
    assert np.array_equal(a["waypoint_index"], b["waypoint_index"])
    assert not a["solver_failures"].any() and not b["solver_failures"].any() and not b["fail_counts"].any()
    assert a["final_pose"].tobytes() == b["final_pose"].tobytes()
    m = scenario.make_ca_missions(96, 5, 0)
    d0 = _clearance(m["pose"], m["world"], 100.0)
    d200 = _clearance(a["final_pose"], m["world"], 100.0)
    assert np.array_equal(np.minimum(b["min_clearance"], d200), np.minimum(a["min_clearance"], d0))


def test_closed_loop_moving_world():
    mod = _sweep()
    r = mod.run(B=96, ticks=200, N=100, quiet=True, resident=True, moving=True)
    assert not r["solver_failures"].any() and not r["fail_counts"].any()
    assert (r["final_pose"][:, 1] > 0.0).all()                                    # started at y = -5: 10 s at 0.7 m/s
