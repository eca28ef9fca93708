"""The path-following front end over a MOVING world on a real MI355X (`pytest -m gpu`): usv_pf_prepare's track selection and its p / lh
stream, usv_pf_world_step, the C ABI usvmpc_pf_world_vel / _world_step / _world_read, option "pf_predict", guidance.PathFollowingFrontEnd.

* host-fed, against the numpy restatement (tests/pf_moving_ref.py) over the scripted sequences: x0, p and lh of every stage and the world
  read-back bit for bit, yref as tests/test_gpu_pf_frontend.py compares it;
* device-resident == host-fed, bit for bit, the world stepped by advance;
* the front end's handle == a plain handle fed the same arrays stage by stage;
* "pf_predict" 0 == a static front end whose world the host steps and re-uploads;
* instances whose mission is over keep p and lh;
* the world step: advance, advance_sim, "obstacle_step_on_advance" 0, usvmpc_pf_world_step against numpy;
* what the front end feeds the solver, through the CPU oracle, under the project's parity rule;
* the mission sweep of examples/pf_mission_sweep.py over a moving world against the oracle's own run (profiles/pf_moving_oracle.txt);
* refusals.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from mpc_collisionavoidance_amd import AcadosSim, BatchOcpSolver, BatchSimSolver, scenario, usv_models
from mpc_collisionavoidance_amd.guidance import PathFollowingFrontEnd
from tests import parity_rule, util
from tests import pf_frontend_ref as R
from tests import pf_moving_ref as MR

pytestmark = pytest.mark.gpu

M1, M2 = "usv_model_guidance_ca1", "usv_model_pf_ca"
DT, STEPS = 0.05, 5
# a state the model can be linearised at (u = 0 is not one): heading up leg 1 at 0.7 m/s
GENERIC = np.array([np.pi / 2, 1.0, 0.0, 0.7, 0.0, 0.0, 0.0, 4.0, -5.0, np.pi / 2, 4.0, -4.5, 0.0, 0.0])


def _solver(B, N, K=4, x0=None):
    ocp = usv_models.make_ocp(M2, N * DT, N, K)
    ocp.solver_options.sim_method_num_steps = STEPS
    s = BatchOcpSolver(ocp, B)
    x0 = np.tile(GENERIC, (B, 1)) if x0 is None else x0
    s.set("x0", 0, x0)
    s.set_all("x", np.tile(x0[:, None, :], (1, N + 1, 1)))
    s.set_all("u", np.zeros((B, N, 2)))
    s.set_all("yref", np.zeros((B, N, 16)))
    s.set("yref", N, np.zeros((B, 14)))
    return ocp, s


def _beside_leg_1(B, L, rng, vmax=0.1):
    """Obstacles beside leg 1 (x = 4, heading +y), not on it, drifting slowly: a closed loop from GENERIC stays solvable"""
    world = np.concatenate([4.0 + rng.uniform(-2.5, 2.5, (B, L, 1)), rng.uniform(-4.0, 0.0, (B, L, 1)), rng.uniform(0.1, 0.3, (B, L, 1))], axis=2)
    near = np.abs(world[:, :, 0] - 4.0) < 1.6
    world[:, :, 0] = np.where(near, 4.0 + np.sign(world[:, :, 0] - 4.0 + 1e-30) * 1.6, world[:, :, 0])
    vel = rng.uniform(-vmax, vmax, (B, L, 2))
    vel[:, :, 0] = np.abs(vel[:, :, 0]) * np.sign(world[:, :, 0] - 4.0)        # away from the leg
    return world, vel


def _starts(B, rng):
    x0 = np.tile(GENERIC, (B, 1))
    x0[:, 10] += rng.uniform(-0.5, 0.5, B)
    x0[:, 11] += rng.uniform(-0.3, 0.3, B)
    x0[:, 0] += rng.uniform(-0.2, 0.2, B)
    x0[:, 4] = rng.uniform(-0.02, 0.02, B)
    return x0


# ---- 6. host-fed against the numpy restatement
@pytest.mark.parametrize("B,N,K,L,classes", [(70, 6, 4, 0, None), (70, 6, 4, 9, None), (70, 6, 20, 30, None), (1, 6, 4, 3, [2]),
                                             (70, 5, 3, 9, None)])      # (N K odd: a pair of lh can straddle two instances)
def test_host_fed_front_end_is_the_reference(B, N, K, L, classes):
    T = 12
    rng = np.random.default_rng(600 + L)
    wps, vel, pose = R.scripted_sequence(B, T, classes=classes)
    world, wvel = MR.make_world(B, L, rng)
    ocp, s = _solver(B, N, K)
    fe = PathFollowingFrontEnd(s)
    fe.reset(wps)
    fe.set_world(world, max_radius=12.0, vel=wvel)
    ref = MR.PfMovingRef(B, N, K, s.dt)        # (the handle's own dt = Tf / N: N * 0.05 / N need not be 0.05)
    ref.x0[:] = GENERIC
    ref.reset(wps)
    ref.set_world(world, 12.0, wvel)
    seen, moved = set(), False
    for t in range(T):
        fe.prepare(vel[t], pose[t])
        ref.prepare(vel[t], pose[t])
        p, lh = s.get_all("p"), s.get_all("lh")
        st = fe.state()
        got = dict(x0=s.get("x0", 0), yref=s.get_all("yref"), yref_e=s.get("yref", N), p0=p[:, 0], lh0=lh[:, 0], k=st["wp_index"],
                   finish_tick=st["finish_tick"], min_clearance=st["min_clearance"])
        what = "B %d N %d K %d L %d tick %d" % (B, N, K, L, t)
        R.check(ref, got, what)
        assert st["yref_writes"] == ref.yref_writes, (what, st["yref_writes"], ref.yref_writes)
        assert np.array_equal(p, ref.p), what + " p"
        assert np.array_equal(lh, ref.lh), what + " lh"
        moved |= bool((p[:, N] != p[:, 0]).any())
        fe.step_world(DT)
        ref.step_world(DT)
        w, v = fe.world()
        assert np.array_equal(w, ref.world) and np.array_equal(v, ref.wvel), what + " world"
        seen |= set(ref.phase.tolist())
    assert seen == {R.OVER, R.ACTIVE, R.SWITCH} or classes is not None
    assert moved == (L > 0)
    s.close()


# ---- 7. device-resident == host-fed
def test_device_resident_equals_host_fed_bit_for_bit():
    """No instance switches inside the window (tests/test_gpu_pf_frontend.py, test 7, says why)."""
    B, N, K, L, T = 70, 6, 4, 9, 10
    rng = np.random.default_rng(77)
    x0 = _starts(B, rng)
    world, wvel = _beside_leg_1(B, L, rng)
    wps = scenario.PF_MISSION_WAYPOINTS
    hs = []
    for _ in range(2):
        ocp, s = _solver(B, N, K, x0)
        s.set_option("disturbance_mask", (1 << 3) | (1 << 5))
        fe = PathFollowingFrontEnd(s)
        fe.reset(wps)
        fe.set_world(world, vel=wvel)
        hs.append((s, fe))
    (sa, fa), (sb, fb) = hs
    w = world.copy()
    for t in range(T):
        fa.prepare()
        xb = sb.get("x0", 0)
        fb.prepare(xb[:, 3:6], xb[:, [10, 11, 0]])
        for f in ("x0", "yref", "p", "lh"):
            a, b = (sa.get("x0", 0), sb.get("x0", 0)) if f == "x0" else (sa.get_all(f), sb.get_all(f))
            assert np.array_equal(a, b), (t, f)
        pa = sa.get_all("p")
        assert (pa[:, N] != pa[:, 0]).any()
        sa.solve_async(), sb.solve()
        sa.sync()
        assert np.array_equal(sa.get_all("x"), sb.get_all("x")) and np.array_equal(sa.get_all("u"), sb.get_all("u")), t
        oa, ob = fa.publish(), fb.publish()
        for nm in oa:
            assert np.array_equal(oa[nm], ob[nm]), (t, nm)
        assert oa["active"].all()
        sa.advance(1e-3, 100 + t), sb.advance(1e-3, 100 + t)
        w[:, :, :2] = w[:, :, :2] + sa.dt * wvel
        for f in (fa, fb):
            assert np.array_equal(f.world()[0], w), t
    assert np.array_equal(sa.get("x0", 0), sb.get("x0", 0))
    sta, stb = fa.state(), fb.state()
    assert sta["yref_writes"] == stb["yref_writes"] == B and np.array_equal(sta["min_clearance"], stb["min_clearance"])
    assert (sta["min_clearance"] < 1e300).all()
    sa.close(), sb.close()


# ---- 8. the front end's handle == a plain handle
@pytest.mark.parametrize("K,L", [(4, 9), (20, 30)])
def test_front_end_handle_equals_a_plain_handle(K, L):
    B, N = 70, 6
    rng = np.random.default_rng(80 + K)
    x0 = _starts(B, rng)
    world, wvel = _beside_leg_1(B, L, rng, vmax=0.5)
    ocp, s = _solver(B, N, K, x0)
    fe = PathFollowingFrontEnd(s)
    fe.reset(scenario.PF_MISSION_WAYPOINTS)
    fe.set_world(world, vel=wvel)
    fe.prepare()
    x0d, yref, yref_e, p, lh = s.get("x0", 0), s.get_all("yref"), s.get("yref", N), s.get_all("p"), s.get_all("lh")
    assert (p[:, 0] != 1000.0).any() and (p[:, N] != p[:, 0]).any()
    s.solve()
    ocp2, s2 = _solver(B, N, K, x0)
    s2.set_option("static_obstacles", 0)
    s2.set("x0", 0, x0d)
    for k in range(N):
        s2.set("yref", k, yref[:, k])
        s2.set("lh", k, lh[:, k])
    s2.set("yref", N, yref_e)
    for k in range(N + 1):
        s2.set("p", k, p[:, k])
    s2.solve()
    assert np.array_equal(s2.get_all("x"), s.get_all("x")) and np.array_equal(s2.get_all("u"), s.get_all("u"))
    # and the stages matter: the same handle with stage 0's set on every stage solves something else
    s2.set_all("x", np.tile(x0[:, None, :], (1, N + 1, 1)))
    s2.set_all("u", np.zeros((B, N, 2)))
    s2.set_all("p", np.tile(p[:, :1], (1, N + 1, 1)))
    s2.solve()
    print("instances whose solution the predicted stages change: %d of %d" % ((s2.get_all("u") != s.get_all("u")).any(axis=(1, 2)).sum(), B))
    s.close(), s2.close()


# ---- 9. "pf_predict" 0 == a static front end whose world the host moves
def test_pf_predict_0_equals_a_static_front_end():
    B, N, K, L, T = 70, 6, 4, 9, 4
    rng = np.random.default_rng(9)
    x0 = _starts(B, rng)
    world, wvel = _beside_leg_1(B, L, rng)
    wps = scenario.PF_MISSION_WAYPOINTS
    ocp, sa = _solver(B, N, K, x0)
    sa.set_option("pf_predict", 0)
    fa = PathFollowingFrontEnd(sa)
    fa.reset(wps)
    fa.set_world(world, vel=wvel)
    ocp, sb = _solver(B, N, K, x0)
    fb = PathFollowingFrontEnd(sb)
    fb.reset(wps)
    w = world.copy()
    p_init = sa.get_all("p")
    for t in range(T):
        fb.set_world(w)
        fa.prepare(), fb.prepare()
        pa, pb = sa.get_all("p"), sb.get_all("p")
        assert np.array_equal(pa, pb) and np.array_equal(sa.get_all("lh"), sb.get_all("lh")), t
        assert np.array_equal(pa[:, 1:], p_init[:, 1:]) and (pa[:, 0] != 0.0).all()   # stage 0 only
        sa.solve(), sb.solve()
        assert np.array_equal(sa.get_all("x"), sb.get_all("x")) and np.array_equal(sa.get_all("u"), sb.get_all("u")), t
        fa.publish(fetch=False), fb.publish(fetch=False)
        sa.advance(), sb.advance()
        w[:, :, :2] = w[:, :, :2] + sa.dt * wvel
        assert np.array_equal(fa.world()[0], w), t
    assert not np.array_equal(w, world)
    sa.close(), sb.close()


# ---- 10. instances whose mission is over keep p and lh
def test_finished_instances_keep_p_and_lh():
    B, N, K, L, T = 70, 6, 4, 9, 6
    classes = [0] * 30 + [3] * 40                  # cruising | over from tick 3
    cls = np.array(classes)
    rng = np.random.default_rng(10)
    wps, vel, pose = R.scripted_sequence(B, T, classes=classes)
    world, wvel = MR.make_world(B, L, rng)
    ocp, s = _solver(B, N, K)
    fe = PathFollowingFrontEnd(s)
    fe.reset(wps)
    fe.set_world(world, max_radius=12.0, vel=wvel)
    ref = MR.PfMovingRef(B, N, K, s.dt)        # (the handle's own dt = Tf / N: N * 0.05 / N need not be 0.05)
    ref.reset(wps)
    ref.set_world(world, 12.0, wvel)
    for t in range(T):
        if t >= 3:
            s.set_all("p", np.full((B, N + 1, 2 * K), -7.0 - t))
            s.set_all("lh", np.full((B, N, K), -3.0 - t))
        fe.prepare(vel[t], pose[t])
        ref.prepare(vel[t], pose[t])
        p, lh = s.get_all("p"), s.get_all("lh")
        over = ref.phase == R.OVER
        assert over.any() == (t >= 3) and (over == ((cls == 3) & (t >= 3))).all()
        assert np.array_equal(p[~over], ref.p[~over]) and np.array_equal(lh[~over], ref.lh[~over]), t
        if t >= 3:
            assert (p[over] == -7.0 - t).all() and (lh[over] == -3.0 - t).all(), t
    s.close()


# ---- 11. the world step
def test_world_step():
    B, N, K, L = 70, 6, 4, 9
    rng = np.random.default_rng(11)
    world, wvel = MR.make_world(B, L, rng)
    ocp, s = _solver(B, N, K)
    fe = PathFollowingFrontEnd(s)
    fe.reset(scenario.PF_MISSION_WAYPOINTS)
    fe.set_world(world, vel=wvel)
    w = world.copy()
    assert np.array_equal(fe.world()[0], w) and np.array_equal(fe.world()[1], wvel)
    s.advance()                                                  # one shooting interval
    w[:, :, :2] = w[:, :, :2] + s.dt * wvel
    assert np.array_equal(fe.world()[0], w)
    sim = AcadosSim()
    sim.model = ocp.model
    sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = 0.02, 2, False
    plant = BatchSimSolver(sim, B)
    s.advance_sim(plant)                                         # the plant's period
    w[:, :, :2] = w[:, :, :2] + 0.02 * wvel
    assert np.array_equal(fe.world()[0], w)
    s.set_option("obstacle_step_on_advance", 0)                  # the world is the caller's to move
    s.advance(), s.advance_sim(plant)
    assert np.array_equal(fe.world()[0], w)
    for T in (0.013, -0.4, 0.0):
        fe.step_world(T)
        w[:, :, :2] = w[:, :, :2] + T * wvel
        assert np.array_equal(fe.world()[0], w), T
    assert np.array_equal(fe.world()[0][:, :, 2], world[:, :, 2]) and np.array_equal(fe.world()[1], wvel)
    s.set_option("obstacle_step_on_advance", 1)
    s.advance()
    w[:, :, :2] = w[:, :, :2] + s.dt * wvel
    assert np.array_equal(fe.world()[0], w)
    plant.close()
    s.close()


# ---- 12. what the front end feeds the solver, through the oracle
def pf_parity_starts(B, seed=0):
    """tests/test_gpu_pf_frontend.pf_parity_starts with the moving generator: instances started 1 .. 3 m short of the nearer obstacle of
    leg 1 (measured along the leg), on the leg, heading along it at 0.7 m/s."""
    m = scenario.make_pf_missions(B, seed, moving=True)
    rng = np.random.default_rng(1000 + seed)
    x0 = m["x0"].copy()
    first = np.minimum(m["world"][:, 0, 1], m["world"][:, 2, 1])       # obstacles 0 and 2 lie beside leg 1 (x = 4, heading +y)
    x0[:, 0] = np.pi / 2
    x0[:, 1], x0[:, 2] = 1.0, 0.0
    x0[:, 3] = 0.7
    x0[:, 10] = 4.0
    x0[:, 11] = first - rng.uniform(1.0, 3.0, B)
    return m, x0


def test_front_end_feeds_the_solver_what_the_oracle_gets(oracle):
    B, T = 32, 25
    cfg = scenario.PF_MISSION_OCP
    N, K = cfg["N"], cfg["K"]
    m, x0 = pf_parity_starts(B)
    ocp, s = _solver(B, N, K, x0)
    fe = PathFollowingFrontEnd(s)
    fe.reset(m["waypoints"])
    fe.set_world(m["world"], max_radius=cfg["max_radius"], margin=cfg["margin"], vel=m["world_vel"])
    spec = oracle.spec(util.MODEL_ID[M2], N, N * DT, K, sim_steps=STEPS)
    n_active_rows = 0
    for t in range(T):
        fe.prepare()
        xin, uin = s.get_all("x"), s.get_all("u")
        x0d, p, lh = s.get("x0", 0), s.get_all("p"), s.get_all("lh")
        assert (p[:, N] != p[:, 0]).any()
        data = (s.get_all("yref"), s.get("yref", N), p, lh)              # the device's p / lh of every stage, no tiling
        xs, us = xin.copy(), uin.copy()
        s.solve()
        sts, its = oracle.rti_batch(spec, xs, us, x0d, *data, threads=8)
        qs = s.get_int("qp_status")
        xg, ug = s.get_all("x"), s.get_all("u")
        ok = (qs == 0) & (sts == 0) & (its < spec.opts.qp_iter_max)
        assert ok.mean() >= 0.9, (t, ok.mean())
        e = np.maximum(util.rel_err_per_instance(xg[ok], xs[ok]), util.rel_err_per_instance(ug[ok], us[ok]))
        tmin = s.get("obs_tmin", 0)
        n_active_rows += int((tmin[ok] < 1e-3).sum())
        print("tick %d: converged on both sides %.3f, worst error %.3g, instances with an active obstacle row %d"
              % (t, ok.mean(), e.max() if e.size else 0.0, (tmin[ok] < 1e-3).sum()))
        r = parity_rule.check(oracle, spec, s, ok, e, xin, uin, x0d, data, soft=False)
        assert not r["violations"], (t, r)
        fe.publish(fetch=False)
        s.advance()
    assert n_active_rows > 0, "no instance met an obstacle inside the window: move the starts"
    s.close()


# ---- 13. the mission
def _sweep():
    spec = importlib.util.spec_from_file_location("pf_mission_sweep", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "pf_mission_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# The CPU oracle's own run of the same 64 missions (profiles/pf_moving_oracle.txt: `python tools/pf_mission_oracle.py --batch 64 --ticks 834
# --moving`): missions finished, the slowest finish tick, the smallest clearance.  Never the device's own figures.
ORACLE_FINISHED, ORACLE_SLOWEST, ORACLE_MIN_CLEARANCE = 62, 556, 0.1324


def test_mission_sweep_over_a_moving_world_seeds_0_to_63():
    """examples/pf_mission_sweep.run(moving=True), device-resident, 834 ticks = 1.5 x the oracle's slowest finish.  The margins are those of
    the sweep over a world at rest (tests/test_gpu_pf_frontend.py: 60 against 62 missions, 0.19 against 0.2005 m): two instances at the edge of
    a hard row can fall either way inside the QP's exit-tolerance ball.  yref_writes: the identity of that test - a moving world must not
    change it."""
    ticks = (3 * ORACLE_SLOWEST) // 2
    r = _sweep().run(B=64, ticks=ticks, quiet=True, moving=True)
    ft, mc = r["finish_tick"], r["min_clearance"]
    fin = ft >= 0
    print("finished %d of 64 (oracle %d); finish ticks %s" % (fin.sum(), ORACLE_FINISHED, ft.tolist()))
    print("min clearance %.4f (oracle %.4f): %s" % (mc.min(), ORACLE_MIN_CLEARANCE, np.round(mc, 4).tolist()))
    print("failed solves per tick: total %d; final status %s; waypoint index %s" % (r["failures_per_tick"].sum(), r["final_status"].tolist(),
                                                                                     r["waypoint_index"].tolist()))
    print("yref_writes %d, active at tick 0 %d, switches onto a further segment %d" % (r["yref_writes"], r["active_at_tick_0"], r["new_segments"].sum()))
    assert fin.sum() >= ORACLE_FINISHED - 2
    assert mc.min() >= ORACLE_MIN_CLEARANCE - 0.01
    assert r["yref_writes"] == r["active_at_tick_0"] + r["new_segments"].sum()
    assert r["active_at_tick_0"] == 64 and (r["switches"][fin] == 2).all()


# ---- 14. refusals
def test_refusals():
    B, N, K, L = 8, 6, 4, 5
    E_ARG = -1
    dp = C.POINTER(C.c_double)
    rng = np.random.default_rng(14)
    world, wvel = MR.make_world(B, L, rng)
    wps = np.ascontiguousarray(np.tile(scenario.PF_MISSION_WAYPOINTS.ravel(), (B, 1)))

    def err(s):
        return s._lib.usvmpc_last_error(s._h).decode()

    # another model
    s1 = BatchOcpSolver(usv_models.make_ocp(M1, N * DT, N, 8), B)
    lib = s1._lib
    assert lib.usvmpc_pf_world_vel(s1._h, wvel.ctypes.data_as(dp)) == E_ARG and "usv_model_pf_ca" in err(s1)
    assert lib.usvmpc_pf_world_vel(s1._h, None) == E_ARG and "usv_model_pf_ca" in err(s1)
    assert lib.usvmpc_pf_world_step(s1._h, 0.05) == E_ARG and "usv_model_pf_ca" in err(s1)
    assert lib.usvmpc_pf_world_read(s1._h, None, None) == E_ARG and "usv_model_pf_ca" in err(s1)
    s1.close()
    ocp, s = _solver(B, N, K)
    fe = PathFollowingFrontEnd(s)
    # velocities before a world; a step or a read-back likewise
    assert lib.usvmpc_pf_world_vel(s._h, wvel.ctypes.data_as(dp)) == E_ARG and "no world list yet" in err(s)
    assert lib.usvmpc_pf_world_read(s._h, None, None) == E_ARG and "no world list yet" in err(s)
    fe.reset(scenario.PF_MISSION_WAYPOINTS)
    fe.set_world(world)
    assert lib.usvmpc_pf_world_step(s._h, 0.05) == E_ARG and "at rest" in err(s)
    # NaN / inf
    for bad in (np.nan, np.inf, -np.inf):
        v = wvel.copy()
        v[3, 2, 1] = bad
        assert lib.usvmpc_pf_world_vel(s._h, v.ctypes.data_as(dp)) == E_ARG and "not finite" in err(s)
    with pytest.raises(Exception, match="NaN or infinity"):
        fe.set_world(world, vel=np.full((B, L, 2), np.nan))
    assert np.array_equal(fe.world()[1], np.zeros((B, L, 2)))                        # still at rest
    # the tracks own p, either way round
    s.set("obs_pos", 0, np.zeros((B, K, 2)) + 50.0)
    with pytest.raises(Exception, match="front end owns p"):
        s.set_option("obstacle_tracks", 1)
    ocp, s2 = _solver(B, N, K)
    s2.set_obstacle_tracks(np.zeros((B, K, 2)) + 50.0)
    assert lib.usvmpc_pf_world(s2._h, world.ctypes.data_as(dp), L, 100.0) == 0
    assert lib.usvmpc_pf_world_vel(s2._h, wvel.ctypes.data_as(dp)) == E_ARG and "obstacle_tracks" in err(s2)
    s2.set_option("obstacle_tracks", 0)
    assert lib.usvmpc_pf_world_vel(s2._h, wvel.ctypes.data_as(dp)) == 0              # (no reset yet: the world moves already)
    with pytest.raises(Exception, match="world moves"):
        s2.set_option("obstacle_tracks", 1)
    s2.close()
    # the world moves: every stage; another n_world drops the velocities; the same n_world keeps them
    vel_t, pose_t = np.tile([0.7, 0.0, 0.0], (B, 1)), np.tile([4.0, -4.5, np.pi / 2], (B, 1))
    fe.set_world(world, vel=wvel)
    fe.prepare(vel_t, pose_t)
    p = s.get_all("p")
    assert (p[:, N] != p[:, 0]).any() and (p[:, N] != 0.0).all()
    w2 = world + 0.25
    assert lib.usvmpc_pf_world(s._h, w2.ctypes.data_as(dp), L, 100.0) == 0
    assert np.array_equal(fe.world()[0], w2) and np.array_equal(fe.world()[1], wvel)
    assert lib.usvmpc_pf_world_step(s._h, 0.05) == 0
    w3 = np.ascontiguousarray(world[:, :L - 1])
    assert lib.usvmpc_pf_world(s._h, w3.ctypes.data_as(dp), L - 1, 100.0) == 0
    fe._L = L - 1
    assert np.array_equal(fe.world()[0], w3) and np.array_equal(fe.world()[1], np.zeros((B, L - 1, 2)))
    assert lib.usvmpc_pf_world_step(s._h, 0.05) == E_ARG and "at rest" in err(s)
    # NULL returns to the static behaviour: stage 0 only, "static_obstacles" on
    fe.set_world(world, vel=wvel)
    assert lib.usvmpc_pf_world_vel(s._h, None) == 0
    s.set_all("p", np.full((B, N + 1, 2 * K), -5.0))
    s.set_all("lh", np.full((B, N, K), -6.0))
    fe.prepare(vel_t, pose_t)
    p, lh = s.get_all("p"), s.get_all("lh")
    assert (p[:, 1:] == -5.0).all() and (lh[:, 1:] == -6.0).all() and (p[:, 0] != -5.0).all() and (lh[:, 0] != -6.0).all()
    s.advance()
    assert np.array_equal(fe.world()[0], world)                                      # at rest: advance moves nothing
    s.solve()
    s3 = _solver(B, N, K)[1]                                                         # "static_obstacles" on: stage 0's set on every stage
    s3.set("x0", 0, s.get("x0", 0))
    s3.set_all("yref", s.get_all("yref"))
    s3.set("yref", N, s.get("yref", N))
    s3.set_all("p", np.tile(p[:, :1], (1, N + 1, 1)))
    s3.set_all("lh", np.tile(lh[:, :1], (1, N, 1)))
    s3.solve()
    assert np.array_equal(s3.get_all("x"), s.get_all("x")) and np.array_equal(s3.get_all("u"), s.get_all("u"))
    s.close(), s3.close()
