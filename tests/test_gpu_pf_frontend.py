"""The path-following front end of usv_model_pf_ca on a real MI355X (`pytest -m gpu`): kernels usv_pf_prepare / usv_pf_publish
(csrc/pf_guidance.hpp) through the C ABI usvmpc_pf_* and guidance.PathFollowingFrontEnd.

* host-fed, against the numpy restatement of the node (tests/pf_frontend_ref.py) over the scripted sequences of tests/test_pf_frontend.py:
  exact wherever no sin / cos / atan2 enters, 1e-12 absolute otherwise; also on a single-instance handle (host mirror on);
* device-resident == host-fed, bit for bit, in a disturbed closed loop;
* the rule that rewrites an instance's yref only when its (sin ak, cos ak, u_des) changes, counted by the device;
* static obstacles == stage 0 replicated over the stages;
* the inputs the front end hands the solver, run through the CPU oracle, under the project's parity rule, with active obstacle rows;
* the mission sweep of examples/pf_mission_sweep.py, seeds 0 .. 63;
* refusals.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from mpc_collisionavoidance_amd import BatchOcpSolver, scenario, usv_models
from mpc_collisionavoidance_amd.guidance import PathFollowingFrontEnd
from tests import parity_rule, util
from tests import pf_frontend_ref as R

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


def _world(B, L, rng):
    w = np.concatenate([rng.uniform(-2.0, 10.0, (B, L, 1)), rng.uniform(-8.0, 8.0, (B, L, 1)), rng.uniform(0.1, 0.6, (B, L, 1))], axis=2)
    if L >= 3:
        w[:, 2, :2] += 30.0        # never visible at max_radius 12
    return w


def _inputs(s):
    return dict(x0=s.get("x0", 0), yref=s.get_all("yref"), yref_e=s.get("yref", s.N), p0=s.get_all("p")[:, 0], lh0=s.get_all("lh")[:, 0])


# ---- 6. host-fed against the numpy restatement
@pytest.mark.parametrize("B,L,classes", [(70, 0, None), (70, 3, None), (70, 9, None), (1, 3, [3]), (1, 9, [2])])
def test_host_fed_front_end_is_the_nodes_arithmetic(B, L, classes):
    N, K, T = 6, 4, 12
    rng = np.random.default_rng(60 + L)
    wps, vel, pose = R.scripted_sequence(B, T, classes=classes)
    world = _world(B, L, rng)
    ocp, s = _solver(B, N, K)
    fe = PathFollowingFrontEnd(s)
    fe.reset(wps)
    fe.set_world(world, max_radius=12.0)
    ref = R.PfRef(B, N, K)
    ref.x0[:] = GENERIC
    ref.reset(wps)
    ref.set_world(world, 12.0)
    assert fe.state()["min_clearance"].tolist() == [1e300] * B and fe.state()["finish_tick"].tolist() == [-1] * B
    seen = set()
    for t in range(T):
        fe.prepare(vel[t], pose[t])
        ref.prepare(vel[t], pose[t])
        got = _inputs(s)
        st = fe.state()
        got.update(k=st["wp_index"], finish_tick=st["finish_tick"], min_clearance=st["min_clearance"])
        R.check(ref, got, "B %d L %d tick %d (prepare)" % (B, L, t))
        assert st["yref_writes"] == ref.yref_writes, (t, st["yref_writes"], ref.yref_writes)
        s.solve()
        x1 = s.get("x", 1)
        out = fe.publish()
        ref.publish(x1)
        R.check(ref, dict(out=out), "B %d L %d tick %d (publish)" % (B, L, t))
        seen |= set(ref.phase.tolist())
    assert seen == {R.OVER, R.ACTIVE, R.SWITCH} or classes == [2]
    # the obstacle stages beyond 0 are not the front end's: static mode reads stage 0 only
    s.close()


# ---- 7. device-resident == host-fed
def test_device_resident_equals_host_fed_bit_for_bit():
    """No instance switches inside the window: on a switch tick the node keeps its past thrust while the plant state moves on, so the two
    modes are DEFINED to differ on the tick after (host-fed: past thrust of the last published tick; device-resident: x0[12..13])."""
    B, N, K, L, T = 70, 6, 4, 3, 10
    rng = np.random.default_rng(7)
    x0 = np.tile(GENERIC, (B, 1))
    x0[:, 10] += rng.uniform(-0.5, 0.5, B)
    x0[:, 11] += rng.uniform(-0.3, 0.3, B)
    x0[:, 0] += rng.uniform(-0.2, 0.2, B)
    x0[:, 4] = rng.uniform(-0.02, 0.02, B)
    world = np.concatenate([4.0 + rng.uniform(-2.5, 2.5, (B, L, 1)), rng.uniform(-4.0, 0.0, (B, L, 1)), rng.uniform(0.1, 0.3, (B, L, 1))], axis=2)
    far = np.abs(world[:, :, 0] - 4.0) < 1.6
    world[:, :, 0] = np.where(far, 4.0 + np.sign(world[:, :, 0] - 4.0 + 1e-30) * 1.6, world[:, :, 0])   # beside the leg, not on it
    wps = scenario.PF_MISSION_WAYPOINTS
    hs = []
    for _ in range(2):
        ocp, s = _solver(B, N, K, x0)
        s.set_option("disturbance_mask", (1 << 3) | (1 << 5))
        fe = PathFollowingFrontEnd(s)
        fe.reset(wps)
        fe.set_world(world)
        hs.append((s, fe))
    (sa, fa), (sb, fb) = hs
    for t in range(T):
        fa.prepare()
        xb = sb.get("x0", 0)
        fb.prepare(xb[:, 3:6], xb[:, [10, 11, 0]])
        for f in ("x0", "yref", "p", "lh"):
            a, b = (sa.get("x0", 0), sb.get("x0", 0)) if f == "x0" else (sa.get_all(f), sb.get_all(f))
            assert np.array_equal(a, b), (t, f)
        sa.solve(), sb.solve()
        assert np.array_equal(sa.get_all("x"), sb.get_all("x")) and np.array_equal(sa.get_all("u"), sb.get_all("u")), t
        oa, ob = fa.publish(), fb.publish()
        for nm in oa:
            assert np.array_equal(oa[nm], ob[nm]), (t, nm)
        assert oa["active"].all()
        sa.advance(1e-3, 100 + t), sb.advance(1e-3, 100 + t)
    assert np.array_equal(sa.get("x0", 0), sb.get("x0", 0))
    sta, stb = fa.state(), fb.state()
    assert sta["yref_writes"] == stb["yref_writes"] == B and np.array_equal(sta["min_clearance"], stb["min_clearance"])
    assert (sta["min_clearance"] < 1e300).all()
    sa.close(), sb.close()


# ---- 8. the yref rule on the device
def test_yref_is_rewritten_only_when_its_triple_changes():
    B, N, K, T = 70, 6, 4, 8
    classes = [0] * 30 + [2] * 30 + [3] * 10       # cruising | switch at tick 3 | switch at ticks 0 and 2, over from tick 3
    cls = np.array(classes)
    wps, vel, pose = R.scripted_sequence(B, T, classes=classes)
    ocp, s = _solver(B, N, K)
    fe = PathFollowingFrontEnd(s)
    fe.reset(wps)
    fe.set_world(None)
    writes, act = [], []
    ak_sin = {}
    for t in range(6):
        fe.prepare(vel[t], pose[t])
        writes.append(fe.state()["yref_writes"])
        act.append(fe.publish()["active"].copy())
        ak_sin[t] = s.get_all("yref")[:, 0, 1].copy()
    assert writes[0] == act[0].sum() == 60                     # the first prepare: every active instance
    assert writes[1] == 70                                     # class 3, the tick after its switch tick: one each
    assert writes[2] == 70 and writes[3] == 70                 # unchanged segments (poses and speeds differ every tick); switch ticks write nothing
    assert not act[3][cls == 2].any() and not act[3][cls == 3].any()
    assert writes[4] == 100                                    # class 2, the tick after its switch tick: exactly one each
    assert writes[5] == 100
    assert not np.array_equal(ak_sin[4][cls == 2], ak_sin[2][cls == 2]) and np.array_equal(ak_sin[4][cls == 0], ak_sin[0][cls == 0])
    # a caller write of yref: the next prepare restores every active instance's rows exactly; inactive ones keep what the caller wrote
    before, before_e = s.get_all("yref"), s.get("yref", N)
    garbage = np.random.default_rng(1).uniform(-9.0, 9.0, before.shape)
    s.set_all("yref", garbage)
    fe.prepare(vel[6], pose[6])
    active = fe.publish()["active"] != 0
    assert active.sum() == 60 and not active[cls == 3].any()
    after = s.get_all("yref")
    assert np.array_equal(after[active], before[active]) and np.array_equal(after[~active], garbage[~active])
    assert np.array_equal(s.get("yref", N), before_e)
    assert fe.state()["yref_writes"] == 160
    fe.prepare(vel[7], pose[7])
    assert fe.state()["yref_writes"] == 160
    # the terminal reference counts as yref too (set through stage N)
    s.set("yref", N, garbage[:, 0, :14])
    fe.prepare(vel[7], pose[7])
    assert fe.state()["yref_writes"] == 220 and np.array_equal(s.get("yref", N)[active], before_e[active])
    s.close()


# ---- 9. static mode == replicated stages
def test_static_obstacles_equal_replicated_stages():
    B, N, K, L = 70, 6, 4, 9
    rng = np.random.default_rng(9)
    wps, vel, pose = R.scripted_sequence(B, 2)
    world = _world(B, L, rng)
    world[:, :, 0] = np.where(np.abs(world[:, :, 0] - pose[1, :, None, 0]) < 2.0, world[:, :, 0] + 4.0, world[:, :, 0])   # not on top of the vessel
    ocp, s = _solver(B, N, K)
    fe = PathFollowingFrontEnd(s)
    fe.reset(wps)
    fe.set_world(world, max_radius=12.0)
    fe.prepare(vel[1], pose[1])
    x0, yref, yref_e, p, lh = s.get("x0", 0), s.get_all("yref"), s.get("yref", N), s.get_all("p"), s.get_all("lh")
    assert (p[:, 0] != 1000.0).any()
    s.solve()
    ocp2, s2 = _solver(B, N, K)
    s2.set("x0", 0, x0)
    s2.set_all("yref", yref)
    s2.set("yref", N, yref_e)
    s2.set_all("p", np.tile(p[:, :1], (1, N + 1, 1)))
    s2.set_all("lh", np.tile(lh[:, :1], (1, N, 1)))
    s2.solve()
    assert np.array_equal(s2.get_all("x"), s.get_all("x")) and np.array_equal(s2.get_all("u"), s.get_all("u"))
    s.close(), s2.close()


# ---- 10. what the front end feeds the solver, through the oracle
def pf_parity_starts(B, seed=0):
    """Generator instances started 1 .. 3 m short of the nearer obstacle of leg 1 (measured along the leg), on the leg, heading along it at
    0.7 m/s."""
    m = scenario.make_pf_missions(B, seed)
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
    fe.set_world(m["world"], max_radius=cfg["max_radius"], margin=cfg["margin"])
    spec = oracle.spec(util.MODEL_ID[M2], N, N * DT, K, sim_steps=STEPS)
    n_active_rows = 0
    for t in range(T):
        fe.prepare()
        xin, uin = s.get_all("x"), s.get_all("u")
        x0d, p, lh = s.get("x0", 0), s.get_all("p"), s.get_all("lh")
        data = (s.get_all("yref"), s.get("yref", N), np.tile(p[:, :1], (1, N + 1, 1)), np.tile(lh[:, :1], (1, N, 1)))
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


# ---- 11. the mission
def _sweep():
    spec = importlib.util.spec_from_file_location("pf_mission_sweep", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "pf_mission_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mission_sweep_seeds_0_to_63():
    """examples/pf_mission_sweep.run, device-resident, 560 ticks = 1.5 x the CPU oracle's slowest finish (373).  The oracle alone (numpy
    front end, seeds 0 .. 63): 62 of 64 finish at ticks 317 .. 373, smallest clearance 0.2005 m.
    yref_writes: the issue words it "active-at-tick-0 + number of switches observed"; the switch that ends a mission is followed by no
    active tick and, by the front end's own rule, by no write - so the count here is the switches ONTO a further segment (run():
    new_segments), which for a finished two-leg mission is one of its two switches."""
    r = _sweep().run(B=64, ticks=560, quiet=True)
    ft, mc = r["finish_tick"], r["min_clearance"]
    fin = ft >= 0
    print("finished %d of 64; finish ticks %s" % (fin.sum(), ft.tolist()))
    print("min clearance %s" % np.round(mc, 4).tolist())
    print("failed solves per tick: total %d; final status %s; waypoint index %s" % (r["failures_per_tick"].sum(), r["final_status"].tolist(),
                                                                                     r["waypoint_index"].tolist()))
    print("yref_writes %d, active at tick 0 %d, switches onto a further segment %d" % (r["yref_writes"], r["active_at_tick_0"], r["new_segments"].sum()))
    assert fin.sum() >= 60
    assert (ft[fin] >= 300).all()
    assert (mc >= 0.19).all()
    assert (mc < 1.2).all()
    assert r["yref_writes"] == r["active_at_tick_0"] + r["new_segments"].sum()
    assert r["active_at_tick_0"] == 64 and (r["switches"][fin] == 2).all()


# ---- 12. refusals
def test_refusals():
    B, N, K = 8, 6, 4
    E_ARG = -1
    wps = np.ascontiguousarray(np.tile(scenario.PF_MISSION_WAYPOINTS.ravel(), (B, 1)))
    dp = C.POINTER(C.c_double)
    zeros = np.zeros((B, 3))

    def err(s):
        return s._lib.usvmpc_last_error(s._h).decode()

    # another model
    s1 = BatchOcpSolver(usv_models.make_ocp(M1, N * DT, N, 8), B)
    L = s1._lib
    assert L.usvmpc_pf_reset(s1._h, wps.ctypes.data_as(dp), 3) == E_ARG and "usv_model_pf_ca" in err(s1)
    assert L.usvmpc_pf_prepare(s1._h, None, None) == E_ARG and "usv_model_pf_ca" in err(s1)
    assert L.usvmpc_pf_world(s1._h, None, 0, 100.0) == E_ARG and L.usvmpc_pf_publish(s1._h, *([None] * 8)) == E_ARG
    assert L.usvmpc_pf_state(s1._h, None, None, None, None) == E_ARG
    with pytest.raises(Exception, match="belongs to usv_model_pf_ca"):
        PathFollowingFrontEnd(s1)
    s1.close()
    ocp, s = _solver(B, N, K)
    # prepare / publish / state before reset
    assert L.usvmpc_pf_prepare(s._h, None, None) == E_ARG and "usvmpc_pf_reset" in err(s)
    assert L.usvmpc_pf_prepare(s._h, zeros.ctypes.data_as(dp), zeros.ctypes.data_as(dp)) == E_ARG
    assert L.usvmpc_pf_publish(s._h, *([None] * 8)) == E_ARG and L.usvmpc_pf_state(s._h, None, None, None, None) == E_ARG
    # too many obstacles, too few waypoints
    w65 = np.zeros((B, 65, 3))
    assert L.usvmpc_pf_world(s._h, w65.ctypes.data_as(dp), 65, 100.0) == E_ARG and "n_world" in err(s)
    assert L.usvmpc_pf_world(s._h, None, -1, 100.0) == E_ARG
    assert L.usvmpc_pf_reset(s._h, wps.ctypes.data_as(dp), 1) == E_ARG and "two" in err(s)
    # the tracks own p
    s.set_obstacle_tracks(np.zeros((B, K, 2)) + 50.0)
    assert L.usvmpc_pf_reset(s._h, wps.ctypes.data_as(dp), 3) == E_ARG and "obstacle_tracks" in err(s)
    s.set_option("obstacle_tracks", 0)
    assert L.usvmpc_pf_reset(s._h, wps.ctypes.data_as(dp), 3) == 0
    with pytest.raises(Exception, match="front end owns p"):
        s.set_option("obstacle_tracks", 1)
    # one array without the other
    assert L.usvmpc_pf_prepare(s._h, zeros.ctypes.data_as(dp), None) == E_ARG and "both" in err(s)
    assert L.usvmpc_pf_prepare(s._h, None, None) == 0
    s.sync()
    s.close()
