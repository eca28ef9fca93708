"""The two-layer control stack on a real MI355X (`pytest -m gpu`): guidance.Cascade - guidance layer -> low-level NMPC (usv_model_low_level, in
its generated library) -> 3-DOF vessel; kernels usv_cascade_refs / usv_cascade_step, arithmetic csrc/cascade.hpp - against the CPU oracle
and the numpy restatement of mpc_collisionavoidance_amd/scenario.py.  Shapes: guidance N = 40 / K = 8, low level N = 20 at T = 0.01,
ratio 5."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from mpc_collisionavoidance_amd import scenario, usv_models
from tests import util
from tests.test_cascade import TRIG, ll_workload
from tests.test_gpu_sim import _close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M1, LL = "usv_model_guidance_ca1", "usv_model_low_level"
GN, K, GDT, LN, T, RATIO = 40, 8, 0.05, 20, 0.01, 5
E_ARG = -1
# test_closed_loop_against_the_yardstick: the largest deviation of the device's vessels from the oracle's over 200 low-level ticks, measured
# on an MI355X (positions in m, headings in rad; profiles/cascade_oracle.txt), and the bound: ten times that.  The loop is this sensitive on
# its own: the CPU oracle run twice, the second time with the initial heading and speed moved by 1e-10, ends 5.1e-4 apart (the published
# heading goes through float32 and the QPs' iteration counts change with the last bits)
CLOSED_LOOP_MEASURED = 7.262e-04
CLOSED_LOOP_BOUND = 10 * CLOSED_LOOP_MEASURED


def _oracle_tool():
    spec = importlib.util.spec_from_file_location("cascade_oracle", os.path.join(ROOT, "tools", "cascade_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stack(m, B, wps=None, offset=0, sl=slice(None), c=0.78):
    """(guidance solver, front end, low-level solver, cascade) over instances `sl` of the missions m, reset"""
    from mpc_collisionavoidance_amd import BatchOcpSolver
    from mpc_collisionavoidance_amd.guidance import Cascade, GuidanceFrontEnd
    g = BatchOcpSolver(usv_models.make_ocp(M1, GN * GDT, GN, K), B)
    fe = GuidanceFrontEnd(g)
    ll = BatchOcpSolver(usv_models.make_ocp(LL, LN * T, LN), B)
    assert ll.generated and not g.generated
    pose, vel = m["pose"][sl], np.column_stack([m["vel"][sl], np.zeros(B)])
    fe.reset(m["waypoints"] if wps is None else wps[sl], pose[:, 2])
    fe.set_world(m["world"][sl])
    cas = Cascade(fe, ll, ratio=RATIO, instance_offset=offset, c=c)
    cas.reset(pose, vel)
    return g, fe, ll, cas


def _close_all(*objs):
    for o in objs:
        o.close()


# ------------------------------------------------------------------ 1. the low-level solver against the oracle
def test_low_level_solver_against_the_oracle(oracle):
    from mpc_collisionavoidance_amd import BatchOcpSolver
    tool = _oracle_tool()
    B = 40
    wl = ll_workload(LN, B, np.random.default_rng(6), u_lo=0.2, u_hi=1.4)
    assert (wl["x0"][:, 3] > 1.25).any() and (wl["x0"][:, 3] < 1.25).any()
    spec = tool.low_level_spec(LN, T)
    s = BatchOcpSolver(usv_models.make_ocp(LL, LN * T, LN), B)
    assert s.generated and (s.nx, s.nu, s.K) == (8, 2, 0)
    s.set("x0", 0, wl["x0"]); s.set_all("x", wl["x_init"]); s.set_all("u", wl["u_init"])
    s.set_all("yref", wl["yref"]); s.set("yref", LN, wl["yref_e"])
    xo, uo = wl["x_init"].copy(), wl["u_init"].copy()
    for it in range(4):
        st = s.solve()
        xo, uo, sto, ito = util.oracle_rti(oracle, spec, wl, xo, uo)
        ex, eu = util.rel_err(s.get_all("x"), xo), util.rel_err(s.get_all("u"), uo)
        print("iteration %d: rel_err x %.3e u %.3e, status %s" % (it, ex, eu, np.unique(st)))
        assert np.array_equal(st, sto) and (st == 0).all()
        assert ex < 1e-7 and eu < 1e-7
    s.close()


# ------------------------------------------------------------------ 2. / 3. twelve ticks, everything read back around both kernels
NT, BT, FROZEN = 12, 67, 66


@pytest.fixture(scope="module")
def trace():
    """12 low-level ticks over B = 67 (one full usv_guidance_tick group and a partial one) of make_ca_missions(67, 6, seed=0); instance 66
    flies a mission that is over at the second guidance tick (its set-points freeze at 0, 0).  Per tick: what each kernel read and wrote."""
    m = scenario.make_ca_missions(BT, 6, seed=0)
    wps = np.tile(m["waypoints"][None], (BT, 1, 1))
    wps[FROZEN] = [[4.0, -8.0], [4.0, -5.5], [4.0, -5.6]]
    m["pose"][FROZEN, 0] = 4.2
    g, fe, ll, cas = _stack(m, BT, wps=wps)
    rec, pub = [], None
    for t in range(NT):
        r = dict(guidance=cas.guidance_tick())
        if r["guidance"]:
            fe.prepare(); g.solve_async()
            pub = fe.publish()                                   # (fetched: the set-points usv_cascade_refs is about to read)
        r["heading"], r["speed"], r["active"] = pub["heading"].copy(), pub["speed"].copy(), pub["active"].copy()
        r["before"] = cas.state()
        r["yref_before"], r["yref_e_before"] = ll.get_all("yref"), ll.get("yref", LN)
        cas.refs()
        r["mid"] = cas.state()
        r["ll_x0"], r["yref"], r["yref_e"] = ll.get("x0", 0), ll.get_all("yref"), ll.get("yref", LN)
        ll.solve_async()
        r["x1"], r["ll_status"] = ll.get("x", 1), ll.get_int("status")
        r["gx0_before"] = g.get("x0", 0)
        cas.step()
        r["after"], r["gx0_after"] = cas.state(), g.get("x0", 0)
        rec.append(r)
    _close_all(cas, ll, g)
    return rec


def test_one_step_checks(trace):
    sums = np.zeros((BT, 4))
    for t, r in enumerate(trace):
        assert r["guidance"] == (t % RATIO == 0)
        s0, past0 = r["before"]["state"], r["before"]["past_thrust"]
        # ---- usv_cascade_refs: the low-level x0 and reference rows from what it read
        x0, row = scenario.cascade_ll_inputs(s0, past0, r["heading"], r["speed"])
        for j in (0, 3, 4, 5, 6, 7):
            assert r["ll_x0"][:, j].tobytes() == x0[:, j].tobytes(), (t, j)
        assert np.abs(r["ll_x0"][:, 1:3] - x0[:, 1:3]).max() <= TRIG
        assert r["mid"]["state"].tobytes() == s0.tobytes() and r["mid"]["past_thrust"].tobytes() == past0.tobytes()
        for j in (0, 3):
            assert r["yref_e"][:, j].tobytes() == row[:, j].tobytes(), (t, j)
        assert np.abs(r["yref_e"][:, 1:3] - row[:, 1:3]).max() <= TRIG and (r["yref_e"][:, 4:] == 0.0).all()
        assert (r["yref"][:, :, :8] == r["yref_e"][:, None, :]).all() and (r["yref"][:, :, 8:] == 0.0).all()   # every row is the same row
        assert (r["ll_status"] == 0).all(), t
        # ---- usv_cascade_step: thrusts, errors, one plant period, the hand-over
        thr, past, eu, epsi = scenario.cascade_ll_outputs(r["x1"], r["heading"], r["speed"], s0)
        a = r["after"]
        assert a["thrust"].tobytes() == thr.tobytes() and a["past_thrust"].tobytes() == past.tobytes(), t
        ok, err = _close(a["state"], scenario.cascade_plant_step(s0, thr, T, 1, 0.78))
        assert ok, (t, err)
        eu, epsi = eu.astype(np.float64), epsi.astype(np.float64)
        sums = np.column_stack([sums[:, 0] + np.abs(eu), sums[:, 1] + np.abs(epsi), sums[:, 2] + eu * eu, sums[:, 3] + epsi * epsi])
        assert a["err_sums"].tobytes() == sums.tobytes(), t
        assert (a["ticks"] == t + 1).all()
        gb, ga = r["gx0_before"], r["gx0_after"]
        assert ga[:, 2:5].tobytes() == gb[:, 2:5].tobytes(), t                  # never touched by the cascade
        if (t + 1) % RATIO == 0:
            assert ga[:, [0, 1, 5, 6, 7]].tobytes() == a["state"][:, [3, 4, 0, 1, 2]].tobytes(), t
        else:
            assert ga.tobytes() == gb.tobytes(), t
    assert (trace[0]["speed"] == 0.7).all() and np.abs(trace[-1]["after"]["thrust"]).max() > 0.1


def test_yref_is_rewritten_only_on_change(trace):
    bits = lambda r: np.column_stack([r["heading"].view(np.uint64), r["speed"].view(np.uint64)])
    last, writes = None, 0
    for t, r in enumerate(trace):
        due = np.ones(BT, dtype=bool) if last is None else (bits(r) != last).any(axis=1)
        writes += int(due.sum())
        last = bits(r)
        assert r["before"]["yref_writes"] + int(due.sum()) == r["mid"]["yref_writes"] == r["after"]["yref_writes"] == writes, t
        if t % RATIO:
            assert not due.any(), t
            assert r["yref"].tobytes() == r["yref_before"].tobytes() and r["yref_e"].tobytes() == r["yref_e_before"].tobytes(), t
        else:
            assert due.sum() >= BT - 1, t                                      # the heading moves every guidance tick
            keep = ~due
            assert r["yref"][keep].tobytes() == r["yref_before"][keep].tobytes(), t
    # the frozen instance: active at tick 0, over at tick 5 (set-points 0, 0: a change), untouched at tick 10
    assert trace[0]["active"][FROZEN] == 1 and trace[5]["active"][FROZEN] == 0 and trace[10]["active"][FROZEN] == 0
    assert trace[5]["heading"][FROZEN] == 0.0 and trace[5]["speed"][FROZEN] == 0.0
    row = trace[5]["yref"][FROZEN]
    assert (row[:, [0, 1, 3, 4, 5, 6, 7, 8, 9]] == 0.0).all() and np.abs(row[:, 2] - 1.0).max() <= TRIG   # (0, sin 0, cos 0, 0, 0 ..)
    assert trace[10]["mid"]["yref_writes"] - trace[10]["before"]["yref_writes"] <= BT - 1
    assert trace[10]["yref"][FROZEN].tobytes() == trace[9]["yref"][FROZEN].tobytes()


# ------------------------------------------------------------------ 4. a mission that ends
def test_a_mission_that_ends():
    B = 8
    m = scenario.make_ca_missions(B, 6, seed=0)
    m["waypoints"] = np.array([[4.0, -5.0], [4.0, -3.5]])
    g, fe, ll, cas = _stack(m, B)
    stopped_at = np.full(B, -1)
    u_stop = np.zeros(B)
    for period in range(160):
        cas.tick()                                               # the guidance tick of this period
        out = fe.publish()                                       # (the same set-points again, fetched)
        stop = out["speed"] == 0.0
        for i in range(RATIO - 1):
            cas.tick()
            if i == 0:
                st = cas.state()
                x1 = ll.get("x", 1)
                assert (st["thrust"][stop] == 0.0).all() and st["past_thrust"][stop].tobytes() == x1[stop, 6:8].tobytes(), period
                assert st["thrust"][~stop].tobytes() == x1[~stop, 6:8].tobytes(), period
        new = stop & (stopped_at < 0)
        st = cas.state()
        stopped_at[new], u_stop[new] = period, st["state"][new, 3]
        if new.any():
            d = np.hypot(st["state"][new, 0] - 4.0, st["state"][new, 1] + 3.5)
            assert (d < 1.0).all(), d
        if (stopped_at >= 0).all() and period >= stopped_at.max() + 20:
            break
    assert (stopped_at >= 0).all(), stopped_at
    assert (out["active"] == 0).all() and (out["speed"] == 0.0).all()
    st = cas.state()
    assert (u_stop > 0.3).all() and (st["state"][:, 3] < 0.8 * u_stop).all(), (u_stop, st["state"][:, 3])   # u decays
    assert np.abs(st["past_thrust"]).max() > 0.0                                                             # past_T still follows x1
    assert (fe.mission_state()["finish_tick"] >= 0).all()
    _close_all(cas, ll, g)


# ------------------------------------------------------------------ 5. closed loop against the yardstick
def test_closed_loop_against_the_yardstick(oracle):
    """Device and oracle solves agree only to the parity tolerance and the loop feeds the difference back: the bound is ten times the
    largest deviation measured on an MI355X (CLOSED_LOOP_MEASURED; recorded in profiles/cascade_oracle.txt)."""
    B, GT = 8, 40
    tool = _oracle_tool()
    m = scenario.make_ca_missions(B, 6, seed=0)
    ref = tool.run(m, GT, N=GN, K=K, dt=GDT, ll_N=LN, ratio=RATIO, record=True)
    assert ref["guidance_failures"] == 0 and ref["low_level_failures"] == 0
    g, fe, ll, cas = _stack(m, B)
    states = [cas.state()["state"]]
    gfail = lfail = 0
    for t in range(GT * RATIO):
        cas.tick()
        states.append(cas.state()["state"])
        lfail += int((ll.get_int("status") != 0).sum())
        if t % RATIO == 0:
            gfail += int((g.get_int("status") != 0).sum())
    states = np.array(states)
    dev = np.abs(states[:, :, :3] - ref["states"][:, :, :3]).max()
    print("closed loop: largest deviation of (nedx, nedy, psi) from the oracle over %d low-level ticks: %.3e; of (u, v, r): %.3e; travelled %.2f m"
          % (GT * RATIO, dev, np.abs(states[:, :, 3:] - ref["states"][:, :, 3:]).max(), np.hypot(*(states[-1, :, :2] - states[0, :, :2]).T).min()))
    assert gfail == 0 and lfail == 0
    assert np.hypot(*(states[-1, :, :2] - states[0, :, :2]).T).min() > 0.8      # (the vessels are under way: 2 s at up to 0.7 m/s)
    assert CLOSED_LOOP_BOUND is not None, "no bound recorded yet: measured deviation %.3e" % dev
    assert dev <= CLOSED_LOOP_BOUND, (dev, CLOSED_LOOP_BOUND)
    _close_all(cas, ll, g)


# ------------------------------------------------------------------ 6. disturbance and shards
def test_disturbance_and_shards():
    B, H, NTK, SIG = 64, 32, 10, 1e-3
    m = scenario.make_ca_missions(B, 6, seed=0)
    runs = []
    for sl, off in ((slice(0, B), 0), (slice(0, H), 0), (slice(H, B), H)):
        n = sl.stop - sl.start
        g, fe, ll, cas = _stack(m, n, offset=off, sl=sl)
        first = cas.state()
        out = []
        for t in range(NTK):
            cas.tick(SIG, 100 + t)
            out.append(cas.state())
        runs.append((first, out))
        _close_all(cas, ll, g)
    whole, a, b = (r[1] for r in runs)
    for t in range(NTK):
        assert np.concatenate([a[t]["state"], b[t]["state"]]).tobytes() == whole[t]["state"].tobytes(), t
    # sigma lands on (u, v, r) only: after the first tick position and heading are the undisturbed plant period's
    s0, s1 = runs[0][0]["state"], whole[0]["state"]
    want = scenario.cascade_plant_step(s0, whole[0]["thrust"], T, 1, 0.78)
    ok, err = _close(s1[:, :3], want[:, :3])
    assert ok, err
    d = s1[:, 3:] - want[:, 3:]
    assert (np.abs(d) > 1e-9).all() and np.abs(d).max() < 6 * SIG and 0.7 * SIG < d.std() < 1.3 * SIG, (np.abs(d).max(), d.std())


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    from mpc_collisionavoidance_amd import BatchOcpSolver
    from mpc_collisionavoidance_amd.guidance import Cascade, GuidanceFrontEnd
    B = 8
    m = scenario.make_ca_missions(B, 6, seed=0)
    ll = BatchOcpSolver(usv_models.make_ocp(LL, LN * T, LN), B)
    ptrs = [C.c_void_p(ll.device_ptr(f)) for f in ("x0", "x", "yref", "yref_e")]
    g = BatchOcpSolver(usv_models.make_ocp(M1, GN * GDT, GN, K), B)
    fe = GuidanceFrontEnd(g)
    lib = g._lib

    def refused(h, word, ratio=RATIO, Tt=T, steps=1, c=0.78, off=0, batch=B, N=LN, p=ptrs):
        out = C.c_void_p()
        rc = lib.usvmpc_cascade_create(h, ratio, Tt, steps, c, off, batch, N, *p, C.byref(out))
        msg = lib.usvmpc_cascade_last_error(None).decode()
        assert rc == E_ARG and out.value is None and word in msg, (rc, msg)

    pf = BatchOcpSolver(usv_models.make_ocp("usv_model_pf_ca", 20 * 0.01, 20, 4), B)
    refused(pf._h, M1)                                           # another guidance model
    pf.close()
    refused(g._h, "usvmpc_guidance_reset")                       # no reset yet
    fe.reset(m["waypoints"], m["pose"][:, 2])
    refused(g._h, "usvmpc_guidance_world")                       # no world yet
    fe.set_world(m["world"])
    x0 = g.get("x0", 0)
    refused(g._h, "shooting interval", ratio=4)                  # ratio * T is not the guidance dt
    refused(g._h, "shooting interval", Tt=0.02)
    refused(g._h, "ratio >= 1", ratio=0)
    refused(g._h, "finite", Tt=float("nan"))
    refused(g._h, "finite", c=float("inf"))
    for i in range(4):
        refused(g._h, "null device pointer", p=ptrs[:i] + [C.c_void_p(None)] + ptrs[i + 1:])
    refused(g._h, "batch", batch=B + 1)
    assert g.get("x0", 0).tobytes() == x0.tobytes()              # nothing changed
    ll2 = BatchOcpSolver(usv_models.make_ocp(LL, LN * T, LN), B + 1)
    with pytest.raises(Exception, match="same batch"):
        Cascade(fe, ll2)
    with pytest.raises(Exception, match="usv_model_low_level"):
        Cascade(fe, g)
    ll2.close()
    cas = Cascade(fe, ll, ratio=RATIO)                           # ... and the accepted call
    with pytest.raises(Exception, match="usvmpc_cascade_reset"):
        cas.refs()
    with pytest.raises(Exception, match="usvmpc_cascade_reset"):
        cas.step()
    cas.reset(m["pose"], np.column_stack([m["vel"], np.zeros(B)]))
    cas.tick()
    assert (cas.state()["ticks"] == 1).all()
    _close_all(cas, ll, g)


# ------------------------------------------------------------------ a moving guidance world follows the guidance periods
@pytest.mark.parametrize("follow", [1, 0])
def test_moving_world_moves_once_per_guidance_period(follow):
    B = 8
    m = scenario.make_ca_missions(B, 6, seed=0, moving=True)
    g, fe, ll, cas = _stack(m, B)
    fe.set_world(m["world"], vel=m["world_vel"])                  # (after the cascade exists: the step looks the world up at every call)
    g.set_option("obstacle_step_on_advance", follow)
    w = m["world"].copy()
    for t in range(2 * RATIO + 1):
        cas.tick()
        if follow and (t + 1) % RATIO == 0:
            w[:, :, :2] = w[:, :, :2] + (RATIO * T) * m["world_vel"]
        got, vel = fe.world()
        assert got.tobytes() == w.tobytes(), t
        assert vel.tobytes() == m["world_vel"].tobytes()
    assert (g.get_int("status") == 0).all() and (ll.get_int("status") == 0).all()
    _close_all(cas, ll, g)
