"""The objective value on a real MI355X (`pytest -m gpu`): kernels usv_cost_eval and usv_cost_track through the C ABI (usvmpc_get "cost" /
"cost_stage" / "cost_parts", usvmpc_eval_cost, usvmpc_cost_track / _tracked) and BatchOcpSolver.get_cost / eval_cost / track_cost /
tracked_cost, AcadosOcpSolver.get_cost (include/usvmpc.h, "Objective value").

The yardstick is the numpy restatement of tests/cost_numpy.py (loops over i and j in Python, vectorised over instances only) on the arrays
the host reads back - get_all of x, u, yref, sl, su - and the comparison is always bit for bit: csrc/cost_eval.hpp rounds every operation on
its own and fixes the order of every sum.  The shapes are those of tests/test_gpu_closed_loop_log.py: N = 6, B = 70 (seven stages per
instance: the second wave pass of an instance has an idle 16-lane row, and the last workgroup two idle waves), 5 RK4 steps for
usv_model_pf_ca."""
import ctypes as C

import numpy as np
import pytest

from mpc_collisionavoidance_amd import AcadosOcpSolver, AcadosSim, BatchOcpSolver, BatchSimSolver, scenario, usv_models
from tests import cost_numpy as cn

pytestmark = pytest.mark.gpu

M0, M1, M2 = "usv_model", "usv_model_guidance_ca1", "usv_model_pf_ca"
SOFT = {M0: False, M1: True, M2: False}
DT, STEPS = 0.05, 5
GENERIC = np.array([np.pi / 2, 1.0, 0.0, 0.7, 0.0, 0.0, 0.0, 4.0, -5.0, np.pi / 2, 4.0, -4.5, 0.0, 0.0])
E_ARG, E_FIELD, E_SIZE = -1, -2, -4
B0, N0 = 70, 6
_dp = C.POINTER(C.c_double)


def _solver(B, N, K=4, x0=None):
    ocp = usv_models.make_ocp(M2, N * DT, N, K)
    ocp.solver_options.sim_method_num_steps = STEPS
    s = BatchOcpSolver(ocp, B)
    x0 = np.tile(GENERIC, (B, 1)) if x0 is None else x0
    s.set("x0", 0, x0)
    s.set_all("x", np.tile(x0[:, None, :], (1, N + 1, 1)))
    s.set_all("u", np.zeros((B, N, 2)))
    yr = np.zeros(16)
    yr[1], yr[2], yr[3] = 1.0, 0.0, 0.7     # (a reference the state is not at: the cost is not zero)
    s.set_all("yref", np.tile(yr, (B, N, 1)))
    s.set("yref", N, np.tile(yr[:14], (B, 1)))
    return ocp, s


def _x0(B):
    rng = np.random.default_rng(33)
    x0 = np.tile(GENERIC, (B, 1))
    x0[:, 0] += rng.uniform(-0.2, 0.2, B)
    x0[:, 3] += rng.uniform(-0.1, 0.1, B)
    x0[:, 4] = rng.uniform(-0.02, 0.02, B)
    x0[:, 6] = rng.uniform(-0.3, 0.3, B)
    x0[:, 10] += rng.uniform(-0.5, 0.5, B)
    return x0


def _scenario_solver(name, N, K, B, seed=5, wl=None, ocp=None):
    ocp = ocp or usv_models.make_ocp(name, N * scenario.DT[name], N, K or None)
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, wl or scenario.make_batch(name, N, K, B, seed=seed))
    s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
    return ocp, s


def _slice(wl, a, b):
    return {k: (v[a:b] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == wl["x0"].shape[0] else v) for k, v in wl.items()}


def _want(ocp, s, name):
    """the numpy restatement on what the host reads back"""
    tab = cn.tab_of_ocp(ocp, s.K, SOFT[name])
    K = s.K
    sl = s.get_all("sl") if K else np.zeros((s.B, s.N, 0))
    su = s.get_all("su") if K else np.zeros((s.B, s.N, 0))
    return cn.evaluate(tab, s.dt, s.get_all("x"), s.get_all("u"), s.get_all("yref"), s.get("yref", s.N), sl, su)


def _check_all(ocp, s, name, stage=3):
    wc, wcost, wparts = _want(ocp, s, name)
    cost = s.get_cost()
    assert cost.shape == (s.B,) and cn.same_bits(cost, wcost), np.abs(cost - wcost).max()
    assert cn.same_bits(s.get("cost_stage", -1), wc)
    assert cn.same_bits(s.get("cost_stage", stage), wc[:, stage]) and cn.same_bits(s.get("cost_stage", s.N), wc[:, s.N])
    assert cn.same_bits(s.get("cost_parts", 0), wparts)
    return wc, wcost, wparts


def _err(s):
    return s._lib.usvmpc_last_error(s._h).decode()


# ---- 1. solved iterates, three models
def _fresh(name, K, a=0, b=B0):
    """instances a .. b - 1 of the B0-instance workload of `name`, on a handle of their own"""
    if name == M2:
        return _solver(b - a, N0, K, _x0(B0)[a:b])
    return _scenario_solver(name, N0, K, b - a, wl=_slice(scenario.make_batch(name, N0, K, B0, seed=5), a, b))


def _copy_inputs(dst, src):
    dst.set("x0", 0, src.get("x0", 0))
    for f in ("x", "u", "yref") + (("p", "lh") if src.K else ()):
        dst.set_all(f, src.get_all(f))
    dst.set("yref", src.N, src.get("yref", src.N))


@pytest.mark.parametrize("name,K", [(M0, 0), (M1, 3), (M2, 4)])
def test_solved_iterates_equal_the_numpy_restatement(name, K):
    ocp, s = _fresh(name, K)
    for _ in range(2):
        s.solve()
    wc, wcost, wparts = _check_all(ocp, s, name)
    # (a soft handle's slacks may be negative - the formula has no clamp - and so may its cost)
    assert np.isfinite(wcost).all() and (wcost != 0).all() and (wcost[0] != wcost[1:]).any() and (wparts[:, 0] > 0).all()
    if not SOFT[name]:
        assert cn.same_bits(wparts[:, 2], np.zeros(B0)) and (wcost > 0).all()
    # AcadosOcpSolver.get_cost(): a float, element 0 of a one-instance batch (and an instance's cost does not depend on its batch)
    ocp1, one = _fresh(name, K, 0, 1)
    acados = AcadosOcpSolver(ocp1)
    _copy_inputs(acados._b, one)
    for _ in range(2):
        one.solve()
        acados.solve()
    c = acados.get_cost()
    assert isinstance(c, float) and cn.same_bits(np.array([c]), one.get_cost())
    assert cn.same_bits(one.get_cost(), wcost[:1])
    s.close(), one.close()


# ---- 2. general tables, no solve: dense random W, Vx, Vu, W_e; x, u, yref set by the caller; slacks 0.  Also the pending-writes flush
# of a small handle (B = 3 keeps a host mirror: the sets below are still in it when the evaluation is enqueued)
@pytest.mark.parametrize("name,K,B", [(M0, 0, 3), (M1, 3, 70), (M2, 4, 70)])
def test_general_tables_without_a_solve(name, K, B):
    rng = np.random.default_rng(17)
    ocp = usv_models.make_ocp(name, N0 * scenario.DT[name], N0, K or None)
    nx, nu = np.asarray(ocp.cost.Vx).shape[1], np.asarray(ocp.cost.Vu).shape[1]
    ny = nx + nu
    A, Ae = rng.normal(size=(ny, ny)), rng.normal(size=(nx, nx))
    ocp.cost.W, ocp.cost.W_e = A @ A.T, Ae @ Ae.T
    ocp.cost.Vx, ocp.cost.Vu = rng.normal(size=(ny, nx)), rng.normal(size=(ny, nu))
    s = BatchOcpSolver(ocp, B)
    x, u = rng.normal(size=(B, N0 + 1, nx)), rng.normal(size=(B, N0, nu))
    yref, yref_e = rng.normal(size=(B, N0, ny)), rng.normal(size=(B, nx))
    s.set_all("x", x), s.set_all("u", u), s.set_all("yref", yref), s.set("yref", N0, yref_e)
    tab = cn.tab_of_ocp(ocp, K, SOFT[name])
    zero = np.zeros((B, N0, K))
    wc, wcost, wparts = cn.evaluate(tab, s.dt, x, u, yref, yref_e, zero, zero)
    assert cn.same_bits(s.get_cost(), wcost) and cn.same_bits(s.get("cost_stage", -1), wc) and cn.same_bits(s.get("cost_parts", 0), wparts)
    assert cn.same_bits(wparts[:, 2], np.zeros(B))
    # one stage set anew (on a small multi-instance handle: a strided row, remembered per stage): the next get sees it
    x[:, 2] = rng.normal(size=(B, nx))
    s.set("x", 2, x[:, 2])
    wc2, wcost2, _ = cn.evaluate(tab, s.dt, x, u, yref, yref_e, zero, zero)
    assert cn.same_bits(s.get_cost(), wcost2) and cn.same_bits(s.get("cost_stage", 2), wc2[:, 2]) and not cn.same_bits(wc2[:, 2], wc[:, 2])
    # a NaN stays in its instance
    x[1, 4, 0] = np.nan
    s.set_all("x", x)
    got = s.get_cost()
    assert np.isnan(got[1]) and cn.same_bits(np.delete(got, 1), np.delete(wcost2, 1))
    s.close()


# ---- 3. two obstacle chunks and live slacks: usv_model_guidance_ca1 with K = 20, the vessel inside soft keep-out circles of both chunks
def test_two_obstacle_chunks_with_live_slacks():
    K = 20
    ocp = usv_models.make_ocp(M1, N0 * DT, N0, K)
    ocp.cost.Zl, ocp.cost.Zu = 0.5 * np.ones(K), 0.25 * np.ones(K)    # (the quadratic penalties enter too)
    # (the registry OCP lets a slack go down to -0.2, where every idle row's then rests and pays a negative share; with the bound at 0 the
    # slack share of the cost is what the two live rows pay)
    ocp.constraints.lsh = np.zeros(K)
    wl = scenario.make_batch(M1, N0, K, B0, seed=5)
    for i in (2, 17):    # a circle of radius 1 around a point 0.3 m from every other vessel, in every stage: it cannot be left in 0.3 s
        wl["p"][::2, :, 2 * i] = wl["x0"][::2, None, 5] + 0.3
        wl["p"][::2, :, 2 * i + 1] = wl["x0"][::2, None, 6]
        wl["lh"][::2, :, i] = 1.0
    _, s = _scenario_solver(M1, N0, K, B0, wl=wl, ocp=ocp)
    for _ in range(2):
        s.solve()
    sl = s.get_all("sl")
    assert (sl[:, :, 2] != 0).any() and (sl[:, :, 17] != 0).any(), "no live slack: the scenario does not exercise the slack terms"
    wc, wcost, wparts = _check_all(ocp, s, M1)
    assert (wparts[:, 2] > 0).any() and np.isfinite(wcost).all()
    s.close()


# ---- 4. the asynchronous path
def test_eval_cost_behind_solve_async():
    from mpc_collisionavoidance_amd import sharding
    ocp, s = _scenario_solver(M1, N0, 3, B0)
    s.solve()
    s.solve_async()
    s.eval_cost()
    view = sharding.device_tensor(s.device_ptr("cost"), (B0,))
    s.sync()
    out = view.cpu().numpy().copy()
    assert (out != 0).all() and cn.same_bits(out, s.get_cost())
    _check_all(ocp, s, M1)
    assert s.device_ptr("cost_stage") and s.device_ptr("cost_parts")
    s.close()


# ---- 5. nothing else moves: 16 384 instances (the pipelined lineariser runs), 8 ticks with every cost call against a twin without any
def test_cost_calls_change_no_result_and_keep_the_pipeline():
    B, N, K, T = 16384, 20, 8, 8
    wl = scenario.make_batch(M1, N, K, B, seed=3)
    runs = {}
    for cost in (True, False):
        _, s = _scenario_solver(M1, N, K, B, wl=wl)
        if cost:
            s.track_cost(True)
        for t in range(T):
            s.solve_async()
            if cost:
                s.eval_cost()
            s.advance(1e-3, 40 + t)
        s.sync()
        runs[cost] = (s.get_all("x"), s.get_all("u"), s.get("x0", 0), s.pipeline_stats())
        if cost:
            assert s.tracked_cost()[1] == T and np.isfinite(s.tracked_cost()[0]).all()
        s.close()
    for a, b in zip(runs[True][:3], runs[False][:3]):
        assert a.tobytes() == b.tobytes()
    assert runs[True][3] == runs[False][3], (runs[True][3], runs[False][3])
    used, discarded = runs[False][3]
    assert used > 0 and discarded == 0, (used, discarded)    # (the loop is one the lineariser runs ahead in)


# ---- 6. tracking: the sequential numpy sum over what a twin's host reads before each hand-over
def _track_loop(advance, start=None, T=12):
    (ocp, a), (_, b) = _solver(B0, N0, 4, _x0(B0)), _solver(B0, N0, 4, _x0(B0))
    if start:
        start(a)
    a.track_cost(True)
    tab = cn.tab_of_ocp(ocp, 4, False)
    want = np.zeros(B0)
    for t in range(T):
        a.solve(), b.solve()
        c0, _, _ = cn.stage(tab, b.dt, b.get("u", 0), b.get("x0", 0), b.get("yref", 0), b.get("sl", 0), b.get("su", 0))
        want = want + c0
        advance(a, t), advance(b, t)
    return a, b, want


def test_tracked_cost_through_advance():
    a, b, want = _track_loop(lambda s, t: s.advance(1e-3, 100 + t))
    got, count = a.tracked_cost()
    assert count == 12 and cn.same_bits(got, want) and (got > 0).all() and (got[0] != got[1:]).any()
    assert a.device_ptr("cost_tracked")
    for k in ("x", "u"):
        assert a.get_all(k).tobytes() == b.get_all(k).tobytes()
    a.track_cost(True)      # again: zeroes
    got, count = a.tracked_cost()
    assert count == 0 and cn.same_bits(got, np.zeros(B0))
    before = a.device_bytes()
    a.track_cost(False)
    assert a.device_bytes() == before - 8 * B0
    with pytest.raises(Exception, match="cost_tracked: no tracking is running"):
        a.tracked_cost()
    a.close(), b.close()


def test_tracked_cost_through_advance_sim_beside_a_log():
    sim = AcadosSim()
    sim.model = usv_models.make_ocp(M2, N0 * DT, N0, 4).model
    sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = DT, 3, False
    plant = BatchSimSolver(sim, B0)
    a, b, want = _track_loop(lambda s, t: s.advance_sim(plant, 1e-3, 7 + t), start=lambda s: s.start_log(12))
    got, count = a.tracked_cost()
    assert count == 12 and cn.same_bits(got, want)
    # the log beside it: its records are what a handle that only logs makes
    ocp, c = _solver(B0, N0, 4, _x0(B0))
    c.start_log(12)
    for t in range(12):
        c.solve()
        c.advance_sim(plant, 1e-3, 7 + t)
    la, lc = a.read_log(), c.read_log()
    assert a.log_info() == c.log_info()
    for k in ("x", "u", "status", "qp_iter"):
        assert np.ascontiguousarray(la[k]).tobytes() == np.ascontiguousarray(lc[k]).tobytes(), k
    a.close(), b.close(), c.close(), plant.close()


# ---- 7. shards: two handles over instances 0 .. 34 and 35 .. 69 return the whole batch's bits
def test_shards_return_the_whole_batchs_bits():
    wl = scenario.make_batch(M1, N0, 3, B0, seed=5)
    _, whole = _scenario_solver(M1, N0, 3, B0, wl=wl)
    parts = [_scenario_solver(M1, N0, 3, 35, wl=_slice(wl, a, a + 35))[1] for a in (0, 35)]
    parts[1].set_option("instance_offset", 35)
    for s in [whole] + parts:
        s.track_cost(True)
        for t in range(3):
            s.solve()
            s.advance(1e-3, 9 + t)
        s.solve()
    for f in (lambda s: s.get_cost(), lambda s: s.get("cost_stage", -1), lambda s: s.get("cost_parts", 0), lambda s: s.tracked_cost()[0]):
        assert cn.same_bits(np.concatenate([f(p) for p in parts]), f(whole))
    for s in [whole] + parts:
        s.close()


# ---- 8. refusals: each carries a message and changes nothing
def test_refusals():
    ocp, s = _scenario_solver(M1, N0, 3, B0)
    s.solve()
    want = s.get_cost()
    L, h = s._lib, s._h
    buf = np.zeros(B0 * (N0 + 1))
    p = buf.ctypes.data_as(_dp)
    assert L.usvmpc_get(h, b"cost", 0, p, 2) == E_SIZE and "mismatching dimension for field 'cost'" in _err(s)
    assert L.usvmpc_get(h, b"cost_parts", 0, p, 1) == E_SIZE and "expected 3" in _err(s)
    assert L.usvmpc_get(h, b"cost_stage", N0 + 1, p, 1) == -3 and "out of range for field 'cost_stage'" in _err(s)
    for f in (b"cost", b"cost_stage", b"cost_parts"):
        assert L.usvmpc_set(h, f, 0, p, 3 if f == b"cost_parts" else 1) == E_FIELD and "unknown field" in _err(s)
    assert L.usvmpc_get(h, b"cost", 0, None, 1) == E_ARG and _err(s) == "null buffer"
    assert L.usvmpc_cost_tracked(h, p, None) == E_ARG and "no tracking is running" in _err(s)
    pv = C.c_void_p()
    assert L.usvmpc_get_device_ptr(h, b"cost_tracked", C.byref(pv)) == E_ARG and "no tracking is running" in _err(s)
    assert L.usvmpc_get_device_ptr(h, b"cost", None) == E_ARG
    assert L.usvmpc_eval_cost(None) == E_ARG and L.usvmpc_cost_track(None, 1) == E_ARG and L.usvmpc_cost_tracked(None, None, None) == E_ARG
    assert (buf == 0).all() and cn.same_bits(s.get_cost(), want)
    s.track_cost(True)
    cnt = C.c_longlong(-1)
    assert L.usvmpc_cost_tracked(h, None, C.byref(cnt)) == 0 and cnt.value == 0      # (a null sum is allowed)
    s.close()
    # a handle with soft state bounds: every entry point
    ocp = usv_models.make_ocp(M0, N0 * DT, N0, None)
    ocp.constraints.idxsbx = np.array([0])
    ocp.constraints.lsbx, ocp.constraints.usbx = np.zeros(1), np.zeros(1)
    for nm in ("zl", "zu", "Zl", "Zu"):
        setattr(ocp.cost, nm, np.full(1, 10.0))
    s = BatchOcpSolver(ocp, 4)
    scenario.load_into(s, scenario.make_batch(M0, N0, 0, 4, seed=5))
    s.solve()
    before, x = s.device_bytes(), s.get_all("x")
    L, h = s._lib, s._h
    small = np.zeros(4 * (N0 + 1))
    p = small.ctypes.data_as(_dp)
    for rc in (L.usvmpc_get(h, b"cost", 0, p, 1), L.usvmpc_get(h, b"cost_stage", -1, p, 1), L.usvmpc_get(h, b"cost_parts", 0, p, 3),
               L.usvmpc_eval_cost(h), L.usvmpc_cost_track(h, 1), L.usvmpc_cost_track(h, 0), L.usvmpc_get_device_ptr(h, b"cost", C.byref(pv))):
        assert rc == E_ARG and _err(s) == "cost: not built for soft state bounds"
    assert s.device_bytes() == before and (small == 0).all() and s.get_all("x").tobytes() == x.tobytes()
    s.advance(0.0, 1)       # (and no tracking was started)
    assert L.usvmpc_cost_tracked(h, p, None) == E_ARG
    s.close()
