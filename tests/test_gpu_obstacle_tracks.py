"""Obstacle tracks on a real MI355X (`pytest -m gpu`): option "obstacle_tracks" - p derived on the device from a position and a velocity per
obstacle slot (kernel usv_obstacle_predict), the world stepped by the hand-over (usv_obstacle_step), the clearance kept.

* the device's p is scenario.predict_tracks bit for bit, for one and two obstacle chunks, static and per-stage;
* a handle with tracks and a handle whose host rebuilds p every tick solve the same closed loop bit for bit - both mappings, the partially
  condensed QP, full SQP;
* positions, clearance and its running minimum against numpy, with advance, advance_sim (another period) and with the world left to the caller;
* the moving loop against the CPU oracle handed the same inputs, judged by the project's parity rule;
* ownership of p, errors, lazy buffers; shards; the pipelined lineariser is not disturbed.
"""
import numpy as np
import pytest

from mpc_collisionavoidance_amd import AcadosSim, BatchOcpSolver, BatchSimSolver, scenario, sharding, usv_models
from tests import parity_rule, util

pytestmark = pytest.mark.gpu

M1, M2 = "usv_model_guidance_ca1", "usv_model_pf_ca"
ULP = 2.0 ** -52


def _mk(name, N, K, B, seed=1234, cond_N=None):
    wl = scenario.make_bench_batch(name, N, K, B, seed=seed, moving=True)
    ocp = usv_models.make_ocp(name, N * scenario.BENCH_DT, N, K)
    ocp.solver_options.sim_method_num_steps = scenario.BENCH_SIM_STEPS[name]
    if cond_N:
        ocp.solver_options.qp_solver_cond_N = cond_N
    return ocp, wl


def _solver(ocp, wl, B, name, tracks):
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, wl)
    s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
    if tracks:
        scenario.load_tracks(s, wl)
    return s


def _clearance(x0, pos, lh0, name):
    ipx = {M1: 5, M2: 10}[name]
    d = np.sqrt((x0[:, None, ipx] - pos[:, :, 0]) ** 2 + (x0[:, None, ipx + 1] - pos[:, :, 1]) ** 2)
    i = np.argmin(d - lh0, axis=1)
    return (d - lh0).min(axis=1), d[np.arange(d.shape[0]), i]


# ---- 4. prediction
@pytest.mark.parametrize("name,N,K,B", [(M1, 100, 8, 1000), (M2, 40, 10, 2050), (M2, 80, 20, 300)])
def test_device_p_is_predict_tracks(name, N, K, B):
    ocp, wl = _mk(name, N, K, B, seed=5)
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, wl)
    held = np.random.default_rng(1).uniform(-50.0, 50.0, wl["p"].shape)
    s.set_all("p", held)                                  # what the stages hold before the tracks take over
    s.set_option("static_obstacles", 1)
    s.set_obstacle_tracks(wl["obs_pos"], wl["obs_vel"])
    s.solve()
    p = s.get_all("p")
    want = scenario.predict_tracks(wl["obs_pos"], wl["obs_vel"], N, s.dt)
    assert np.array_equal(want, wl["p"])
    assert np.array_equal(p[:, 0], want[:, 0]) and np.array_equal(p[:, 1:], held[:, 1:])
    s.set_option("static_obstacles", 0)
    s.solve()
    assert np.array_equal(s.get_all("p"), want)
    # a course change is one small set; the next solve predicts again
    s.set("obs_vel", 0, -wl["obs_vel"])
    s.solve()
    assert np.array_equal(s.get_all("p"), scenario.predict_tracks(wl["obs_pos"], -wl["obs_vel"], N, s.dt))
    assert np.array_equal(s.get("obs_pos", 0), wl["obs_pos"]) and np.array_equal(s.get("obs_vel", 0), -wl["obs_vel"])
    s.close()


# ---- 5. + 6. the solver cannot tell the difference; world and clearance
def _twin_loop(name, N, K, B, ticks=8, wide=None, cond_N=None, sqp=False, step="advance"):
    ocp, wl = _mk(name, N, K, B, cond_N=cond_N)
    a, b = _solver(ocp, wl, B, name, True), _solver(ocp, wl, B, name, False)
    plant, T = None, a.dt
    if step == "advance_sim":
        sim = AcadosSim()
        sim.model = ocp.model
        T = 0.02
        sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = T, 4, False
        plant = BatchSimSolver(sim, B)
    if step == "manual":
        a.set_option("obstacle_step_on_advance", 0)
    for s in (a, b):
        if wide is not None:
            s.set_option("wide", wide)
    pos, vel, lh0 = wl["obs_pos"].copy(), wl["obs_vel"], wl["lh"][:, 0]
    run_min = np.full(B, 1e300)
    assert np.all(a.get("clearance_min", 0) == 1e300)
    for t in range(ticks):
        b.set_all("p", scenario.predict_tracks(pos, vel, N, b.dt))
        ra = a.solve_sqp() if sqp else a.solve()
        rb = b.solve_sqp() if sqp else b.solve()
        assert np.array_equal(ra, rb), t
        if wide is not None:
            assert (a.last_mapping() > 0) == (wide > 0) and (b.last_mapping() > 0) == (wide > 0)
        for f in ("status", "qp_status", "qp_iter"):
            assert np.array_equal(a.get_int(f), b.get_int(f)), (t, f)
        assert np.array_equal(a.get_all("x"), b.get_all("x")) and np.array_equal(a.get_all("u"), b.get_all("u")), t
        assert np.array_equal(a.get_all("p"), b.get_all("p")), t
        for s in (a, b):
            if plant is None:
                s.advance(1e-3, seed=t)
            else:
                s.advance_sim(plant, sigma=1e-3, seed=t)
        if step == "manual":
            assert np.array_equal(a.get("obs_pos", 0), pos)      # the hand-over left the world alone
            a.step_obstacles(T)
        pos = pos + T * vel
        x0 = a.get("x0", 0)
        assert np.array_equal(x0, b.get("x0", 0)), t
        assert np.array_equal(a.get("obs_pos", 0), pos), t
        want, dist = _clearance(x0, pos, lh0, name)
        got = a.get("clearance", 0)
        print("tick %d: clearance differs from numpy's by at most %.3g (bound %.3g)" % (t, np.abs(got - want).max(), (4 * ULP * dist).min()))
        assert np.all(np.abs(got - want) <= 4 * ULP * dist), t
        run_min = np.minimum(run_min, got)
        assert np.array_equal(a.get("clearance_min", 0), run_min), t
        if t == ticks // 2:      # the caller sets the positions anew: the minimum starts again
            a.set("obs_pos", 0, pos)
            assert np.all(a.get("clearance_min", 0) == 1e300)
            run_min = np.full(B, 1e300)
    for s in (a, b):
        s.close()
    if plant is not None:
        plant.close()


def test_twin_loop_guidance_ca1():
    _twin_loop(M1, 40, 10, 256)


@pytest.mark.parametrize("wide", [0, 1])
def test_twin_loop_pf_ca_both_mappings(wide):
    _twin_loop(M2, 40, 10, 256, wide=wide)


def test_twin_loop_pf_ca_two_chunks():
    _twin_loop(M2, 80, 20, 128)


def test_twin_loop_pf_ca_two_chunks_condensed():
    _twin_loop(M2, 80, 20, 128, cond_N=10)


def test_twin_loop_guidance_ca1_full_sqp():
    _twin_loop(M1, 40, 10, 256, sqp=True)


def test_world_steps_by_the_plants_period():
    _twin_loop(M2, 40, 10, 256, step="advance_sim")


def test_world_left_to_the_caller():
    _twin_loop(M1, 40, 10, 256, step="manual")


# ---- 7. against the oracle
@pytest.mark.parametrize("name", [M1, M2])
def test_moving_loop_against_the_oracle(oracle, name):
    N, K, B = 40, 10, 256
    ocp, wl = _mk(name, N, K, B)
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, wl)
    scenario.load_tracks(s, wl)
    spec = oracle.spec(util.MODEL_ID[name], N, N * scenario.BENCH_DT, K, sim_steps=scenario.BENCH_SIM_STEPS[name])
    pos, vel = wl["obs_pos"].copy(), wl["obs_vel"]
    xg, ug, x0 = wl["x_init"].copy(), wl["u_init"].copy(), wl["x0"].copy()
    for t in range(8):
        xs, us, xin, uin = xg.copy(), ug.copy(), xg.copy(), ug.copy()
        data = (wl["yref"], wl["yref_e"], scenario.predict_tracks(pos, vel, N, s.dt), wl["lh"])
        s.solve()
        sts, its = oracle.rti_batch(spec, xs, us, x0, *data, threads=8)
        qs = s.get_int("qp_status")
        xg, ug = s.get_all("x"), s.get_all("u")
        ok = (qs == 0) & (sts == 0) & (its < spec.opts.qp_iter_max)
        print(name, "tick", t, "converged on both sides: %.4f" % ok.mean())
        assert ok.mean() >= 0.97, (name, t, ok.mean())
        e = np.maximum(util.rel_err_per_instance(xg[ok], xs[ok]), util.rel_err_per_instance(ug[ok], us[ok]))
        print(name, "tick", t, "worst error %.3g, median %.3g" % (e.max(), np.median(e)))
        if name == M1:
            assert e.max() <= 1e-7, (t, e.max())
        else:
            r = parity_rule.check(oracle, spec, s, ok, e, xin, uin, x0, data, soft=False)
            assert not r["violations"], (t, r)
        s.advance(0.0)
        pos = pos + s.dt * vel
        x0 = s.get("x0", 0)
        assert np.array_equal(s.get("obs_pos", 0), pos)
    s.close()


# ---- 8. ownership and errors
def test_ownership_errors_and_lazy_buffers():
    N, K, B = 20, 6, 96
    ocp, wl = _mk(M2, N, K, B, seed=3)
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, wl)
    with pytest.raises(Exception, match="obs_pos"):
        s.set_option("obstacle_tracks", 1)                # no positions yet
    with pytest.raises(Exception, match="obs_pos"):
        s.get("obs_pos", 0)
    with pytest.raises(Exception, match="obs_pos"):
        s.step_obstacles(0.05)
    before = s.device_bytes()
    s.set("obs_pos", 0, wl["obs_pos"])
    own = 2 * B * 2 * K * 8
    grown = s.device_bytes() - before
    assert own <= grown < 2 * own + 65536, (own, grown)
    assert np.all(s.get("obs_vel", 0) == 0.0)             # the default
    with_tracks = s.device_bytes()
    s.set_all("p", wl["p"])                               # still the caller's
    s.set_option("obstacle_tracks", 1)
    with pytest.raises(Exception, match="obstacle_tracks"):
        s.set_all("p", wl["p"])
    with pytest.raises(Exception, match="obstacle_tracks"):
        s.set("p", 3, wl["p"][:, 3])
    s.solve()
    assert np.array_equal(s.get_all("p"), scenario.predict_tracks(wl["obs_pos"], np.zeros_like(wl["obs_vel"]), N, s.dt))
    s.set_option("obstacle_tracks", 0)
    s.set_all("p", wl["p"])                               # handed back
    s.solve()
    assert np.array_equal(s.get_all("p"), wl["p"])
    s.set_option("obstacle_tracks", 1)
    assert s.device_bytes() == with_tracks
    with pytest.raises(Exception, match="mismatching dimension"):
        s._check(s._lib.usvmpc_set(s._h, b"obs_pos", 0, np.zeros(B * 2 * K).ctypes.data_as(_dp()), 2 * K + 1))
    with pytest.raises(Exception, match="read-only"):
        s._check(s._lib.usvmpc_set(s._h, b"clearance", 0, np.zeros(B).ctypes.data_as(_dp()), 1))
    s.close()
    s0 = BatchOcpSolver(usv_models.make_ocp("usv_model", 1.0, 20), 8)   # K = 0
    bytes0 = s0.device_bytes()
    for call in (lambda: s0.get("obs_pos", 0), lambda: s0.get("clearance", 0), lambda: s0.set("obs_vel", 0, np.zeros((8, 0))),
                 lambda: s0.step_obstacles(0.05)):
        with pytest.raises(Exception, match="no obstacle rows"):
            call()
    assert s0._lib.usvmpc_get(s0._h, b"obs_pos", 0, np.zeros(8).ctypes.data_as(_dp()), 0) == -2      # USVMPC_E_FIELD
    assert s0.device_bytes() == bytes0
    s0.close()


def _dp():
    from mpc_collisionavoidance_amd import _capi
    return _capi._dp


def test_device_pointer_to_the_tracks_keeps_the_prediction_running():
    import torch
    N, K, B = 20, 4, 64
    ocp, wl = _mk(M1, N, K, B, seed=9)
    s = _solver(ocp, wl, B, M1, True)
    s.solve()
    t = sharding.device_tensor(s.device_ptr("obs_pos"), (B, K, 2))
    t += 0.25                                             # the caller's own kernel moves the obstacles behind the handle's back
    torch.cuda.synchronize()
    s.solve()
    assert np.array_equal(s.get_all("p"), scenario.predict_tracks(wl["obs_pos"] + 0.25, wl["obs_vel"], N, s.dt))
    s.close()


# ---- 9. shards
def test_shards_with_tracks_equal_the_unsharded_batch():
    name, N, K, B = M2, 20, 6, 203
    ocp, wl = _mk(name, N, K, B, seed=77)

    def run(w, n, offset):
        s = _solver(ocp, w, n, name, True)
        s.set_option("instance_offset", offset)
        for t in range(4):
            s.solve()
            s.advance(1e-3, seed=50 + t)
        s.sync()
        out = (s.get_all("x"), s.get_all("u"), s.get_int("status"), s.get_int("qp_iter"), s.get("x0", 0), s.get_all("p"), s.get("obs_pos", 0),
               s.get("clearance", 0), s.get("clearance_min", 0))
        s.close()
        return out

    whole = run(wl, B, 0)
    parts = []
    for r in range(2):
        lo, hi = sharding.shard_bounds(B, 2, r)
        parts.append(run(sharding.split_workload(wl, 2, r), hi - lo, lo))
    for i in range(len(whole)):
        assert np.array_equal(np.concatenate([parts[0][i], parts[1][i]], axis=0), whole[i]), i


# ---- 10. the pipelined lineariser
def test_tracks_do_not_disturb_the_pipelined_lineariser():
    name, N, K, B = M2, 40, 10, 16384
    ocp, wl = _mk(name, N, K, B)
    wl = dict(wl, p=scenario.predict_tracks(wl["obs_pos"], np.zeros_like(wl["obs_vel"]), N, scenario.BENCH_DT))   # a world that stands still
    res = []
    for tracks in (True, False):
        s = BatchOcpSolver(ocp, B)
        scenario.load_into(s, wl)
        s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
        if tracks:
            s.set_obstacle_tracks(wl["obs_pos"])          # zero velocity: both loops solve the same problems
        for t in range(6):
            s.solve_async()
            s.advance(1e-3, seed=t)
        s.sync()
        res.append((s.pipeline_stats(), s.get_all("x"), s.get_all("u"), s.get_all("p")))
        s.close()
    print("pipeline_stats with tracks / without:", res[0][0], res[1][0])
    assert res[0][0] == res[1][0] and res[0][0][0] > 0
    for i in (1, 2, 3):
        assert np.array_equal(res[0][i], res[1][i]), i
