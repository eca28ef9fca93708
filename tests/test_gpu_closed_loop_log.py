"""The closed-loop log on a real MI355X (`pytest -m gpu`): kernel usv_log_record through the C ABI usvmpc_log_* and
BatchOcpSolver.start_log / read_log / log_errors (include/usvmpc.h, "Closed-loop log").

The yardstick is always a TWIN handle without a log, driven through the same calls, from which the host reads get("x0", 0), get("u", 0),
get_int("status") and get_int("qp_iter") just before each hand-over - the reference's simX[i] = get(0, "x"), simU[i] = get(0, "u").  The
logged handle's records must equal those arrays bit for bit, and its final x / u must equal the twin's bit for bit: logging changes no result.
The shapes are those of tests/test_gpu_pf_frontend.py (N = 6, K = 4, 5 RK4 steps per interval)."""
import ctypes as C

import numpy as np
import pytest

from mpc_collisionavoidance_amd import AcadosSim, BatchOcpSolver, BatchSimSolver, scenario, usv_models
from mpc_collisionavoidance_amd.guidance import PathFollowingFrontEnd

pytestmark = pytest.mark.gpu

M0, M1, M2 = "usv_model", "usv_model_guidance_ca1", "usv_model_pf_ca"
DT, STEPS = 0.05, 5
# a state the model can be linearised at (u = 0 is not one): heading up leg 1 at 0.7 m/s
GENERIC = np.array([np.pi / 2, 1.0, 0.0, 0.7, 0.0, 0.0, 0.0, 4.0, -5.0, np.pi / 2, 4.0, -4.5, 0.0, 0.0])
CHANNELS = [(0, 9), (3, 0.7), (6, 0.0)]     # psi - ak, u - 0.7, ye (scripts/usv_pf_ca/main.py)


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


def _x0(B):
    """instances that differ: a record in the wrong place shows"""
    rng = np.random.default_rng(33)
    x0 = np.tile(GENERIC, (B, 1))
    x0[:, 0] += rng.uniform(-0.2, 0.2, B)
    x0[:, 3] += rng.uniform(-0.1, 0.1, B)
    x0[:, 4] = rng.uniform(-0.02, 0.02, B)
    x0[:, 6] = rng.uniform(-0.3, 0.3, B)
    x0[:, 10] += rng.uniform(-0.5, 0.5, B)
    return x0


def _scenario_solver(name, N, K, B, seed=5):
    ocp = usv_models.make_ocp(name, N * scenario.DT[name], N, K or None)
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, scenario.make_batch(name, N, K, B, seed=seed))
    s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
    return ocp, s


def _readback(s):
    """what the reference's loop stores just before the hand-over"""
    return dict(x=s.get("x0", 0), u=s.get("u", 0), status=s.get_int("status").copy(), qp_iter=s.get_int("qp_iter").copy())


def _stack(rows):
    """per-tick read-backs -> instance-major arrays [B][T][..], the shape of read_log"""
    return {k: np.stack([r[k] for r in rows], axis=1) for k in rows[0]}


def _same(log, want, ticks, states=None, b=slice(None), what=""):
    """the log's channels against the twin's read-backs at the hand-overs `ticks`"""
    assert log["tick"].tolist() == list(ticks), (what, log["tick"])
    if "x" in log:
        wx = want["x"][b][:, ticks]
        wx = wx if states is None else wx[:, :, states]
        assert log["x"].shape == wx.shape and np.array_equal(log["x"].view(np.uint64), np.ascontiguousarray(wx).view(np.uint64)), what
    if "u" in log:
        wu = np.ascontiguousarray(want["u"][b][:, ticks])
        assert log["u"].shape == wu.shape and np.array_equal(np.ascontiguousarray(log["u"]).view(np.uint64), wu.view(np.uint64)), what
    if "status" in log:
        assert np.array_equal(log["status"], want["status"][b][:, ticks]) and np.array_equal(log["qp_iter"], want["qp_iter"][b][:, ticks]), what


def _final_equal(a, b):
    assert np.array_equal(a.get_all("x").view(np.uint64), b.get_all("x").view(np.uint64))
    assert np.array_equal(a.get_all("u").view(np.uint64), b.get_all("u").view(np.uint64))
    assert np.array_equal(a.get("x0", 0).view(np.uint64), b.get("x0", 0).view(np.uint64))


B3, T3 = 70, 12


@pytest.fixture(scope="module")
def twin3():
    """The twin of tests 3, 5 and 9, computed once: usv_model_pf_ca, B = 70 (a partial last wave), 12 ticks of solve + advance(1e-3)."""
    ocp, s = _solver(B3, 6, 4, _x0(B3))
    rows = []
    for t in range(T3):
        s.solve()
        rows.append(_readback(s))
        s.advance(1e-3, 100 + t)
    out = dict(_stack(rows), final_x=s.get_all("x"), final_u=s.get_all("u"), final_x0=s.get("x0", 0))
    s.close()
    return out


def _run3(start, ticks=T3):
    """the loop of twin3 on a handle whose log `start` starts"""
    ocp, s = _solver(B3, 6, 4, _x0(B3))
    start(s)
    for t in range(ticks):
        s.solve()
        s.advance(1e-3, 100 + t)
    return s


# ---- 3. all channels, a schedule with a first, a stride and a full buffer
def test_records_equal_the_twins_readbacks(twin3):
    s = _run3(lambda s: s.start_log(5, every=2, first=1))
    info = s.log_info()
    assert (info["records"], info["handovers"], info["missed"], info["nsel"]) == (5, 12, 1, 14)
    ticks = [1, 3, 5, 7, 9]
    log = s.read_log()
    assert log["states"] == list(range(14)) and log["x"].shape == (70, 5, 14) and log["u"].shape == (70, 5, 2) and log["status"].shape == (70, 5)
    _same(log, twin3, ticks, what="whole log")
    assert (log["qp_iter"] > 0).any() and (log["x"][:, 0] != log["x"][:, 4]).any() and (log["x"][0] != log["x"][69]).any()
    _same(s.read_log(instances=(64, 70)), twin3, ticks, b=slice(64, 70), what="instances 64 .. 69")
    _same(s.read_log(records=(2, 4)), twin3, ticks[2:4], what="records 2 .. 3")
    _same(s.read_log(records=range(4, 5), instances=range(69, 70)), twin3, ticks[4:], b=slice(69, 70), what="last instance of the last record")
    for k in ("x", "u", "x0"):
        got = s.get_all(k) if k != "x0" else s.get("x0", 0)
        assert np.array_equal(got.view(np.uint64), twin3["final_" + k].view(np.uint64)), k
    s.close()


# ---- 4. packing: an odd selection on a model with one input; a single instance behind the host mirror, no u
@pytest.mark.parametrize("name,K,B,states,u", [(M1, 4, 257, [5, 6, 7], True), (M0, 0, 1, [0], False)])
def test_packing(name, K, B, states, u):
    T = 6
    (_, a), (_, b) = _scenario_solver(name, 6, K, B), _scenario_solver(name, 6, K, B)
    a.start_log(T, states=states, u=u)
    rows = []
    for t in range(T):
        a.solve(), b.solve()
        rows.append(_readback(b))
        a.advance(1e-3, 40 + t), b.advance(1e-3, 40 + t)
    log = a.read_log()
    assert log["states"] == states and log["x"].shape == (B, T, len(states)) and ("u" in log) == u
    if u:
        assert log["u"].shape == (B, T, a.nu)
    _same(log, _stack(rows), list(range(T)), states=states, what=name)
    assert (log["x"][:, 0] != log["x"][:, T - 1]).any()
    _final_equal(a, b)
    a.close(), b.close()


# ---- 5. the error sums
def _numpy_sums(X, channels):
    """X [B][T][nx]: the sequential loop, one rounding per operation, in tick order"""
    sa, sq = np.zeros((X.shape[0], len(channels))), np.zeros((X.shape[0], len(channels)))
    for t in range(X.shape[1]):
        for c, (i, j) in enumerate(channels):
            e = X[:, t, i] - (X[:, t, j] if isinstance(j, int) else np.float64(j))
            sa[:, c] = sa[:, c] + np.abs(e)
            sq[:, c] = sq[:, c] + e * e
    return sa, sq


def test_error_sums_are_the_sequential_numpy_sums(twin3):
    s = _run3(lambda s: s.start_log(T3, errors=CHANNELS, errors_first=4))
    log = s.read_log()
    _same(log, twin3, list(range(T3)), what="every tick")
    sa, sq = _numpy_sums(log["x"][:, 4:], CHANNELS)
    err = s.log_errors()
    assert err["count"] == 8 and err["sum_abs"].shape == (B3, 3)
    assert np.array_equal(err["sum_abs"].view(np.uint64), sa.view(np.uint64)) and np.array_equal(err["sum_sq"].view(np.uint64), sq.view(np.uint64))
    assert (sa[:, 1] > 0).all() and (sq > 0).any()
    s.close()
    # errors alone: no record, the same sums
    s = _run3(lambda s: s.start_log(1, states=[], u=False, status=False, errors=CHANNELS, errors_first=4))
    info = s.log_info()
    assert (info["records"], info["handovers"], info["missed"], info["nsel"]) == (0, 12, 0, 0)
    err2 = s.log_errors()
    assert err2["count"] == 8
    assert np.array_equal(err2["sum_abs"].view(np.uint64), sa.view(np.uint64)) and np.array_equal(err2["sum_sq"].view(np.uint64), sq.view(np.uint64))
    assert np.array_equal(s.get("x0", 0).view(np.uint64), twin3["final_x0"].view(np.uint64))
    s.close()


# ---- 6. a plant of its own
def test_advance_sim_is_a_hand_over():
    B, N, T = 70, 6, 6
    (ocp, a), (_, b) = _solver(B, N, 4, _x0(B)), _solver(B, N, 4, _x0(B))
    sim = AcadosSim()
    sim.model = ocp.model
    sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = DT, 3, False
    plant = BatchSimSolver(sim, B)
    a.start_log(T)
    rows = []
    for t in range(T):
        a.solve(), b.solve()
        rows.append(_readback(b))
        a.advance_sim(plant, 1e-3, 7 + t), b.advance_sim(plant, 1e-3, 7 + t)
    assert a.log_info()["handovers"] == T
    _same(a.read_log(), _stack(rows), list(range(T)), what="advance_sim")
    _final_equal(a, b)
    a.close(), b.close(), plant.close()


# ---- 7. a device-resident mission
def test_resident_mission_is_logged_without_a_host_array():
    B, N, K, T = 64, 6, 4, 10
    m = scenario.make_pf_missions(B, 0)
    hs = []
    for _ in range(2):
        ocp, s = _solver(B, N, K, m["x0"])
        fe = PathFollowingFrontEnd(s)
        fe.reset(m["waypoints"])
        fe.set_world(m["world"], max_radius=scenario.PF_MISSION_OCP["max_radius"], margin=scenario.PF_MISSION_OCP["margin"])
        hs.append((s, fe))
    (a, fa), (b, fb) = hs
    a.start_log(T, states=[0, 10, 11], errors=CHANNELS)
    rows = []
    for t in range(T):
        for s, fe in hs:
            fe.prepare()
            s.solve_async()
            fe.publish(fetch=False)
        rows.append(_readback(b))      # (the twin pays the synchronisation the log saves)
        a.advance(), b.advance()
    log = a.read_log()
    want = _stack(rows)
    _same(log, want, list(range(T)), states=[0, 10, 11], what="resident mission")
    assert (log["x"][:, 0, 2] != log["x"][:, T - 1, 2]).any()      # vessels moved north
    sa, sq = _numpy_sums(want["x"], CHANNELS)
    err = a.log_errors()
    assert err["count"] == T and np.array_equal(err["sum_abs"].view(np.uint64), sa.view(np.uint64))
    assert np.array_equal(err["sum_sq"].view(np.uint64), sq.view(np.uint64))
    sta, stb = fa.state(), fb.state()
    assert sta.keys() == stb.keys()
    for k in sta:
        assert np.array_equal(sta[k], stb[k]), k
    _final_equal(a, b)
    a.close(), b.close()


# ---- 8. the pipelined lineariser keeps running
def test_logging_leaves_the_pipeline_alone():
    name, N, B, T = M0, 20, 16384, 8      # the smallest batch that pipelines
    (_, a), (_, b) = _scenario_solver(name, N, 0, B), _scenario_solver(name, N, 0, B)
    a.start_log(T)
    last = None
    for t in range(T):
        a.solve_async(), b.solve_async()
        if t == T - 1:
            last = _readback(b)
        a.advance(1e-3, 50 + t), b.advance(1e-3, 50 + t)
    a.sync(), b.sync()
    _final_equal(a, b)
    used, discarded = b.pipeline_stats()
    assert used > 0 and discarded == 0, (used, discarded)      # the test did exercise the pipeline
    assert a.pipeline_stats() == (used, discarded)
    a.log_device_ptr("x")                                       # (exposes log memory only: nothing is cancelled)
    assert a.pipeline_stats() == (used, discarded)
    assert a.log_info()["records"] == T
    log = a.read_log(records=(T - 1, T))
    assert log["tick"].tolist() == [T - 1]
    assert np.array_equal(log["x"][:, 0].view(np.uint64), last["x"].view(np.uint64))
    assert np.array_equal(log["u"][:, 0].view(np.uint64), last["u"].view(np.uint64))
    assert np.array_equal(log["status"][:, 0], last["status"]) and np.array_equal(log["qp_iter"][:, 0], last["qp_iter"])
    a.close(), b.close()


# ---- 9. book-keeping
def test_bookkeeping(twin3):
    ocp, s = _solver(B3, 6, 4, _x0(B3))
    lib, h = s._lib, s._h
    buf = np.zeros(B3 * 14)
    E_ARG = -1

    def refused(rc, text):
        assert rc == E_ARG and text in lib.usvmpc_last_error(h).decode(), (rc, lib.usvmpc_last_error(h))

    refused(lib.usvmpc_log_read(h, b"x", 0, 1, 0, B3, buf.ctypes.data_as(C.c_void_p), buf.nbytes), "no log is running")
    refused(lib.usvmpc_log_stop(h), "no log is running")
    with pytest.raises(Exception, match="no log is running"):
        s.read_log()
    for t in range(3):
        s.solve()
        s.advance(1e-3, 100 + t)
    base = s.device_bytes()
    s.start_log(4, errors=CHANNELS[:2])
    layout = 4 * B3 * (14 * 8 + 2 * 8 + 4) + 2 * B3 * 2 * 8
    assert s.device_bytes() == base + layout
    with pytest.raises(Exception, match="usvmpc_log_stop first"):
        s.start_log(4)
    assert s.device_bytes() == base + layout and s.log_info() == dict(records=0, handovers=0, missed=0, nsel=14)
    for t in range(3, 5):
        s.solve()
        s.advance(1e-3, 100 + t)
    # a log started after 3 ticks counts hand-overs from 0: records 0, 1 are the twin's ticks 3, 4
    assert s.log_info() == dict(records=2, handovers=2, missed=0, nsel=14)
    log = s.read_log()
    assert log["tick"].tolist() == [0, 1]
    assert np.array_equal(log["x"].view(np.uint64), np.ascontiguousarray(twin3["x"][:, 3:5]).view(np.uint64))
    assert np.array_equal(log["status"], twin3["status"][:, 3:5]) and np.array_equal(log["qp_iter"], twin3["qp_iter"][:, 3:5])
    two = np.zeros(2 * B3 * 14)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    refused(lib.usvmpc_log_read(h, b"x", 0, 3, 0, B3, vp(np.zeros(3 * B3 * 14)), 3 * B3 * 14 * 8), "records outside")
    refused(lib.usvmpc_log_read(h, b"x", 2, 1, 0, B3, vp(buf), buf.nbytes), "records outside")
    refused(lib.usvmpc_log_read(h, b"x", 0, 1, 69, 2, vp(two), 2 * 14 * 8), "instances outside")
    refused(lib.usvmpc_log_read(h, b"x", 0, 2, 0, B3, vp(two), two.nbytes - 8), "exactly")
    refused(lib.usvmpc_log_read(h, b"x", 0, 2, 0, B3, vp(two), two.nbytes + 8), "exactly")
    refused(lib.usvmpc_log_read(h, b"cost", 0, 2, 0, B3, vp(two), two.nbytes), "channels")
    assert (two == 0).all() and s.log_info() == dict(records=2, handovers=2, missed=0, nsel=14)
    assert lib.usvmpc_log_read(h, b"x", 0, 2, 0, B3, vp(two), two.nbytes) == 0
    assert np.array_equal(two.reshape(2, B3, 14).view(np.uint64), np.ascontiguousarray(twin3["x"][:, 3:5].transpose(1, 0, 2)).view(np.uint64))
    assert s.log_errors()["count"] == 2
    s.stop_log()
    assert s.device_bytes() == base
    with pytest.raises(Exception, match="no log is running"):
        s.log_info()
    for kw, text in ((dict(capacity=0), "capacity"), (dict(capacity=2, states=[14]), "state_mask"),
                     (dict(capacity=2, states=[], u=False, status=False), "records nothing"), (dict(capacity=2, errors=[(0, 14)]), "err_b")):
        with pytest.raises(Exception, match=text):
            s.start_log(**kw)
        assert s.device_bytes() == base
    s.start_log(1, states=[3], u=False, status=False)      # a new log after a stop; close() stops it
    assert s.device_bytes() == base + B3 * 8
    s.close()


# ---- 10. the examples' --log-every
def _example(name):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_examples_keep_their_trajectories():
    pf = _example("pf_mission_sweep")
    a, b = pf.run(64, 12, N=6, quiet=True, log_every=4), pf.run(64, 12, N=6, quiet=True)
    assert a["log_tick"].tolist() == [0, 4, 8] and a["log_pose"].shape == (64, 3, 3) and a["error_count"] == 12
    assert np.array_equal(a["final_pose"], b["final_pose"]) and "log_pose" not in b
    m = scenario.make_pf_missions(64, 0)
    assert np.array_equal(a["log_pose"][:, 0], m["x0"][:, [10, 11, 0]])       # record 0 is the start pose
    assert a["mean_abs_error"].shape == (64, 3) and np.isfinite(a["mean_sq_error"]).all()
    ca = _example("scenario_sweep")
    a, b = ca.run(64, 8, N=10, quiet=True, resident=True, log_every=3), ca.run(64, 8, N=10, quiet=True, resident=True)
    assert a["log_tick"].tolist() == [0, 3, 6] and a["log_pose"].shape == (64, 3, 3) and a["error_count"] == 8
    assert np.array_equal(a["final_pose"], b["final_pose"])
    m = scenario.make_ca_missions(64, 5, 0)
    assert np.array_equal(a["log_pose"][:, 0], m["pose"])
