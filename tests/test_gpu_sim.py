"""The integrator on a real MI355X (`pytest -m gpu`): usvmpc_sim_* / BatchSimSolver / AcadosSimSolver against the oracle's ERK4 with
forward sensitivities (oracle.binding.erk_sens), bit identities (sens_forw on / off, an instance alone / in a batch), the symbolic model
through its generated library, and the closed-loop plant step usvmpc_advance_sim with the global noise key (option "instance_offset")."""
import numpy as np
import pytest

from mpc_collisionavoidance_amd import BatchOcpSolver, scenario, sharding, usv_models
from mpc_collisionavoidance_amd.acados_template import AcadosSim, AcadosSimSolver, BatchSimSolver
from tests import util

pytestmark = pytest.mark.gpu
MODELS = ["usv_model", "usv_model_guidance_ca1", "usv_model_pf_ca"]


def _points(name, B, seed=0):
    """States / inputs inside each model's operating range: surge 0.3 .. 1 m/s (below the 1.25 m/s switch of the 3-DOF drag), and for
    the 3-DOF block sway |v| <= 0.02 m/s, yaw rate |r| <= 0.1 rad/s.  The sway drag is stiff - its eigenvalue is about
    2 (CY + Yvv) |v| / (m - Yvd), 800 |v| 1/s - and one RK4 step of 0.1 s is stable only for |lambda| T < 2.8; at |v| = 0.2 a step
    amplifies rounding by up to 15^4 / 24, so neither implementation's digits would mean anything there."""
    rng = np.random.default_rng(seed)
    U = lambda lo, hi: rng.uniform(lo, hi, B)
    if name == "usv_model":
        x = np.column_stack([U(0.3, 1.0), U(-0.02, 0.02), U(-0.1, 0.1), U(-20, 20), U(-20, 20)])
        u = np.column_stack([U(-5, 5), U(-5, 5)])
    elif name == "usv_model_guidance_ca1":
        x = np.column_stack([U(0.3, 1.0), U(-0.2, 0.2), U(-2, 2), U(-1, 1), U(-0.5, 0.5), U(-5, 5), U(-5, 5), U(-np.pi, np.pi)])
        u = U(-0.5, 0.5)[:, None]
    else:
        psi = U(-np.pi, np.pi)
        x = np.column_stack([psi, np.sin(psi), np.cos(psi), U(0.3, 1.0), U(-0.02, 0.02), U(-0.1, 0.1), U(-2, 2), U(-5, 5), U(-5, 5),
                             U(-np.pi, np.pi), U(-5, 5), U(-5, 5), U(-20, 20), U(-20, 20)])
        u = np.column_stack([U(-5, 5), U(-5, 5)])
    return x, u


def _oracle(oracle, mid, T, steps, x, u):
    B, nx = x.shape
    xn, S = np.empty_like(x), np.empty((B, nx, nx + u.shape[1]))
    for b in range(B):
        xn[b], S[b, :, :nx], S[b, :, nx:] = oracle.erk_sens(mid, T, steps, x[b], u[b])
    return xn, S


def _close(g, o):
    """1e-12 relative, with an absolute floor of 1e-12"""
    return np.all(np.abs(g - o) <= np.maximum(1e-12 * np.abs(o), 1e-12)), np.max(np.abs(g - o) / np.maximum(np.abs(o), 1.0))


def _sim(name, T, steps, sens=True):
    sim = AcadosSim()
    sim.model = usv_models.make_ocp(name, 1.0, 20).model
    sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = T, steps, sens
    return sim


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("steps", [1, 3, 10])
def test_matches_oracle_and_is_independent_of_the_batch(oracle, name, steps):
    x, u = _points(name, 4099, seed=steps)
    mid = util.MODEL_ID[name]
    for T in (0.05, 0.1):
        xo, So = _oracle(oracle, mid, T, steps, x, u)
        out = {}
        for B in (1, 5, 4099):
            s = BatchSimSolver(_sim(name, T, steps), B)
            s.set("x", x[:B])
            s.set("u", u[:B])
            assert s.solve() == 0
            xg, Sg = s.get("x"), s.get("S_forw")
            s.close()
            ok_x, ex = _close(xg, xo[:B])
            ok_s, es = _close(Sg, So[:B])
            assert ok_x and ok_s, (name, steps, T, B, ex, es)
            out[B] = (xg, Sg)
        # an instance solved alone, or among 5, is the same bits as inside the batch of 4099
        for B in (1, 5):
            assert np.array_equal(out[B][0], out[4099][0][:B]) and np.array_equal(out[B][1], out[4099][1][:B]), (name, steps, T, B)


@pytest.mark.parametrize("name", MODELS)
def test_x_next_is_the_same_bits_with_and_without_sensitivities(name):
    x, u = _points(name, 1000, seed=5)
    res = []
    for sens in (True, False):
        s = BatchSimSolver(_sim(name, 0.05, 10, sens), 1000)
        s.set("x", x)
        s.set("u", u)
        s.solve()
        res.append(s.get("x"))
        if not sens:
            with pytest.raises(Exception, match="sens_forw"):
                s.get("S_forw")
        s.close()
    assert np.array_equal(res[0], res[1]), name


def test_acados_protocol(oracle):
    name, N, Tf = "usv_model_pf_ca", 20, 1.0
    ocp = usv_models.make_ocp(name, Tf, N, 4)
    ocp.solver_options.sim_method_num_steps = 3
    integ = AcadosSimSolver(ocp, json_file="acados_sim.json")
    assert integ.T == pytest.approx(Tf / N)
    x, u = _points(name, 2, seed=11)
    integ.set("x", x[0])
    integ.set("u", u[0])
    assert integ.solve() == 0
    xn, S, Sx, Su = integ.get("x"), integ.get("S_forw"), integ.get("Sx"), integ.get("Su")
    assert xn.shape == (14,) and S.shape == (14, 16) and Sx.shape == (14, 14) and Su.shape == (14, 2)
    assert np.array_equal(Sx, S[:, :14]) and np.array_equal(Su, S[:, 14:])
    xo, So = _oracle(oracle, 2, Tf / N, 3, x[:1], u[:1])
    assert _close(xn, xo[0])[0] and _close(S, So[0])[0]
    # simulate(x, u): set, solve, x_next; fresh arrays
    assert np.array_equal(integ.simulate(x[0], u[0]), xn)
    xn[:] = 0.0
    assert not np.array_equal(integ.get("x"), xn)
    x1 = integ.simulate(x[1], u[1])
    assert _close(x1, _oracle(oracle, 2, Tf / N, 3, x[1:], u[1:])[0][0])[0]
    # T at run time
    integ.set("T", 0.1)
    assert _close(integ.simulate(x[0], u[0]), _oracle(oracle, 2, 0.1, 3, x[:1], u[:1])[0][0])[0]
    with pytest.raises(Exception, match="mismatching dimension"):
        integ.set("x", np.zeros(13))
    with pytest.raises(Exception, match="mismatching dimension"):
        integ.set("u", np.zeros(3))
    integ.set("p", np.zeros(8))   # (np = 2K; the dynamics read no parameter)
    # the same integrator from an AcadosSim
    sim = AcadosSim()
    sim.model = ocp.model
    sim.solver_options.T, sim.solver_options.num_steps = Tf / N, 3
    assert np.array_equal(AcadosSimSolver(sim).simulate(x[0], u[0]), AcadosSimSolver(ocp).simulate(x[0], u[0]))


def test_batch_faces():
    name = "usv_model_guidance_ca1"
    x, u = _points(name, 64, seed=3)
    s = BatchSimSolver(_sim(name, 0.05, 2), 64)
    s.set("x", x)
    s.set("u", u[0])   # one vector for every instance
    s.solve()
    xa = s.get("x")
    s.set("u", np.tile(u[0], (64, 1)))
    s.solve()
    assert np.array_equal(xa, s.get("x"))
    assert all(s.device_ptr(f) for f in ("x", "u", "x_next", "S_forw"))
    with pytest.raises(Exception, match="mismatching dimension"):
        s.set("x", np.zeros((63, 8)))
    import torch
    st = torch.cuda.Stream()
    s.set_stream(st.cuda_stream)
    s.solve()
    assert np.array_equal(xa, s.get("x"))
    s.close()


def test_symbolic_model_runs_its_generated_library(oracle):
    name, N, K = "usv_model_guidance_ca1", 20, 8
    ocp = usv_models.make_ocp(name, N * 0.05, N, K, symbolic=True)
    x, u = _points(name, 257, seed=21)
    for steps in (1, 10):
        ocp.solver_options.sim_method_num_steps = steps
        s = BatchSimSolver(ocp, 257)
        assert s.generated and s.model_id == 3
        s.set("x", x)
        s.set("u", u)
        s.solve()
        xo, So = _oracle(oracle, 1, 0.05, steps, x, u)
        ok_x, ex = _close(s.get("x"), xo)
        ok_s, es = _close(s.get("S_forw"), So)
        assert ok_x and ok_s, (steps, ex, es)
        s.close()
    assert _close(AcadosSimSolver(ocp).simulate(x[0], u[0]), xo[0])[0]


def _ocp_batch(name, B, seed=31):
    N, K = 20, 6
    wl = scenario.make_bench_batch(name, N, K, B, seed=seed)
    ocp = usv_models.make_ocp(name, N * scenario.BENCH_DT, N, K)
    ocp.solver_options.sim_method_num_steps = scenario.BENCH_SIM_STEPS[name]
    return wl, ocp


@pytest.mark.parametrize("name", ["usv_model_guidance_ca1", "usv_model_pf_ca"])
def test_advance_sim_with_no_noise_is_the_integrator(name):
    B = 96
    wl, ocp = _ocp_batch(name, B)
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, wl)
    s.solve()
    x0, u0 = s.get("x0", 0), s.get("u", 0)
    sim = _sim(name, 0.05, 10, sens=False)
    plant = BatchSimSolver(sim, B)
    s.advance_sim(plant)
    s.sync()
    plant.set("x", x0)
    plant.set("u", u0)
    plant.solve()
    assert np.array_equal(s.get("x0", 0), plant.get("x"))
    # the noise lands on the masked states only
    s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
    s.set("x0", 0, x0)
    s.advance_sim(plant, sigma=1e-3, seed=4)
    s.sync()
    d = s.get("x0", 0) - plant.get("x")
    mask = np.array([(scenario.NOISE_MASK[name] >> j) & 1 for j in range(d.shape[1])], dtype=bool)
    assert np.all(d[:, ~mask] == 0.0) and 0.5e-3 < d[:, mask].std() < 2e-3
    plant.close()
    s.close()


@pytest.mark.parametrize("step", ["advance", "advance_sim"])
def test_halves_with_instance_offsets_reproduce_the_whole_batch(step):
    name, B = "usv_model_pf_ca", 128
    wl, ocp = _ocp_batch(name, B, seed=41)

    def run(w, n, offset):
        s = BatchOcpSolver(ocp, n)
        scenario.load_into(s, w)
        s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
        if offset is not None:
            s.set_option("instance_offset", offset)
        plant = BatchSimSolver(_sim(name, 0.05, 4, sens=False), n)
        for t in range(3):
            s.solve()
            if step == "advance":
                s.advance(1e-3, seed=7 + t)
            else:
                s.advance_sim(plant, sigma=1e-3, seed=7 + t)
        s.sync()
        out = (s.get("x0", 0), s.get_all("x"), s.get_all("u"), s.get_int("status"))
        plant.close()
        s.close()
        return out

    whole = run(wl, B, None)
    halves = [run(sharding.split_workload(wl, 2, r), B // 2, sharding.shard_bounds(B, 2, r)[0]) for r in range(2)]
    for i in range(4):
        assert np.array_equal(np.concatenate([halves[0][i], halves[1][i]], axis=0), whole[i]), (step, i)
    # without the offset the second half draws the first half's noise
    second = run(sharding.split_workload(wl, 2, 1), B // 2, None)
    assert not np.array_equal(second[0], halves[1][0])


def test_advance_sim_refuses_a_foreign_plant():
    wl, ocp = _ocp_batch("usv_model_pf_ca", 8)
    s = BatchOcpSolver(ocp, 8)
    other = BatchSimSolver(_sim("usv_model_guidance_ca1", 0.05, 1), 8)
    with pytest.raises(Exception, match="differs"):
        s.advance_sim(other)
    gocp = usv_models.make_ocp("usv_model_guidance_ca1", 1.0, 20, 8, symbolic=True)
    h1 = BatchOcpSolver(usv_models.make_ocp("usv_model_guidance_ca1", 1.0, 20, 8), 8)
    gen = BatchSimSolver(gocp, 8)
    with pytest.raises(Exception, match="another solver library"):
        h1.advance_sim(gen)
    with pytest.raises(Exception, match="instance_offset"):
        s.set_option("instance_offset", -1)
    import torch
    if torch.cuda.device_count() > 1:
        far = BatchSimSolver(_sim("usv_model_pf_ca", 0.05, 1), 8, device=1)
        with pytest.raises(Exception, match="device"):
            s.advance_sim(far)
        far.close()
    for o in (other, gen, h1, s):
        o.close()


def test_closed_loop_guidance_ca1_reference_scenario_with_a_finer_plant(oracle):
    """scripts/usv_guidance_ca1/main.py protocol (N = 100, Tf = 5, obstacles of r = 1.5 at (4, 4), (4, 7), (4, 12), (4, 20);
    tests/test_oracle_qp.py runs it with the controller's own prediction as plant) with a plant that integrates each 0.05 s period in
    10 RK4 steps instead of the controller's one, through usvmpc_advance_sim.  Status 0 on every tick; the loop is the oracle's loop
    with the oracle's 10-step plant (erk_sens) tick by tick; and the clearance stays inside the soft rows' margin that
    tests/test_guidance.py's sweep asserts (never deeper than 0.3 m into a circle).  The 0.15 m of the prediction-plant loop does not
    hold here, on the oracle either: with this plant the vessel takes another line past the second obstacle, 0.12 m inside its circle
    (the rows are soft: an L1 penalty, not a wall)."""
    N, Tf, K, ticks = 100, 5.0, 8, 300
    ocp = usv_models.make_ocp("usv_model_guidance_ca1", Tf, N, K)
    s = BatchOcpSolver(ocp, 1)
    ak = np.arctan2(30.0, 0.0)
    obs = [(4, 4), (4, 7.0), (4, 12), (4, 20)]
    pobs, robs = np.ones(16) * 100, np.zeros(8)
    for i, (ox, oy) in enumerate(obs):
        pobs[2 * i], pobs[2 * i + 1], robs[i] = ox, oy, 1.5
    x0 = np.array([0.7, 0, 4.0, -ak, -ak, 0, 0, 0])
    s.set_all("x", np.zeros((1, N + 1, 8)))
    s.set_all("u", np.zeros((1, N, 1)))
    s.set("x0", 0, x0)
    s.set_all("yref", np.zeros((1, N, 9)))
    s.set("yref", N, np.zeros(8))
    s.set_all("p", np.tile(pobs, (1, N + 1, 1)))
    s.set_all("lh", np.tile(robs, (1, N, 1)))
    plant = BatchSimSolver(_sim("usv_model_guidance_ca1", Tf / N, 10, sens=False), 1)
    spec = oracle.spec(1, N, Tf, K)
    xo, uo, x0o = np.zeros((N + 1, 8)), np.zeros((N, 1)), x0.copy()
    p, lh, yref, yref_e = np.tile(pobs, (N + 1, 1)), np.tile(robs, (N, 1)), np.zeros((N, 9)), np.zeros(8)
    clear, worst = [], 0.0
    for i in range(ticks):
        st = s.solve()
        assert st[0] == 0, i
        x = s.get("x0", 0)[0]
        worst = max(worst, np.abs(x - x0o).max())
        clear.append(min(np.hypot(x[5] - ox, x[6] - oy) - 1.5 for ox, oy in obs))
        s.advance_sim(plant)
        r = oracle.rti(spec, xo, uo, x0o, yref, yref_e, p, lh)
        assert r["status"] == 0, i
        xo, uo = r["x"], r["u"]
        x0o = oracle.erk_sens(1, Tf / N, 10, xo[0], uo[0])[0]
    x = s.get("x0", 0)[0]
    assert worst <= 1e-6, worst
    assert min(clear) > -0.3, min(clear)
    assert min(clear) < 0.3              # the path really passes the obstacles
    assert x[6] > 5.0, x                 # 15 s at 0.7 m/s along the leg
    plant.close()
    s.close()


def test_scenario_sweep_with_a_finer_plant():
    """examples/scenario_sweep.py --plant-steps 10: the invariants of tests/test_guidance.py's sweep with the plant integrated in 10 steps"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("scenario_sweep", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "scenario_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.run(B=96, ticks=400, N=100, quiet=True, plant_steps=10)
    assert not r["solver_failures"].any()
    mc = r["min_clearance"]
    assert np.median(mc) > 0.17 and np.percentile(mc, 5) > 0.1 and mc.min() > -0.3
    assert (r["final_pose"][:, 1] > 5.0).all()
