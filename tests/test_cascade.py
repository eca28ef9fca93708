"""The two-layer control stack without a device: the low-level OCP usv_model_low_level through the symbolic route (analysis, generated
kernels on the lane emulator against the oracle's generated-model hook), and the coupling arithmetic of csrc/cascade.hpp compiled with
the host compiler (tests/cascade_harness.cpp, a stand-alone program; built a second time with -fsanitize=address,undefined and run as a
program) against the numpy restatement in mpc_collisionavoidance_amd/scenario.py.

Rules of comparison: copied entries bit for bit; sines and cosines within 8 * 2^-52, the project's allowance for two maths libraries
(scenario.ca_fleet_world); a plant period within tests/test_gpu_sim.py's _close rule, 1e-12 relative with a floor of 1e-12."""
import os
import subprocess

import numpy as np
import pytest

from mpc_collisionavoidance_amd import _capi, codegen, genbuild, scenario, usv_models
from tests import util
from tests.test_emu_kernels import emu_rti
from tests.test_gpu_sim import _close
from tests.test_symbolic import _emu_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
WORK = os.path.join(CSRC, "gen")
TRIG = 8 * 2.0 ** -52
NPTS = 257


def ll_workload(N, B, rng, u_lo=0.3, u_hi=1.0):
    """B low-level problems: a vessel under way, thrusts 0 .. 10, a heading step of up to 0.8 rad and u_des = 0.7"""
    psi = rng.uniform(-3.0, 3.0, B)
    s = np.column_stack([np.zeros(B), np.zeros(B), psi, rng.uniform(u_lo, u_hi, B), rng.uniform(-0.05, 0.05, B), rng.uniform(-0.1, 0.1, B)])
    x0, row = scenario.cascade_ll_inputs(s, rng.uniform(0.0, 10.0, (B, 2)), psi + rng.uniform(-0.8, 0.8, B), np.full(B, 0.7))
    return dict(x0=x0, yref=np.ascontiguousarray(np.tile(row[:, None, :], (1, N, 1))), yref_e=np.ascontiguousarray(row[:, :8]),
                p=np.zeros((B, N + 1, 0)), lh=np.zeros((B, N, 0)), x_init=np.ascontiguousarray(np.tile(x0[:, None, :], (1, N + 1, 1))),
                u_init=np.zeros((B, N, 2)), K=0)


# ------------------------------------------------------------------ the low-level OCP
def test_low_level_ocp_as_the_issue_states_it():
    ocp = usv_models.make_ocp("usv_model_low_level", 1.0, 100)
    info = codegen.analyse(ocp.model)
    assert (info.nx, info.nu, info.K) == (8, 2, 0)
    assert ocp.model.name == "usv_model_low_level" and ocp.solver_options.model_source == "symbolic"
    assert np.array_equal(np.diag(ocp.cost.W), [0, .1, .1, .1, 0, 0, 1e-7, 0, 0, 0]) and np.count_nonzero(ocp.cost.W) == 4
    assert np.array_equal(np.diag(ocp.cost.W_e), [0, .05, .05, .1, 0, 0, 1e-6, 0])
    assert ocp.cost.Vu[8, 0] == 1 and ocp.cost.Vu[9, 1] == 1 and np.count_nonzero(ocp.cost.Vu) == 2
    assert list(ocp.constraints.idxbx) == [3, 4, 5, 6, 7]
    assert list(ocp.constraints.lbx) == [-2, -2, -10, -30, -30] and list(ocp.constraints.ubx) == [2, 2, 10, 35, 35]
    assert list(ocp.constraints.lbu) == [-30, -30] and list(ocp.constraints.ubu) == [30, 30]
    assert list(ocp.constraints.x0) == [0, 0, 1, 0.001, 0, 0, 0, 0]
    so = ocp.solver_options
    assert (so.nlp_solver_type, so.hessian_approx, so.integrator_type) == ("SQP_RTI", "GAUSS_NEWTON", "ERK")
    assert usv_models.ocp_low_level(1.0, 100)[1].name == "usv_model_low_level"
    # the dynamics at a point on either side of the u > 1.25 branch, against the numpy restatement of the 3-DOF block
    from mpc_collisionavoidance_amd import casadi_lite as ca
    for u in (0.9, 1.4):
        x = np.array([0.3, 0.1, 0.2, u, 0.04, -0.07, 6.0, 4.0])
        U = np.array([1.5, -2.5])
        f = ca.evaluate(info.f, {**dict(zip(info.x, x)), **dict(zip(info.u, U))})
        fu, fv, fr = scenario._dof3(0.78, x[3], x[4], x[5], x[6], x[7])
        want = [x[5], np.cos(x[0]) * x[5], -np.sin(x[0]) * x[5], fu, fv, fr, U[0], U[1] / 0.78]
        assert np.allclose(f, want, rtol=1e-14, atol=1e-14)


def test_low_level_kernels_on_the_emulator_against_the_oracle_hook(oracle):
    N, B = 8, 3
    ocp = usv_models.make_ocp("usv_model_low_level", N * 0.01, N)
    wl = ll_workload(N, B, np.random.default_rng(2))
    info = codegen.analyse(ocp.model)
    os.makedirs(WORK, exist_ok=True)
    oracle.register_generated(codegen.emit_oracle_c(info), WORK)
    spec = oracle.spec_from_ocp(ocp, oracle.MGEN)
    gen = _emu_lib(genbuild.build_emu_lib(info, 0, False, EMU))
    desc = _capi.desc_from_ocp(ocp, batch=B, generated=True)
    xe, ue, xo, uo = wl["x_init"], wl["u_init"], wl["x_init"].copy(), wl["u_init"].copy()
    for it in range(3):
        r = emu_rti(gen, desc, wl, xe, ue)
        xe, ue = r["x"], r["u"]
        xo, uo, sto, ito = util.oracle_rti(oracle, spec, wl, xo, uo)
        assert np.array_equal(r["status"], sto) and (sto == 0).all()
        assert util.rel_err(xe, xo) < 1e-8 and util.rel_err(ue, uo) < 1e-8


# ------------------------------------------------------------------ cascade.hpp through its harness
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off"] + extra +
                          ["-I" + EMU, "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cascade_harness.cpp")])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """(plain build, sanitized build): every case runs through both and their outputs must be the same bytes"""
    tmp = tmp_path_factory.mktemp("cascade")
    return _build(tmp, "cascade_harness", []), _build(tmp, "cascade_harness_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def call(harness, tmp_path, mode, records, nout):
    rec = np.ascontiguousarray(records, dtype=np.float64)
    fin = str(tmp_path / "in.bin")
    rec.tofile(fin)
    outs = []
    for i, exe in enumerate(harness):
        fout = str(tmp_path / ("out%d.bin" % i))
        r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok %d" % rec.shape[0], r.stdout + r.stderr
        outs.append(np.fromfile(fout).reshape(rec.shape[0], nout))
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


def _points(rng, n=NPTS):
    s = np.column_stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-3.2, 3.2, n), rng.uniform(-0.2, 1.6, n),
                         rng.uniform(-0.1, 0.1, n), rng.uniform(-0.5, 0.5, n)])
    s[::9, 3] = 0.0                                      # u == 0 -> 0.001
    s[1::9, 3] = rng.uniform(1.26, 1.6, len(s[1::9]))    # the fast branch of the surge damping
    return s


def test_low_level_inputs_are_numpys(harness, tmp_path):
    rng = np.random.default_rng(11)
    s, past = _points(rng), rng.uniform(-30, 35, (NPTS, 2))
    psi_des, u_des = rng.uniform(-3.2, 3.2, NPTS), np.where(np.arange(NPTS) % 4 == 0, 0.0, 0.7)
    got = call(harness, tmp_path, "inputs", np.column_stack([s, past, psi_des, u_des]), 18)
    x0, row = scenario.cascade_ll_inputs(s, past, psi_des, u_des)
    for j in (0, 3, 4, 5, 6, 7):                         # psi, u, v, r, past thrusts: copies
        assert got[:, j].tobytes() == x0[:, j].tobytes(), j
    assert (got[::9, 3] == 0.001).all() and (s[::9, 3] == 0.0).all()
    assert got[:, 3][s[:, 3] != 0.0].tobytes() == s[:, 3][s[:, 3] != 0.0].tobytes()
    assert np.abs(got[:, 1:3] - x0[:, 1:3]).max() <= TRIG
    for j in (0, 3):                                     # psi_des, u_des: copies; the rest of the row is zero
        assert got[:, 8 + j].tobytes() == row[:, j].tobytes(), j
    assert np.abs(got[:, 9:11] - row[:, 1:3]).max() <= TRIG
    assert (got[:, 12:] == 0.0).all() and not np.signbit(got[:, 12:]).any()


def test_low_level_outputs_are_numpys(harness, tmp_path):
    rng = np.random.default_rng(12)
    s = _points(rng)
    x1 = rng.uniform(-30, 35, (NPTS, 8))
    psi_des, u_des = rng.uniform(-3.2, 3.2, NPTS), np.where(np.arange(NPTS) % 4 == 0, 0.0, 0.7)
    got = call(harness, tmp_path, "outputs", np.column_stack([x1, psi_des, u_des, s[:, 2], s[:, 3]]), 6)
    thr, past, eu, epsi = scenario.cascade_ll_outputs(x1, psi_des, u_des, s)
    assert got[:, 0:2].tobytes() == thr.tobytes() and got[:, 2:4].tobytes() == past.tobytes()
    stop = u_des == 0.0
    assert stop.any() and (got[stop, 0:2] == 0.0).all() and got[stop, 2:4].tobytes() == x1[stop, 6:8].tobytes()   # zero thrust, past_T follows x1
    assert got[~stop, 0:2].tobytes() == x1[~stop, 6:8].tobytes()
    assert got[:, 4].astype(np.float32).tobytes() == eu.tobytes() and got[:, 5].astype(np.float32).tobytes() == epsi.tobytes()
    assert (got[:, 4] == got[:, 4].astype(np.float32)).all()                                                       # rounded through float


@pytest.mark.parametrize("steps", [1, 3])
def test_plant_period_is_numpys(harness, tmp_path, steps):
    rng = np.random.default_rng(13 + steps)
    s = _points(rng)
    thr = rng.uniform(-30, 35, (NPTS, 2))
    thr[::5] = 0.0
    c = np.where(np.arange(NPTS) % 3 == 0, 1.0, 0.78)
    T = 0.01
    got = call(harness, tmp_path, "plant", np.column_stack([s, thr, c, np.full(NPTS, T), np.full(NPTS, float(steps))]), 6)
    want = np.empty_like(got)
    for cv in (1.0, 0.78):
        want[c == cv] = scenario.cascade_plant_step(s[c == cv], thr[c == cv], T, steps, cv)
    assert (s[:, 3] > 1.25).any() and (s[:, 3] == 0.0).any()
    ok, err = _close(got, want)
    assert ok, err
    assert np.abs(got - s).max() > 1e-4                  # (the period moves the state)


def test_setpoints_are_compared_bit_for_bit(harness, tmp_path):
    rec = [[-1.0, -1.0, 0.0, 0.0],        # nothing written yet: always due
           [0.3, 0.7, 0.3, 0.7],
           [0.3, 0.7, np.nextafter(0.3, 1.0), 0.7],
           [0.3, 0.7, 0.3, 0.0],
           [0.0, 0.0, -0.0, 0.0],         # the bits differ
           [0.0, 0.0, 0.0, 0.0]]
    assert list(call(harness, tmp_path, "changed", rec, 1)[:, 0]) == [1, 0, 1, 1, 1, 0]


def test_tick_logic(harness, tmp_path):
    rec = [[t, r] for r in (5, 1, 3) for t in range(13)]
    got = call(harness, tmp_path, "ticks", rec, 2)
    for (t, r), (g, h) in zip(rec, got):
        assert bool(g) == scenario.cascade_guidance_tick(t, r) == (t % r == 0)
        assert bool(h) == scenario.cascade_hands_over(t, r) == ((t + 1) % r == 0)
    r5 = got[:13]
    assert [t for t in range(13) if r5[t, 0]] == [0, 5, 10]          # guidance ticks at ratio 5 ...
    assert [t for t in range(13) if r5[t, 1]] == [4, 9]              # ... and the steps that write the guidance x0 ahead of them
