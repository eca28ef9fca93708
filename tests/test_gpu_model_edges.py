"""The device's model arithmetic at the edges of its range against the 40-digit reference of tests/model_ref.py, on a real MI355X
(`pytest -m gpu`): lanes::frcp / lanes::frsqrt in ulp, f and J of the three models pointwise in every regime (usvmpc_debug_model_eval)
and inside an interval (usvmpc_debug_model_eval_from: ModelM2's series over d = psi - psi0, its seam and its fallback), the obstacle
rows (usvmpc_debug_obstacle_eval), and the integrator with sensitivities (BatchSimSolver) - hand-written models and the generated
library.

Rule of comparison: statistic E (tests/model_ref.py stat_E) of the device against the reference must not exceed E of the CPU oracle on
the same points, computed in the same run, times a margin.  The margins (MARGIN below) were set once from the MI355X run recorded in
profiles/model_edges.txt, which holds the measured E of both: the measured ratio device / oracle rounded up to the next power of two,
at most 8; an entry that is absent is 1.  They exist because lanes::frsqrt rounds to within about 2 ulp where the oracle's square
root rounds to half an ulp, and because the device contracts into FMAs where the oracle does not."""
import math

import mpmath
import numpy as np
import pytest

from mpc_collisionavoidance_amd import _capi, usv_models
from mpc_collisionavoidance_amd.acados_template import AcadosSim, BatchSimSolver
from tests import model_ref as R
from tests.test_model_edges import MODEL_REGIMES, obstacle_cases, obstacle_ref, oracle_integ, oracle_pointwise, stat_rel

pytestmark = pytest.mark.gpu

# measured ratio device / oracle, rounded up to the next power of two (profiles/model_edges.txt); absent: 1
MARGIN = {
    "point/usv_model/switch/f": 2,
    "point/usv_model/switch/J": 2,
    "point/usv_model/turning/J": 4,
    "point/usv_model_guidance_ca1/reversing/J": 4,
    "point/usv_model_pf_ca/reversing/J": 2,
    "sweep/psi0=0/f": 2,
    "sweep/psi0=0/J": 4,
    "sweep/psi0=0.75/f": 2,
    "obstacle/K=1": 2,
    "integ/usv_model/fast/S/steps=1": 2,
    "integ/usv_model/reversing/x_next/steps=1": 2,
    "integ/usv_model/reversing/x_next/steps=4": 4,
    "integ/usv_model/turning/S/steps=4": 8,
    "integ/usv_model_guidance_ca1/reversing/x_next/steps=4": 4,
    "integ/usv_model_guidance_ca1/slow/S/steps=4": 2,
    "integ/usv_model_guidance_ca1/far_heading/x_next/steps=4": 2,
    "integ/usv_model_pf_ca/fast/S/steps=1": 4,
    "integ/usv_model_pf_ca/fast/x_next/steps=4": 2,
    "integ/usv_model_pf_ca/fast/S/steps=4": 2,
    "integ/usv_model_pf_ca/switch/x_next/steps=1": 2,
    "integ/usv_model_pf_ca/switch/S/steps=4": 2,
    "integ/usv_model_pf_ca/reversing/x_next/steps=4": 2,
    "integ/usv_model_pf_ca/reversing/S/steps=4": 2,
    "integ/usv_model_pf_ca/turning/x_next/steps=4": 2,
    "generated/usv_model_guidance_ca1/reversing/S/steps=1": 2,
    "generated/usv_model_guidance_ca1/reversing/x_next/steps=4": 4,
    "generated/usv_model_guidance_ca1/reversing/S/steps=4": 2,
    "generated/usv_model_guidance_ca1/slow/S/steps=4": 2,
    "generated/usv_model_guidance_ca1/far_heading/x_next/steps=4": 2,
}
# lanes::frcp / lanes::frsqrt: the measured maximum over the normal-range operands, rounded up to a whole ulp
FAST_MATH_ULP = {"frcp": 1, "frsqrt": 1}      # (measured: 0.500 and 0.942)


def _dp(a):
    return a.ctypes.data_as(_capi._dp)


def _check(lines, key, e_dev, e_orc):
    """one comparison: record it, return whether the device is within the oracle's E times the key's margin"""
    margin = MARGIN.get(key, 1)
    assert margin in (1, 2, 4, 8)
    ratio = e_dev / e_orc if e_orc > 0 else (0.0 if e_dev == 0 else math.inf)
    ok = e_dev <= e_orc * margin
    lines.append("%-58s device %.2e  oracle %.2e  ratio %6.2f  margin %d%s" % (key, e_dev, e_orc, ratio, margin, "" if ok else "  EXCEEDED"))
    return ok


def device_eval(m, x, U, x_start=None):
    L = _capi.lib()
    x, U = np.ascontiguousarray(x), np.ascontiguousarray(U)
    n, (nx, nu) = x.shape[0], R.DIMS[m]
    f, J = np.zeros((n, nx)), np.zeros((n, nx, nu + nx))
    if x_start is None:
        rc = L.usvmpc_debug_model_eval(m, 0, n, _dp(x), _dp(U), _dp(f), _dp(J))
    else:
        xs = np.ascontiguousarray(x_start)
        rc = L.usvmpc_debug_model_eval_from(m, 0, n, _dp(xs), _dp(x), _dp(U), _dp(f), _dp(J))
    assert rc == 0
    return f, J


# ------------------------------------------------------------------ frcp / frsqrt
def _operands():
    rng = np.random.default_rng(4096)
    x = [10.0 ** rng.uniform(-300, 300, 4096)]
    # the edges of two adjacent binades (the rsq estimate depends on the exponent's parity) and their neighbours in double
    x.append(np.array([f(e) for e in (1.0, 2.0, 4.0) for f in (lambda e: np.nextafter(e, 0), lambda e: e, lambda e: np.nextafter(e, 8))]))
    x.append(np.linspace(1.0, 4.0, 97))
    k = np.arange(1, 65, dtype=float)
    x.append(k * k)                                         # exact squares
    x.append((k * k) * 2.0 ** -40)
    x.append((3.0 * 2.0 ** 20 + k) ** 2)
    return np.ascontiguousarray(np.concatenate(x))


def _ulp_err(a, ref):
    return np.array([float(abs(mpmath.mpf(float(p)) - q)) / np.spacing(abs(float(q))) for p, q in zip(a, ref)])


def test_fast_reciprocal_and_reciprocal_square_root_in_ulp():
    """lanes::frcp and lanes::frsqrt (hardware estimate + two Newton steps) against mpmath over 4096 operands log-uniform in
    1e-300 .. 1e300, the edges of the binades [1, 2) and [2, 4) with their neighbours, and exact squares.  Two Newton steps from an
    estimate of about 26 bits leave rounding only: the header's "full FP64 accuracy" means at most FAST_MATH_ULP ulp, the measured
    maximum rounded up (profiles/model_edges.txt).  0, inf, NaN, negative operands and subnormals are recorded there, not bounded."""
    L = _capi.lib()
    x = _operands()
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -4.0, 5e-324, 1e-310, 2.0 ** -1022, np.finfo(float).max])
    xs = np.ascontiguousarray(np.concatenate([x, special]))
    rcp, rsq = np.zeros_like(xs), np.zeros_like(xs)
    assert L.usvmpc_debug_fast_math(0, len(xs), _dp(xs), _dp(rcp), _dp(rsq)) == 0
    with mpmath.workdps(R.DPS):
        e_rcp = _ulp_err(rcp[:len(x)], [1 / mpmath.mpf(float(v)) for v in x])
        e_rsq = _ulp_err(rsq[:len(x)], [1 / mpmath.sqrt(mpmath.mpf(float(v))) for v in x])
    lines = ["frcp   max %.3f ulp at x = %r   (%d operands)" % (e_rcp.max(), float(x[e_rcp.argmax()]), len(x)),
             "frsqrt max %.3f ulp at x = %r" % (e_rsq.max(), float(x[e_rsq.argmax()])),
             "exact squares k^2, k = 1 .. 64: frsqrt max %.3f ulp" % e_rsq[-192:-128].max()]
    lines += ["x = %-24r frcp %-24r frsqrt %r" % (float(v), float(a), float(b)) for v, a, b in zip(special, rcp[len(x):], rsq[len(x):])]
    R.report("lanes::frcp / lanes::frsqrt on the MI355X against mpmath", lines)
    assert np.isfinite(rcp[:len(x)]).all() and np.isfinite(rsq[:len(x)]).all()
    assert e_rcp.max() <= FAST_MATH_ULP["frcp"] and e_rsq.max() <= FAST_MATH_ULP["frsqrt"], (e_rcp.max(), e_rsq.max())


# ------------------------------------------------------------------ f and J pointwise
@pytest.mark.parametrize("m,reg", MODEL_REGIMES)
def test_pointwise_f_and_J(oracle, m, reg):
    x, U = R.points(m, reg)
    fr, Jr = R.point_ref(m, reg)
    fo, Jo = oracle_pointwise(oracle, m, x, U)
    fd, Jd = device_eval(m, x, U)
    lines, ok = [], True
    for out, d, o, r in (("f", fd, fo, fr), ("J", Jd, Jo, Jr)):
        ok &= _check(lines, "point/%s/%s/%s" % (R.NAMES[m], reg, out), R.stat_E(d, r), R.stat_E(o, r))
    if m != 2:
        # (no preparation: the evaluation inside an interval is the same code)
        f2, J2 = device_eval(m, x, U, x_start=x[::-1])
        assert np.array_equal(f2, fd) and np.array_equal(J2, Jd)
    R.report("device f, J pointwise: %s, %s" % (R.NAMES[m], reg), lines)
    assert ok, lines


def test_series_sweep_inside_an_interval(oracle):
    """ModelM2 prepared at x_start and evaluated at d = psi - psi0 over [-0.3, 0.3] (tests/model_ref.py sweep_points: the series, the
    seam |d| = 0.125 with its neighbours in double, the library fallback), per base heading; the oracle evaluates the same points
    with the library's sine and cosine"""
    xs, xx, uu = R.sweep_points()
    fr, Jr = R.sweep_ref()
    fo, Jo = oracle_pointwise(oracle, 2, xx, uu)
    fd, Jd = device_eval(2, xx, uu, x_start=xs)
    n = len(xx) // 3
    lines, ok = [], True
    for b in range(3):
        sl = slice(b * n, (b + 1) * n)
        for out, d, o, r in (("f", fd, fo, fr), ("J", Jd, Jo, Jr)):
            ok &= _check(lines, "sweep/psi0=%g/%s" % (xs[b * n, 0], out), R.stat_E(d[sl], r[sl]), R.stat_E(o[sl], r[sl]))
    # at d == 0 the series returns sin / cos(psi0) themselves: the same bits as the evaluation prepared at the point
    z = xx[:, 0] == xs[:, 0]
    f0, J0 = device_eval(2, xx[z], uu[z])
    assert z.sum() == 3 and np.array_equal(f0, fd[z]) and np.array_equal(J0, Jd[z])
    R.report("device f, J of usv_model_pf_ca inside an interval (d sweep)", lines)
    assert ok, lines


# ------------------------------------------------------------------ obstacle rows
@pytest.mark.parametrize("K", [1, 32])
def test_obstacle_rows(oracle, K):
    """obs_dist (d = d2 * frsqrt(d2), gradient (dx, dy) * frsqrt(d2)) at distances 1e-9 .. 1e7 m, all quadrants and both axes; per
    entry relative error, since the distances span sixteen decades"""
    pos, p = obstacle_cases(K)
    n = len(pos)
    ref = obstacle_ref(pos, p)
    ho = np.array([np.column_stack(oracle.model_h(1, np.r_[np.zeros(5), pos[i], 0.0], p[i])) for i in range(n)])
    h, grad = np.zeros((n, K)), np.zeros((n, K, 2))
    assert _capi.lib().usvmpc_debug_obstacle_eval(0, n, K, _dp(pos), _dp(p), _dp(h), _dp(grad)) == 0
    hd = np.concatenate([h[:, :, None], grad], axis=2)
    lines = []
    ok = _check(lines, "obstacle/K=%d" % K, stat_rel(hd, ref), stat_rel(ho, ref))
    R.report("device obstacle rows, K = %d" % K, lines)
    assert ok, lines


# ------------------------------------------------------------------ the integrator
def _sim(name, steps, sens):
    sim = AcadosSim()
    sim.model = usv_models.make_ocp(name, 1.0, 20).model
    sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = R.T_INT, steps, sens
    return sim


def _run(solver, x, U, sens=True):
    solver.set("x", x)
    solver.set("u", U)
    assert solver.solve() == 0
    out = (solver.get("x"), solver.get("S_forw") if sens else None)
    solver.close()
    return out


def _integ_case(oracle, m, reg, make, tag, sens_off):
    x, U, ref = R.integ_points(m, reg)
    B = len(x)
    assert B % 16 != 0
    lines, ok = [], True
    for steps in R.STEPS:
        xo, So = oracle_integ(oracle, m, x, U, steps)
        xd, Sd = _run(make(steps, True, B), x, U)
        for out, d, o, r in (("x_next", xd, xo, ref[steps][0]), ("S", Sd, So, ref[steps][1])):
            ok &= _check(lines, "%s/%s/%s/%s/steps=%d" % (tag, R.NAMES[m], reg, out, steps), R.stat_E(d, r), R.stat_E(o, r))
        if sens_off:
            xn, _ = _run(make(steps, False, B), x, U, sens=False)
            assert np.array_equal(xn, xd), (m, reg, steps)      # x_next is the same bits with sens_forw off
    R.report("device integrator (%s), T = %g: %s, %s" % (tag, R.T_INT, R.NAMES[m], reg), lines)
    assert ok, lines


@pytest.mark.parametrize("m,reg", MODEL_REGIMES)
def test_integrator_with_sensitivities(oracle, m, reg):
    def make(steps, sens, B):
        return BatchSimSolver(_sim(R.NAMES[m], steps, sens), B)
    _integ_case(oracle, m, reg, make, "integ", True)


@pytest.mark.parametrize("reg", ["reversing", "slow", "far_heading"])
def test_integrator_of_the_generated_library(oracle, reg):
    """usv_model_guidance_ca1 from its symbolic definition (the generated solver library)"""
    def make(steps, sens, B):
        ocp = usv_models.make_ocp("usv_model_guidance_ca1", 20 * R.T_INT, 20, 8, symbolic=True)
        ocp.solver_options.sim_method_num_steps = steps
        s = BatchSimSolver(ocp, B)
        assert s.generated and s.model_id == 3
        return s
    _integ_case(oracle, 1, reg, make, "generated", False)
