"""A 40-digit reference of the three models, independent of every double-precision implementation in this tree: the sympy
restatement of the reference's CasADi expressions (_sym_model, also used by tests/test_oracle_models.py), lambdified to mpmath,
with the RK4 map and its forward sensitivities on top; and the table of edge regimes that tests/test_model_edges.py (CPU) and
tests/test_gpu_model_edges.py (MI355X) evaluate.

Derivative conventions are CasADi's, the ones csrc/models.hpp states: d|a| = sign(a) with sign(0) = 0 (sympy's derivative of Abs
of a real symbol, mpmath's sign), each branch of u > 1.25 differentiates itself (sympy's derivative of a Piecewise), and
sqrt(u^2 + v^2) differentiates to a 0/0 at the origin (mpmath raises ZeroDivisionError there: the singular points are handled by
their tests, not here).

Everything is cached per model (functools) so that the CPU and the GPU tests of one run pay for a reference once."""
import functools
import os

import mpmath
import numpy as np
import sympy as sp

DPS = 40
NAMES = ["usv_model", "usv_model_guidance_ca1", "usv_model_pf_ca"]
DIMS = {0: (5, 2), 1: (8, 1), 2: (14, 2)}
IU = {0: 0, 1: 0, 2: 3}            # index of the surge speed u in the state; v follows it, and r (models 0 and 2) follows v
POS = {1: (5, 6), 2: (10, 11)}     # position states of the obstacle rows
KINK_U = 1.25


# ---- sympy restatement of the reference's CasADi expressions
def _dof3_sym(c, u, v, r, Tp, Ts):
    m, Iz, B = 30, sp.Rational(41, 10), sp.Rational(41, 100)
    Xud, Yvd, Yrd, Nvd, Nrd = -2.25, -23.13, -1.31, -16.41, -2.79
    Yvv, Yvr, Nrv, Nrr = -99.99, -5.49, -8.8, -3.49
    Xu = sp.Piecewise((64.55, u > 1.25), (-25, True))
    Xuu = sp.Piecewise((-70.92, u > 1.25), (0, True))
    Yv = 0.5 * (-40 * 1000 * sp.Abs(v)) * (1.1 + 0.0045 * (1.01 / 0.09) - 0.1 * (0.27 / 0.09) + 0.016 * ((0.27 / 0.09) ** 2))
    Nr = (-0.52) * sp.sqrt(u * u + v * v)
    Tu = Tp + c * Ts
    Tr = (Tp - c * Ts) * B / 2
    fu = (Tu - (-m + 2 * Yvd) * v - (Yrd + Nvd) * r * r - (-Xu * u - Xuu * sp.Abs(u) * u)) / (m - Xud)
    fv = (-(m - Xud) * u * r - (-Yv - Yvv * sp.Abs(v) - Yvr * sp.Abs(r)) * v) / (m - Yvd)
    fr = (Tr - (-2 * Yvd * u * v - (Yrd + Nvd) * r * u + Xud * u * r) - (-Nr * r - Nrv * sp.Abs(v) * r - Nrr * sp.Abs(r) * r)) / (Iz - Nrd)
    return fu, fv, fr


def _sym_model(model):
    if model == 0:
        x = sp.symbols("u v r Tp Ts", real=True)
        U = sp.symbols("U0 U1", real=True)
        fu, fv, fr = _dof3_sym(0.78, *x)
        f = [fu, fv, fr, U[0], U[1]]
    elif model == 1:
        x = sp.symbols("u v ye chie psied xned yned psi", real=True)
        U = sp.symbols("U0,", real=True)
        u, v, ye, chie, psied, xned, yned, psi = x
        beta = sp.atan2(v, u + 0.001)
        psie = chie - beta
        f = [0, 0, u * sp.sin(psie) + v * sp.cos(psie), (psied - psie) / 1.0, U[0], u * sp.cos(psi) - v * sp.sin(psi),
             u * sp.sin(psi) + v * sp.cos(psi), (psied - psie) / 1.0]
    else:
        x = sp.symbols("psi sinpsi cospsi u v r ye x1 y1 ak nedx nedy Tp Ts", real=True)
        U = sp.symbols("U0 U1", real=True)
        psi, sinpsi, cospsi, u, v, r, ye, x1, y1, ak, nedx, nedy, Tp, Ts = x
        c = 1.0
        fu, fv, fr = _dof3_sym(c, u, v, r, Tp, Ts)
        chi = psi + sp.atan2(v, u + .001)
        f = [r, sp.cos(chi) * r, -sp.sin(chi) * r, fu, fv, fr,
             -(u * sp.cos(psi) - v * sp.sin(psi)) * sp.sin(ak) + (u * sp.sin(psi) + v * sp.cos(psi)) * sp.cos(ak),
             0, 0, 0, u * sp.cos(psi) - v * sp.sin(psi), u * sp.sin(psi) + v * sp.cos(psi), U[0], U[1] / c]
    f = sp.Matrix(f)
    return x, U, f


# ---- mpmath evaluators at DPS digits
@functools.lru_cache(maxsize=None)
def _evaluators(model):
    """(f(x, U) -> list of nx mpf, J(x, U) -> nx lists of nu + nx mpf with respect to z = [u; x]).  The constants of the expressions
    are the doubles the CasADi graphs hold; everything between them is carried at DPS digits."""
    xs, Us, f = _sym_model(model)
    z = sp.Matrix(list(Us) + list(xs))
    ff = sp.lambdify((xs, Us), list(f), "mpmath", cse=True)
    jj = sp.lambdify((xs, Us), f.jacobian(z).tolist(), "mpmath", cse=True)
    return ff, jj


def _mp(a):
    return [mpmath.mpf(float(v)) for v in np.asarray(a, dtype=float).ravel()]


def f(model, x, u):
    """f(x, u) as nx mpf"""
    with mpmath.workdps(DPS):
        return [mpmath.mpf(v) for v in _evaluators(model)[0](_mp(x), _mp(u))]


def jac(model, x, u):
    """d f / d [u; x] as nx rows of nu + nx mpf (the layout of usvmpc_debug_model_eval's J)"""
    with mpmath.workdps(DPS):
        return [[mpmath.mpf(v) for v in row] for row in _evaluators(model)[1](_mp(x), _mp(u))]


def obstacle_row(px, py, ox, oy):
    """(d, d d/d px, d d/d py) of the reference's obstacle row sqrt((px - ox)^2 + (py - oy)^2), as mpf"""
    with mpmath.workdps(DPS):
        dx, dy = mpmath.mpf(float(px)) - mpmath.mpf(float(ox)), mpmath.mpf(float(py)) - mpmath.mpf(float(oy))
        d = mpmath.sqrt(dx * dx + dy * dy)
        return d, dx / d, dy / d


def to_float(a):
    """mpf (nested lists) -> float64 array, each entry rounded once"""
    return np.array(a, dtype=object).astype(float)


def _kink(model, x):
    if model == 1:
        return mpmath.inf
    i = IU[model]
    return min(abs(x[i] - KINK_U), abs(x[i + 1]), abs(x[i + 2]))


def rk4_sens(model, x, u, T, steps):
    """`steps` classical RK4 steps of T / steps from x under the constant input u, with the forward sensitivities integrated by the same
    scheme (which makes them the exact derivative of the discrete map).  Returns (x_next [nx] mpf, S [nx][nx + nu] mpf in the layout
    of S_forw = [Sx | Su], the smallest distance of any stage point to a kink u = 1.25, v = 0, r = 0 as a float)."""
    nx, nu = DIMS[model]
    ff, jj = _evaluators(model)
    with mpmath.workdps(DPS):
        X, U = _mp(x), _mp(u)
        S = [[mpmath.mpf(1 if j == i else 0) for j in range(nx + nu)] for i in range(nx)]
        dt = mpmath.mpf(float(T)) / int(steps)
        kink = mpmath.inf

        def rhs(Xs, Ss):
            nonlocal kink
            kink = min(kink, _kink(model, Xs))
            fv = ff(Xs, U)
            J = jj(Xs, U)
            dS = []
            for i in range(nx):
                Ji = J[i]
                nz = [(k, Ji[nu + k]) for k in range(nx) if Ji[nu + k] != 0]
                row = []
                for c in range(nx + nu):
                    a = Ji[c - nx] if c >= nx else 0
                    for k, jv in nz:
                        a = a + jv * Ss[k][c]
                    row.append(a)
                dS.append(row)
            return fv, dS

        def axpy(a, dX, dS_):
            return ([X[i] + a * dX[i] for i in range(nx)],
                    [[S[i][c] + a * dS_[i][c] for c in range(nx + nu)] for i in range(nx)])

        for _ in range(int(steps)):
            k1, s1 = rhs(X, S)
            k2, s2 = rhs(*axpy(dt / 2, k1, s1))
            k3, s3 = rhs(*axpy(dt / 2, k2, s2))
            k4, s4 = rhs(*axpy(dt, k3, s3))
            X = [X[i] + dt / 6 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) for i in range(nx)]
            S = [[S[i][c] + dt / 6 * (s1[i][c] + 2 * s2[i][c] + 2 * s3[i][c] + s4[i][c]) for c in range(nx + nu)] for i in range(nx)]
        return [mpmath.mpf(v) for v in X], S, float(kink)


# ---- statistic E
def stat_E(a, r):
    """Statistic E: per entry |a - r| / max(|r|, 2^-10 M_c), M_c the largest |r| of that entry position over the points (first
    axis); the maximum over entries and points.  `r` is the reference rounded to double (its rounding, 2^-53 relative, is far below
    every bound E is compared with) or an object array of mpf; the difference is formed at DPS digits either way.  An entry position
    that is identically zero in the reference must be zero in `a`."""
    a = np.asarray(a, dtype=float)
    ro = np.asarray(r, dtype=object)
    assert a.shape == ro.shape, (a.shape, ro.shape)
    with mpmath.workdps(DPS):
        ro = np.vectorize(lambda v: mpmath.mpf(v), otypes=[object])(ro)
        rabs = np.vectorize(lambda v: float(abs(v)), otypes=[float])(ro)
        M = rabs.max(axis=0, keepdims=True)
        den = np.maximum(rabs, 2.0 ** -10 * M)
        if not np.isfinite(a).all():
            return float("inf")
        diff = np.vectorize(lambda p, q: float(abs(mpmath.mpf(float(p)) - q)), otypes=[float])(a, ro)
    zero = den == 0.0
    if (diff[zero] != 0.0).any():
        return float("inf")
    return float((diff[~zero] / den[~zero]).max()) if (~zero).any() else 0.0


def stat_A(a, r):
    """The error in units of the component's scale: max |a - r| / M_c, M_c as in stat_E (a component that is identically zero in the
    reference must be zero in `a`)"""
    a = np.asarray(a, dtype=float)
    ro = np.asarray(r, dtype=object)
    assert a.shape == ro.shape, (a.shape, ro.shape)
    if not np.isfinite(a).all():
        return float("inf")
    with mpmath.workdps(DPS):
        rabs = np.vectorize(lambda v: float(abs(mpmath.mpf(v))), otypes=[float])(ro)
        diff = np.vectorize(lambda p, q: float(abs(mpmath.mpf(float(p)) - mpmath.mpf(q))), otypes=[float])(a, ro)
    M = np.broadcast_to(rabs.max(axis=0, keepdims=True), diff.shape)
    zero = M == 0.0
    if (diff[zero] != 0.0).any():
        return float("inf")
    return float((diff[~zero] / M[~zero]).max()) if (~zero).any() else 0.0


def report(section, lines):
    """Print a block of measurements; append it to the file that the environment variable USV_MODEL_EDGES_OUT names, if any (how
    profiles/model_edges.txt is produced)."""
    text = "## %s\n%s\n" % (section, "\n".join(lines))
    print(text)
    out = os.environ.get("USV_MODEL_EDGES_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(text + "\n")


# ---- the regimes
T_INT = 0.1
STEPS = (1, 4)
NPOINT = 61        # points per regime and model of the pointwise tables (f, J)
NINTEG = 35        # ... of the integrator tables (B of the batched integrator: not a multiple of 16)
V_STIFF = 1.0 / (800.0 * T_INT)    # 800 |v| T / steps <= 1 at steps = 1: the stiff sway drag (tests/test_gpu_sim.py _points)
REGIMES = ["fast", "switch", "reversing", "slow", "turning", "far_heading"]
APPLIES = {0: ["fast", "switch", "reversing", "slow", "turning"],        # (no heading state)
           1: ["reversing", "slow", "far_heading"],                      # (no 3-DOF block: no drag branch, no yaw rate)
           2: REGIMES}
_SEED = {r: 1000 + 37 * i for i, r in enumerate(REGIMES)}


def _sgn(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _draw(model, regime, integ, n, rng):
    """One draw of n points: the middle of the operating range (tests/test_gpu_sim.py _points, with the sway speed inside the
    stiffness bound and away from zero), then the regime's own coordinates on top."""
    R = lambda lo, hi: rng.uniform(lo, hi, n)
    u = R(0.3, 1.0)
    v = _sgn(rng, n) * R(1e-4, 0.9 * V_STIFF)
    r = _sgn(rng, n) * R(1e-3, 0.1)
    Tp, Ts = R(-20, 20), R(-20, 20)
    psi, ak = R(-np.pi, np.pi), R(-np.pi, np.pi)
    c = 0.78 if model == 0 else 1.0
    if regime == "fast":
        u = R(1.26, 1.6)
        Tp, Ts = R(10, 20), R(10, 20)
    elif regime == "switch":
        # within 0.02 of the switch, with a total thrust Tu = Tp + c Ts that carries u across inside the period: from below against the
        # slow branch's drag 25 u, from above with the fast branch's 70.92 u^2 - 64.55 u = 30.1 at u = 1.25 (mass 32.25)
        up = np.arange(n) % 2 == 0
        delta = R(0.002, 0.02)
        k = R(1.5, 3.0)
        u = np.where(up, KINK_U - delta, KINK_U + delta)
        Tu = np.where(up, 25.0 * KINK_U + 32.25 * delta / T_INT * k, 30.1 - 32.25 * delta / T_INT * k)
        Tp = Tu / (1.0 + c) + R(-1, 1)
        Ts = (Tu - Tp) / c
        r = _sgn(rng, n) * R(1e-3, 0.02)
    elif regime == "reversing":
        u = R(-0.5, -0.01)
    elif regime == "slow":
        sp_ = _logu(rng, 1e-3 if integ else 1e-8, 1e-2, n)
        th = R(-np.pi, np.pi)
        u = sp_ * np.cos(th) - (0.0 if model == 0 else 0.001)     # (model 0 has no u + 0.001: its speed is hypot(u, v))
        v = sp_ * np.sin(th)
        Tp, Ts = R(-0.05, 0.05), R(-0.05, 0.05)                   # (thrusts that leave the vessel slow over the period)
        r = _sgn(rng, n) * R(1e-3, 0.02)
    elif regime == "turning":
        # |r| T from 0.02 to 0.24: the series' two halves, the seam at 0.125 inside a period, and the library fallback.  A slow surge,
        # so that the sway acceleration -0.6 u r keeps |v| inside the stiffness bound over the period.
        r = _sgn(rng, n) * np.linspace(0.02, 0.24, n)[rng.permutation(n)] / T_INT
        u = R(0.05, 0.15)
        v = _sgn(rng, n) * R(1e-4, 0.3 * V_STIFF)
    elif regime == "far_heading":
        psi = _sgn(rng, n) * _logu(rng, 10.0, 1e5, n)
        ak = _sgn(rng, n) * _logu(rng, 10.0, 1e5, n)
    if model == 0:
        x = np.column_stack([u, v, r, Tp, Ts])
        U = np.column_stack([R(-5, 5), R(-5, 5)])
    elif model == 1:
        chie = ak if regime == "far_heading" else R(-1, 1)
        if regime != "slow":
            v = _sgn(rng, n) * R(1e-3, 0.2)
        x = np.column_stack([u, v, R(-2, 2), chie, R(-0.5, 0.5), R(-5, 5), R(-5, 5), psi])
        U = R(-0.5, 0.5)[:, None]
    else:
        x = np.column_stack([psi, np.sin(psi), np.cos(psi), u, v, r, R(-2, 2), R(-5, 5), R(-5, 5), ak, R(-5, 5), R(-5, 5), Tp, Ts])
        U = np.column_stack([R(-5, 5), R(-5, 5)])
    return np.ascontiguousarray(x), np.ascontiguousarray(U)


KINK_MIN = 1e-9


@functools.lru_cache(maxsize=None)
def points(model, regime):
    """The pointwise table of (model, regime): x [NPOINT][nx], u [NPOINT][nu], no point within KINK_MIN of a kink"""
    assert regime in APPLIES[model]
    rng = np.random.default_rng(_SEED[regime] + model)
    while True:
        x, U = _draw(model, regime, False, NPOINT, rng)
        if model == 1 or min(float(_kink(model, [mpmath.mpf(float(t)) for t in xi])) for xi in x) >= KINK_MIN:
            return x, U


@functools.lru_cache(maxsize=None)
def integ_points(model, regime):
    """The integrator table of (model, regime): x [NINTEG][nx], u [NINTEG][nu] and, per step count of STEPS (T = T_INT), the reference
    {steps: (x_next [NINTEG][nx] mpf, S [NINTEG][nx][nx + nu] mpf, kink [NINTEG])}.  Redrawn as a whole until no stage point of any
    point, at either step count, lies within KINK_MIN of a kink: no test drops a point."""
    assert regime in APPLIES[model]
    rng = np.random.default_rng(_SEED[regime] + 500 + model)
    while True:
        x, U = _draw(model, regime, True, NINTEG, rng)
        ref = {}
        for steps in STEPS:
            out = [rk4_sens(model, x[i], U[i], T_INT, steps) for i in range(NINTEG)]
            ref[steps] = (np.array([o[0] for o in out], dtype=object), np.array([o[1] for o in out], dtype=object),
                          np.array([o[2] for o in out]))
        if min(ref[s][2].min() for s in STEPS) >= KINK_MIN:
            return x, U, ref


@functools.lru_cache(maxsize=None)
def point_ref(model, regime):
    """(f [NPOINT][nx], J [NPOINT][nx][nu + nx]) of the pointwise table as object arrays of mpf"""
    x, U = points(model, regime)
    return (np.array([f(model, x[i], U[i]) for i in range(len(x))], dtype=object),
            np.array([jac(model, x[i], U[i]) for i in range(len(x))], dtype=object))


# d = x[0] - x_start[0] of the sweep through ModelM2::sincos_near: the series' range, the seam |d| = 0.125 exactly with its two
# neighbours in double on either side, 0, and the library fallback out to 0.3
def d_sweep():
    e = 0.125
    seam = [np.nextafter(e, 0), e, np.nextafter(e, 1)]
    d = list(np.linspace(-0.3, 0.3, 25)) + seam + [-s for s in seam] + [0.0, 1e-9, -1e-9, 1e-3, -1e-3, 0.0625, -0.0625]
    return np.array(sorted(set(d)))


@functools.lru_cache(maxsize=None)
def sweep_points():
    """(x_start [n][14], x [n][14], u [n][2]) for ModelCall<ModelM2>::prepare(x_start) / fjvp(pre, x): every d of d_sweep() at three
    base headings psi0 (0, 0.75 and -3141: the last two take +-0.125 exactly as well).  psi of x is psi0 + d rounded; d as the header
    forms it is x[0] - x_start[0]."""
    rng = np.random.default_rng(77)
    xb, Ub = _draw(2, "turning", False, 3, rng)
    xb[:, 0] = [0.0, 0.75, -3141.0]     # (psi0 = 0: d is x[0] itself, so the seam's neighbours in double are hit exactly)
    xs, xx, uu = [], [], []
    for b in range(3):
        s = xb[b].copy()
        s[1], s[2] = np.sin(s[0]), np.cos(s[0])
        # the headings of the sweep, and at every base the doubles next to psi0 +- 0.125 (their d lies just beyond / inside the seam)
        psis = [s[0] + d for d in d_sweep()]
        for e in (s[0] - 0.125, s[0] + 0.125):
            psis += [np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]
        for psi in sorted(set(psis)):
            x = s.copy()
            x[0] = psi
            xs.append(s)
            xx.append(x)
            uu.append(Ub[b])
    return np.ascontiguousarray(xs), np.ascontiguousarray(xx), np.ascontiguousarray(uu)


@functools.lru_cache(maxsize=None)
def sweep_ref():
    xs, xx, uu = sweep_points()
    return (np.array([f(2, xx[i], uu[i]) for i in range(len(xx))], dtype=object),
            np.array([jac(2, xx[i], uu[i]) for i in range(len(xx))], dtype=object))
