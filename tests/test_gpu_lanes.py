"""The device's cross-lane interface (csrc/gfx950/lanes.hpp) against the plain reference of tests/lanes_ref.py AND against the CPU emulator
(tests/emu/lanes.hpp) in the same process, on a real MI355X (`pytest -m gpu`): the probe body of csrc/lanes_probe.hpp through
usvmpc_debug_lanes and usv_emu_lanes, every numbered result bit for bit.  The exceptions are the reciprocal slots (frcp, frsqrt, frcp2):
hardware estimate + Newton steps on the device, IEEE division on the emulator - frcp2 is measured in ulp here, frcp and frsqrt in
tests/test_gpu_model_edges.py.  profiles/lanes_conformance.txt is this file's output under USV_MODEL_EDGES_OUT."""
import mpmath
import numpy as np
import pytest

from mpc_collisionavoidance_amd import _capi
from tests import lanes_ref as LR
from tests import model_ref as R
from tests.test_gpu_model_edges import _operands
from tests.test_lanes_emu import SHAPES, case, check_against, emu_probe, run_probe

pytestmark = pytest.mark.gpu

# lanes::frcp2 on the device may exceed the emulator's maximum error (IEEE division, the same two multiplications) by this many ulp: frcp
# is within 1 ulp of 1 / x (tests/test_gpu_model_edges.py), and that relative error carried through one multiplication is at most 2 ulp of
# the product
FRCP2_EXTRA_ULP = 2.0


@pytest.mark.parametrize("ngroups,block_threads", SHAPES)
def test_device_equals_reference_and_emulator(emu, ngroups, block_threads):
    inputs, ref = case(ngroups, block_threads)
    dev = run_probe(_capi.lib().usvmpc_debug_lanes, ngroups, block_threads, inputs)
    check_against(ngroups, dev, ref, skip=LR.FAST)
    em = run_probe(emu_probe(emu), ngroups, block_threads, inputs)
    check_against(ngroups, dev, em, skip=LR.FAST)


def test_recorded_rules_and_agreement_per_primitive(emu):
    """What the device returns where IEEE 754 and the header leave it open, asserted against lanes_ref.RULES and written down: the sign
    of max / min of -0 and +0 in either order, a signalling and a quiet NaN on either side, through the one-instruction maxima and the
    butterflies.  And one line per primitive: on how many results device, emulator and reference agree (all of them)."""
    dev_fn, emu_fn = _capi.lib().usvmpc_debug_lanes, emu_probe(emu)
    inputs, _ = case(16, 64)
    out, _, _ = run_probe(dev_fn, 16, 64, inputs)
    va, vb = inputs[0][:, LR.S_VA].reshape(-1), inputs[0][:, LR.S_VB].reshape(-1)
    name = {LR.QNAN.tobytes(): "qNaN", LR.NEG_QNAN.tobytes(): "-qNaN", LR.SNAN.tobytes(): "sNaN"}
    show = lambda x: name.get(np.float64(x).tobytes(), "NaN" if np.isnan(x) else repr(float(x)))
    lines = ["%-7s %-7s  vmax %-7s vmax_abs %-7s vmax_abs2 %s" % (show(a), show(b), show(r0), show(r1), show(r2))
             for a, b, r0, r1, r2 in zip(va[:121], vb[:121], out[:, LR.O["vmax"]].reshape(-1), out[:, LR.O["vmax_abs"]].reshape(-1),
                                         out[:, LR.O["vmax_abs2"]].reshape(-1))
             if np.isnan(a) or np.isnan(b) or (a == 0 and b == 0)]
    z = inputs[0][:, LR.S_RED + 5]
    lines += ["zeros, lanes 0 .. 15 %s  gmax %-5r gmin %-5r gsum %r" % ("".join("-" if s else "+" for s in np.signbit(z[g])), float(out[g, LR.O["gmax"] + 5, 0]),
                                                                      float(out[g, LR.O["gmin"] + 5, 0]), float(out[g, LR.O["gsum"] + 5, 0])) for g in range(6)]
    r = out[:, LR.O["vmax"]].reshape(-1)
    zz = (va == 0) & (vb == 0) & (np.signbit(va) != np.signbit(vb))
    sn = LR.is_snan(va) | LR.is_snan(vb)
    lines += ["recorded rules: max(+0, -0) and max(-0, +0) -> %s; min -> %s; a signalling NaN operand -> %s"
              % ("/".join(sorted({show(x) for x in r[zz]})), "/".join(sorted({show(x) for x in out[2:, LR.O["gmin"] + 5].reshape(-1)})),
                 "/".join(sorted({show(x) for x in r[sn & ~(np.isnan(va) & np.isnan(vb))]})))]
    tallies = {}
    for ngroups, block_threads in SHAPES:
        ins, (rout, riout, _) = case(ngroups, block_threads)
        dout, diout, _ = run_probe(dev_fn, ngroups, block_threads, ins)
        eout, eiout, _ = run_probe(emu_fn, ngroups, block_threads, ins)
        for tag, got, got_i in (("device", dout, diout), ("emulator", eout, eiout)):
            t = tallies.setdefault(tag, {})
            LR.tally(t, got, rout, LR.OUT_NAMES, skip=LR.FAST)
            LR.tally(t, LR.normalise(got_i, ngroups), LR.normalise(riout, ngroups), LR.IOUT_NAMES)
        t = tallies.setdefault("device = emulator", {})
        LR.tally(t, dout, eout, LR.OUT_NAMES, skip=LR.FAST)
        LR.tally(t, LR.normalise(diout, ngroups), LR.normalise(eiout, ngroups), LR.IOUT_NAMES)
    prims = list(tallies["device"])
    lines += ["%-18s device = reference %5d / %-5d emulator = reference %5d / %-5d device = emulator %5d / %d"
              % ((p,) + tuple(tallies["device"][p]) + tuple(tallies["emulator"][p]) + tuple(tallies["device = emulator"][p])) for p in prims]
    R.report("recorded rules, and agreement per primitive, over the shapes %r" % (SHAPES,), lines)
    assert (np.signbit(r[zz]) == (LR.RULES["max_zero_sign"] < 0)).all()
    assert np.isnan(r[sn]).all() == LR.RULES["snan_gives_nan"]
    assert (np.signbit(out[2:, LR.O["gmax"] + 5]) == (LR.RULES["max_zero_sign"] < 0)).all()
    assert (np.signbit(out[2:, LR.O["gmin"] + 5]) == (LR.RULES["min_zero_sign"] < 0)).all()
    assert all(a == b for t in tallies.values() for a, b in t.values()), lines


def frcp2_pairs():
    """pairs log-uniform with the product inside 1e-300 .. 1e300 (the header's domain), the binade-edge operands of the frcp test paired
    with each other, and its remaining operands (the ladder over two binades, exact squares) paired in reverse order"""
    rng = np.random.default_rng(8192)
    la, lp = rng.uniform(-300, 300, 3 * 4096), rng.uniform(-300, 300, 3 * 4096)
    ok = np.abs(lp - la) <= 300
    a, b = (10.0 ** la[ok])[:4096], (10.0 ** (lp - la)[ok])[:4096]
    assert len(a) == 4096
    fixed = _operands()[4096:]
    edges, rest = fixed[:9], fixed[9:]
    ea, eb = np.meshgrid(edges, edges, indexing="ij")
    return np.concatenate([a, ea.reshape(-1), rest]), np.concatenate([b, eb.reshape(-1), rest[::-1]])


def _frcp2(fn, a, b):
    """frcp2 of the pairs through the probe's slots: (1 / a, 1 / b)"""
    n = len(a)
    G = -(-n // 16)
    din, iin, out0, iout0, planes0 = LR.make_inputs(G, 256, seed=1)
    fa, fb = np.ones(G * 16), np.ones(G * 16)
    fa[:n], fb[:n] = a, b
    din[:, LR.S_FA], din[:, LR.S_FB] = fa.reshape(G, 16), fb.reshape(G, 16)
    out, _, _ = run_probe(fn, G, 256, (din, iin, out0, iout0, planes0))
    return out[:, LR.O["frcp2.a"]].reshape(-1)[:n], out[:, LR.O["frcp2.b"]].reshape(-1)[:n]


def _ulp(got, ref):
    return np.array([float(abs(mpmath.mpf(float(p)) - q)) / np.spacing(abs(float(q))) for p, q in zip(got, ref)])


def test_frcp2_in_ulp_against_the_emulators_division(emu):
    """lanes::frcp2 (ONE reciprocal of the product, two multiplications - what the IPM calls for its slacks and multipliers) against mpmath,
    beside the emulator's frcp2 on the same pairs as the yardstick."""
    a, b = frcp2_pairs()
    special = [(0.0, 2.0), (2.0, 0.0), (np.inf, 2.0), (1e-200, 1e-200), (1e200, 1e200), (1e-160, 1e-160), (5e-324, 1.0), (-3.0, 2.0)]
    sa, sb = np.array([p[0] for p in special]), np.array([p[1] for p in special])
    n = len(a)
    dev = _frcp2(_capi.lib().usvmpc_debug_lanes, np.concatenate([a, sa]), np.concatenate([b, sb]))
    em = _frcp2(emu_probe(emu), np.concatenate([a, sa]), np.concatenate([b, sb]))
    with mpmath.workdps(R.DPS):
        ra, rb = [1 / mpmath.mpf(float(v)) for v in a], [1 / mpmath.mpf(float(v)) for v in b]
        e_dev = np.maximum(_ulp(dev[0][:n], ra), _ulp(dev[1][:n], rb))
        e_emu = np.maximum(_ulp(em[0][:n], ra), _ulp(em[1][:n], rb))
    lines = ["frcp2 device   max %.3f ulp at (a, b) = (%r, %r)   (%d pairs)" % (e_dev.max(), float(a[e_dev.argmax()]), float(b[e_dev.argmax()]), n),
             "frcp2 emulator max %.3f ulp at (a, b) = (%r, %r)" % (e_emu.max(), float(a[e_emu.argmax()]), float(b[e_emu.argmax()])),
             "binade edges paired with each other: device max %.3f ulp, emulator max %.3f ulp" % (e_dev[4096:4177].max(), e_emu[4096:4177].max())]
    lines += ["(a, b) = (%r, %r): device (%r, %r)  emulator (%r, %r)" % (float(x), float(y), float(p), float(q), float(s), float(t))
              for x, y, p, q, s, t in zip(sa, sb, dev[0][n:], dev[1][n:], em[0][n:], em[1][n:])]
    R.report("lanes::frcp2 on the MI355X and on the emulator against mpmath", lines)
    assert np.isfinite(dev[0][:n]).all() and np.isfinite(dev[1][:n]).all()
    # measured on the MI355X (profiles/lanes_conformance.txt): device 1.783 ulp, emulator 1.783 ulp, at the same pair
    assert e_dev.max() <= e_emu.max() + FRCP2_EXTRA_ULP, (e_dev.max(), e_emu.max())
