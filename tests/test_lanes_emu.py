"""The CPU emulator of the cross-lane interface (tests/emu/lanes.hpp) against the plain reference of tests/lanes_ref.py, through the probe
body of csrc/lanes_probe.hpp (usv_emu_lanes): every numbered result, bit for bit, on the three smallest shapes at which the row of a wave,
the wave of a workgroup and a partly filled last wave differ.  tests/test_gpu_lanes.py holds the device to the same reference and to the
emulator's output, so the emulator - on which every kernel body is developed and on which test_emu_kernels, test_wide_emu, test_cpc_emu,
test_lin_pairs_emu and the emulator half of test_condensing rest - is the device's model by test, not by reading."""
import ctypes as C

import numpy as np
import pytest

from mpc_collisionavoidance_amd import _capi
from tests import lanes_ref as LR

# (groups, threads per workgroup): four one-wave workgroups; one four-wave workgroup; a last wave with two live rows
SHAPES = [(16, 64), (16, 256), (18, 256)]
PROBE_ARGS = [C.c_int, C.c_int, C.c_int, _capi._dp, _capi._ip, _capi._dp, _capi._ip, _capi._dp, C.c_long]


def run_probe(fn, ngroups, block_threads, inputs):
    """the probe through the C entry `fn` (the emulator's or the device's): (out, iout, planes) after the run"""
    din, iin, out0, iout0, planes0 = inputs
    out, iout, planes = out0.copy(), iout0.copy(), planes0.copy()
    rc = fn(0, ngroups, block_threads, din.ctypes.data_as(_capi._dp), iin.ctypes.data_as(_capi._ip), out.ctypes.data_as(_capi._dp),
            iout.ctypes.data_as(_capi._ip), planes.ctypes.data_as(_capi._dp), len(planes))
    assert rc == 0, rc
    return out, iout, planes


def emu_probe(emu):
    emu.usv_emu_lanes.argtypes = PROBE_ARGS
    return emu.usv_emu_lanes


_cache = {}


def case(ngroups, block_threads):
    """operands and reference of one shape, computed once and shared (read-only)"""
    key = (ngroups, block_threads)
    if key not in _cache:
        inputs = LR.make_inputs(ngroups, block_threads)
        ref = LR.reference(ngroups, block_threads, *inputs)
        for a in inputs + ref:
            a.setflags(write=False)
        _cache[key] = (inputs, ref)
    return _cache[key]


def check_against(ngroups, got, want, skip=()):
    """every result, the plane window and the canaries around it"""
    (out, iout, planes), (rout, riout, rplanes) = got, want
    bad = LR.disagreements(out, rout, LR.OUT_NAMES, skip)
    bad.update(LR.disagreements(LR.normalise(iout, ngroups), LR.normalise(riout, ngroups), LR.IOUT_NAMES))
    assert not bad, "results that differ (name: entries): %r" % bad
    w = slice(LR.PL_PAD, LR.PL_PAD + ngroups * LR.NPL * 16)
    assert LR.same_bits(planes[w], rplanes[w]).all(), "Planes.st: the window differs at %r" % np.flatnonzero(~LR.same_bits(planes[w], rplanes[w]))[:8]
    outside = np.ones(len(planes), dtype=bool)
    outside[w] = False
    assert (planes[outside] == LR.CANARY).all(), "a store outside the plane window (parked or out of range) changed the caller's memory"


def test_numbering_matches_the_compiled_probe(emu):
    d = (C.c_int * 6)()
    emu.usv_emu_lanes_dims.argtypes = [C.POINTER(C.c_int)]
    emu.usv_emu_lanes_dims(d)
    assert list(d) == [LR.NIN, LR.NIIN, LR.NOUT, LR.NIOUT, LR.NPL, LR.PL_PAD]
    assert len(LR.OUT_NAMES) == LR.NOUT and len(LR.IOUT_NAMES) == LR.NIOUT


def test_operands_can_tell_a_wrong_implementation():
    """The reference's own operands: a value from the wrong group, lane or slot is a different number; fused and unfused rounding differ;
    the order of a chain changes the last bit; the specials hold a signalling NaN that survived numpy."""
    (din, iin, out0, iout0, planes0), (rout, _, _) = case(16, 64)
    routed = din[:, [LR.S_A, LR.S_B, LR.S_C, LR.S_D, LR.S_E]]
    assert len(np.unique(routed)) == routed.size
    A, B, Cc, D, E = (din[:, s] for s in (LR.S_A, LR.S_B, LR.S_C, LR.S_D, LR.S_E))
    unfused = B[:, 5:6] * A + din[:, LR.S_FC]
    fused = rout[:, LR.O["fma_bc.cancel"]]
    assert (unfused == 0.0).all() and (fused != 0.0).sum() > 200         # the rounding error of the product, lost without the fusion
    for k in range(16):
        assert (rout[:, LR.O["fma_bc"] + k] != B[:, k:k + 1] * A + Cc).sum() > 16
    swapped = LR.fma_chain(Cc, [(4, B, A), (14, E, B), (11, D, E), (6, A, D)])
    assert (swapped != rout[:, LR.O["fma_bc4"]]).sum() > 16
    lane_order = np.zeros(16)
    red0 = din[:, LR.S_RED]
    for l in range(16):
        lane_order = lane_order + red0[:, l]
    assert (lane_order[:, None] != rout[:, LR.O["gsum"]]).any(axis=1).sum() > 4
    assert LR.is_snan(din[:, LR.S_VA]).any() and LR.is_snan(din[:, LR.S_VB]).any()
    pairs = {(a.tobytes(), b.tobytes()) for a, b in zip(din[:, LR.S_VA].reshape(-1), din[:, LR.S_VB].reshape(-1))}
    assert len(pairs) == len(LR.SPECIALS) ** 2


@pytest.mark.parametrize("ngroups,block_threads", SHAPES)
def test_emulator_equals_reference(emu, ngroups, block_threads):
    inputs, ref = case(ngroups, block_threads)
    got = run_probe(emu_probe(emu), ngroups, block_threads, inputs)
    check_against(ngroups, got, ref)


def test_recorded_rules_hold_on_the_emulator(emu):
    """max / min of -0 and +0 and of a signalling NaN, as the MI355X returned them (lanes_ref.RULES, profiles/lanes_conformance.txt):
    the emulator models the device there, it is not left to std::fmax."""
    inputs, _ = case(16, 64)
    out, _, _ = run_probe(emu_probe(emu), 16, 64, inputs)
    va, vb = inputs[0][:, LR.S_VA], inputs[0][:, LR.S_VB]
    r = out[:, LR.O["vmax"]]
    zz = (va == 0) & (vb == 0) & (np.signbit(va) != np.signbit(vb))
    assert zz.sum() >= 2 and (np.signbit(r[zz]) == (LR.RULES["max_zero_sign"] < 0)).all()
    sn = LR.is_snan(va) | LR.is_snan(vb)
    assert np.isnan(r[sn]).all() == LR.RULES["snan_gives_nan"]
    qn = (np.isnan(va) ^ np.isnan(vb)) & ~sn                              # a quiet NaN on one side: the other operand
    assert LR.same_bits(r[qn], np.where(np.isnan(va), vb, va)[qn]).all()
    mixed = inputs[0][2:, LR.S_RED + 5]                                   # groups 2 ..: zeros of both signs
    assert (np.signbit(out[2:, LR.O["gmax"] + 5]) == (LR.RULES["max_zero_sign"] < 0)).all()
    assert (np.signbit(out[2:, LR.O["gmin"] + 5]) == (LR.RULES["min_zero_sign"] < 0)).all()
    assert (np.signbit(mixed).any(axis=1) & ~np.signbit(mixed).all(axis=1)).all()
