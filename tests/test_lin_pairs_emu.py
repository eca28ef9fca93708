"""The paired lineariser (csrc/linearize.hpp run_pair*: two (instance, stage) pairs per 16-lane row, for models that declare the at most 8
columns to integrate) against the 16-lane form, on the lane emulator: every plane of every (group, stage) equal to the bit, in each of
the orders the library launches.  The driver (tests/lin_pairs_emu.cpp) is compiled here and linked to the emulator library for its fibers.
CPU only.  The orders themselves (csrc/lin_order.hpp) are checked by tests/lin_pairs_order_harness.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mpc_collisionavoidance_amd import _capi
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")

ORDERS = {"whole-batch": 0, "speculative": 1, "fix-up": 2, "retire-order": 3, "fix-up-by-groups": 4}


def _d(a):
    return a.ctypes.data_as(_capi._dp)


def _i(a):
    return a.ctypes.data_as(_capi._ip)


@pytest.fixture(scope="module")
def pairs(emu, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lin_pairs") / "liblin_pairs_emu.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + EMU, "-I" + CSRC, "-o", so, os.path.join(ROOT, "tests", "lin_pairs_emu.cpp"),
                           "-L" + EMU, "-lusv_emu", "-Wl,-rpath," + EMU])
    lib = C.CDLL(so)
    lib.usv_emu_lin_pairs.argtypes = [C.POINTER(_capi.Desc), C.c_int] + [_capi._dp] * 4 + [_capi._ip] * 4 + [_capi._dp] * 2 + [_capi._ip] * 2
    return lib


@pytest.fixture(scope="module")
def order_harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lin_pairs_order") / "lin_pairs_order_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "lin_pairs_order_harness.cpp")])
    return exe


@pytest.mark.parametrize("B,Bp", [(1, 4), (5, 8), (13, 16), (13, 24)])
@pytest.mark.parametrize("N", [2, 4, 5])
@pytest.mark.parametrize("maps", [0, 3], ids=["identity", "both-permuted"])
def test_paired_orders_cover_the_grid_once(order_harness, B, Bp, N, maps):
    assert Bp > B
    r = subprocess.run([order_harness, str(B), str(Bp), str(N), str(29 + B + maps), str(maps)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[0] == "ok"


# (model, obstacle rows, RK4 steps per interval): usv_model_pf_ca with 1 and 5 steps (the bench's count); usv_model, which has no
# quadrature entry, with one and several (usv_model_guidance_ca1 declares no columns: it stays on the 16-lane form)
MODELS = [("usv_model_pf_ca", 3, 1), ("usv_model_pf_ca", 3, 5), ("usv_model", 0, 1), ("usv_model", 0, 3)]


@pytest.mark.parametrize("name,K,steps", MODELS)
@pytest.mark.parametrize("N", [4, 5])   # five stages: the last row of an instance in the retire order has a lone half; six: none
@pytest.mark.parametrize("B", [5, 13])  # Bp = 8, 16: padded groups replay the last map entry
def test_paired_lineariser_equals_the_16_lane_form(pairs, name, K, steps, N, B):
    ocp, wl = util.make(name, N, K, B, seed=17 + N + B)
    ocp.solver_options.sim_method_num_steps = steps
    desc = _capi.desc_from_ocp(ocp, batch=B)
    Bp = (B + 3) // 4 * 4
    assert Bp > B
    words = (N + 32) // 32
    rng = np.random.default_rng(100 * N + B)
    model = _capi.MODEL_IDS[name]
    for order_name, order in ORDERS.items():
        pn, pc = rng.permutation(B).astype(np.int32), rng.permutation(B).astype(np.int32)
        assert np.any(pn != np.arange(B)) and np.any(pc != np.arange(B))
        inv = np.empty(B, np.int32)
        inv[pn] = np.arange(B, dtype=np.int32)
        ready = (rng.uniform(size=B) < 0.6).astype(np.int32) if order in (1, 3) else np.ones(B, np.int32)
        mask = np.zeros((B, words), np.int32)
        if order in (2, 4):  # a random pattern of marked (instance, stage) pairs, some instances without any
            bits = rng.uniform(size=(B, N + 1)) < 0.4
            bits[rng.integers(B)] = False
            for k in range(N + 1):
                mask[:, k // 32] |= bits[:, k].astype(np.int32) << (k % 32)
            assert mask.any()
        fill = 7.25  # (what neither form writes stays as it was, in both)
        wsa, wsb = np.full((N + 1, Bp, 64, 16), fill), np.full((N + 1, Bp, 64, 16), fill)
        ra, rb = mask.copy(), mask.copy()
        npt = pairs.usv_emu_lin_pairs(C.byref(desc), order, _d(wl["x_init"]), _d(wl["u_init"]), _d(wl["yref"]), _d(wl["yref_e"]), _i(ready),
                                      _i(pn), _i(inv), _i(pc), _d(wsa), _d(wsb), _i(ra), _i(rb))
        assert npt > 0, (order_name, npt)
        a = wsa.reshape(-1)[: (N + 1) * Bp * npt * 16].reshape(N + 1, Bp, npt, 16)
        b = wsb.reshape(-1)[: (N + 1) * Bp * npt * 16].reshape(N + 1, Bp, npt, 16)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), (order_name, np.argwhere(a.view(np.int64) != b.view(np.int64))[:4])
        assert np.array_equal(ra, rb), order_name
        assert np.any(a != fill), order_name
        if order == 0:
            pmat = pairs.usv_emu_lin_pairs_pmat(model)  # (P_RB0, P_GQ, P_MAT..: the last planes of a stage's window)
            assert not np.any(a[:N, :, pmat - 2:, :] == fill) and not np.any(a[N, :, pmat - 1, :] == fill)  # all of them written
        if order in (1, 3):
            assert ra.any() and np.any(a == fill)  # some stages were left to the fix-up
        if name == "usv_model_pf_ca" and order in (0, 3):
            # the quadrature entry (row ye, column ak) is really exercised: non-zero at every stage of the whole-batch pass
            pos = pairs.usv_emu_lin_pairs_entry(model, 6, 2 + 9)
            assert pos >= 0
            q = a[:N, :, pairs.usv_emu_lin_pairs_pmat(model) + pos // 16, pos % 16]
            assert np.any((q != 0.0) & (q != fill))
            if order == 0:
                assert np.all(q != 0.0)
