"""The front ends' resident world list on a real MI355X (`pytest -m gpu`): one scripted pass through the set-up calls of the C ABI -
usvmpc_guidance_world / _world_vel / _world_step / _world_read / _fleet / _fleet_state and the usvmpc_pf_* calls of the same names - held
to the statement csrc/world_plan.hpp is held to on the CPU (tests/world_calls_ref.py: SCRIPT, the refusals' words, the layout in numpy).
No prepare and no solve; after every call the return code, the message and what world_read returns - shapes and bits - must be as written
there."""
import ctypes as C

import numpy as np
import pytest

from mpc_collisionavoidance_amd import BatchOcpSolver, usv_models
from tests import world_calls_ref as R

pytestmark = pytest.mark.gpu

B, N, K = R.B, 5, 2
MODEL = {"guidance": "usv_model_guidance_ca1", "pf": "usv_model_pf_ca"}
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def dp(a):
    return a.ctypes.data_as(DP)


@pytest.mark.parametrize("kind", R.KINDS)
def test_scripted_pass_through_the_c_abi(kind):
    s = BatchOcpSolver(usv_models.make_ocp(MODEL[kind], N * 0.05, N, K), B)
    lib, h = s._lib, s._h
    fn = lambda name: getattr(lib, "usvmpc_%s%s" % (R.PREFIX[kind], name))
    wps = np.tile(np.array([[0.0, 0.0], [5.0, 0.0], [5.0, 5.0]]).ravel(), (B, 1))
    if kind == "guidance":     # (every call needs the reset first; the path-following world calls work before it: the first one does)
        assert lib.usvmpc_guidance_reset(h, dp(wps), 3, dp(np.zeros(B))) == 0
    model = R.WorldModel()
    nworld, nfixed, fleet = 0, 0, 0
    for i, step in enumerate(R.SCRIPT):
        what = "step %d: %s" % (i, step)
        call = step["call"]
        data = None
        if call == "world":
            data = R.call_data(i, (B, step["n"], 3))
            rc = fn("world")(h, dp(data) if data.size else None, step["n"], C.c_double(step["radius"]))
        elif call == "vel":
            data = R.call_data(i, (B, nfixed if fleet else nworld, 2))
            arg = None if not step["given"] else dp(data if data.size else np.zeros(1))
            rc = fn("world_vel")(h, arg, step["predict"]) if kind == "guidance" else fn("world_vel")(h, arg)
        elif call == "fleet":
            rc = fn("fleet")(h, step["S"], C.c_double(step["radius"]))
        elif call == "step":
            rc = fn("world_step")(h, C.c_double(step["T"]))
        else:
            ms, st = np.zeros(B), np.zeros(B, dtype=np.int32)
            rc = fn("fleet_state")(h, dp(ms), st.ctypes.data_as(IP))
            assert rc == 0 and (ms == 1e300).all() and (st == -1).all(), what      # (no prepare has run: none met yet)
        if "err" in step:
            key, numbers = step["err"]
            assert rc == -1 and lib.usvmpc_last_error(h).decode() == R.refusal(kind, call, key, **numbers), what
        else:
            assert rc == 0, (what, lib.usvmpc_last_error(h).decode())
            model.apply(step, kind, data)
            nworld, nfixed, fleet = (step["state"][k] for k in ("nworld", "nfixed", "fleet_S"))
        # what the device holds, refused or not
        want_w, want_v = model.read()
        assert want_w.shape == (B, nworld, 3), what
        w, v = np.full((B, nworld, 3), -7.0), np.full((B, nworld, 2), -7.0)
        assert fn("world_read")(h, dp(w) if w.size else None, dp(v) if v.size else None) == 0, what
        assert w.tobytes() == want_w.tobytes() and v.tobytes() == want_v.tobytes(), what
        if i == 0 and kind == "pf":
            assert lib.usvmpc_pf_reset(h, dp(wps), 3) == 0
    s.close()
