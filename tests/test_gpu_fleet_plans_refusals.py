"""Exchanged plans on a real MI355X (`pytest -m gpu`): what usvmpc_<kind>_fleet_plans and usvmpc_<kind>_fleet_plan_state refuse through the C
ABI, held word for word and in order to the hand-written table tests/fleet_plans_ref.py (which tests/test_world_plan_plans.py holds
csrc/world_plan.hpp to on the CPU), and that a refused call changes nothing.  N < 2 cannot be met through the C ABI - usvmpc_create refuses
such a horizon - and is held on the CPU only."""
import ctypes as C

import numpy as np
import pytest

from mpc_collisionavoidance_amd import BatchOcpSolver, usv_models
from mpc_collisionavoidance_amd.guidance import GuidanceFrontEnd, PathFollowingFrontEnd
from tests import fleet_plans_ref as R
from tests import test_gpu_guidance_fleet as gbase
from tests import test_gpu_pf_fleet as pbase

pytestmark = pytest.mark.gpu

E_ARG = -1
M = {"guidance": "usv_model_guidance_ca1", "pf": "usv_model_pf_ca"}


def _err(s):
    return s._lib.usvmpc_last_error(s._h).decode()


def _handles(kind, nB, S, n_fixed):
    """(solver of the OTHER model, solver, front end, reset(), set_world()) for `kind`"""
    if kind == "pf":
        wps, x0, fixed, fvel = pbase._scenes(S, n_fixed, 6)
        wps, x0, fixed, fvel = wps[:nB], x0[:nB], np.ascontiguousarray(fixed[:nB]), np.ascontiguousarray(fvel[:nB])
        other = BatchOcpSolver(usv_models.make_ocp(M["guidance"], 8 * 0.05, 8, 8), nB)
        ocp, s = pbase._solver(nB, 4, x0)
        fe = PathFollowingFrontEnd(s)
        return other, s, fe, lambda: fe.reset(wps), lambda: fe.set_world(fixed, vel=fvel)
    wps, x0, fixed, fvel = gbase._scenes(nB, S, n_fixed, 6)
    other = BatchOcpSolver(usv_models.make_ocp(M["pf"], 8 * 0.01, 8, 4), nB)
    ocp, s, fe = gbase._solver(nB, 8, 4, x0)
    return other, s, fe, lambda: fe.reset(wps, x0[:, 7]), lambda: fe.set_world(fixed, max_radius=gbase.R_SENSE, vel=fvel)


@pytest.mark.parametrize("kind", R.KINDS)
def test_refusals_through_the_c_abi(kind):
    nB, S, n_fixed = 12, 3, 5
    other, s, fe, reset, set_world = _handles(kind, nB, S, n_fixed)
    lib = s._lib
    plans = getattr(lib, "usvmpc_%s_fleet_plans" % kind)
    pstate = getattr(lib, "usvmpc_%s_fleet_plan_state" % kind)
    table, stable = dict(R.REFUSALS[kind]), dict(R.STATE_REFUSALS[kind])
    src = np.full((nB, 4), 7, dtype=np.int32)
    fed, launches = C.c_longlong(7), C.c_longlong(7)
    ip = C.POINTER(C.c_int)

    def state():
        return pstate(s._h, src.ctypes.data_as(ip), C.byref(fed), C.byref(launches))

    # another model
    for on in (1, 0):
        assert plans(other._h, on) == E_ARG and _err(other) == table["model"]
    assert pstate(other._h, None, None, None) == E_ARG and _err(other) == stable["model"]
    other.close()
    assert plans(None, 1) != 0
    # before the reset
    assert plans(s._h, 1) == E_ARG and _err(s) == table["reset"]
    assert state() == E_ARG and _err(s) == stable["reset"]
    reset()
    # no fleet yet: with no list, with a list
    assert plans(s._h, 1) == E_ARG and _err(s) == table["fleet"]
    set_world()
    assert plans(s._h, 1) == E_ARG and _err(s) == table["fleet"]
    assert plans(s._h, 0) == E_ARG and _err(s) == table["fleet"]
    # a handle that never switched plans on answers from the host
    assert state() == 0 and (src == -1).all() and fed.value == 0 and launches.value == 0
    assert pstate(s._h, None, None, None) == 0
    # a refused call changes nothing: the handle prepares as a handle without plans
    fe.set_fleet(S)
    fe.prepare()
    p = s.get_all("p")
    assert state() == 0 and (src == -1).all() and fed.value == 0 and launches.value == 0
    # on: the calls succeed; switched off while the fleet is off is refused, and the fleet coming back finds plans as they were
    assert plans(s._h, 1) == 0 and plans(s._h, 1) == 0 and plans(s._h, 0) == 0 and plans(s._h, 1) == 0
    fe.set_fleet(0)
    assert plans(s._h, 0) == E_ARG and _err(s) == table["fleet"]
    fe.set_fleet(S)
    st = (s.solve() == 0).all()
    s.advance(0.0, 1)
    fe.prepare()
    assert state() == 0 and launches.value == 1 and fed.value == (src >= 0).sum()
    if st:
        assert fed.value > 0
    assert (s.get_all("p")[:, 0] != 0.0).any() and s.get_all("p").shape == p.shape
    s.close()
