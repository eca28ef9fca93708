"""Exchanged plans of the path-following front end on a real MI355X (`pytest -m gpu`): the kernel usv_pf_fleet_plans, the C ABI
usvmpc_pf_fleet_plans / _fleet_plan_state and guidance.PathFollowingFrontEnd.set_fleet(plans=True) / fleet_plan_state, at the shapes of
tests/test_gpu_pf_fleet.py (B = 72, N = 6, T = 10: scene 21 straddles the 64-instance group at S = 3).

1. a handle with plans on == its twin with plans off whose host builds p with scenario.fleet_plan_stages every tick, bit for bit;
2. fallbacks: no mate chosen; a mate whose mission ends; prepare twice; advance twice;
3. a scene alone == the scene inside the batch; plans switched off again == never on; a handle that never switches them on;
4. the encounter sweep with plans on against the CPU oracle's own run (profiles/pf_encounter_plans_oracle.txt).
"""
import importlib.util
import os

import numpy as np
import pytest

from mpc_collisionavoidance_amd import scenario
from mpc_collisionavoidance_amd.guidance import PathFollowingFrontEnd
from tests import test_gpu_pf_fleet as base
from tests.fleet_plans_twin import Twin

pytestmark = pytest.mark.gpu

B, N, T = base.B, base.N, base.T
POS = scenario.FLEET_PLAN_POS["usv_model_pf_ca"]


def _pair(S, n_fixed, K, sim, scenes, radius=0.5, nB=B, mask=True):
    """(handle A: plans on, handle B: plans off), each (solver, front end, plant or None)"""
    wps, x0, fixed, fvel = scenes
    hs = []
    for plans in (True, False):
        ocp, s = base._solver(nB, K, x0)
        if mask:
            s.set_option("disturbance_mask", (1 << 3) | (1 << 5))
        fe = PathFollowingFrontEnd(s)
        fe.reset(wps)
        fe.set_world(fixed, vel=fvel if n_fixed else None)
        fe.set_fleet(S, radius, plans=plans)
        hs.append((s, fe, base._plant(ocp, nB) if sim else None))
    return hs


def _twin(hs, S, n_fixed):
    (sa, fa, pa), (sb, fb, pb) = hs
    return Twin((sa, fa), (sb, fb), dict(S=S, n_fixed=n_fixed, pos=POS, tol=0.0, finish=lambda fe: fe.state()["finish_tick"], streams_before=False))


def _tick(tw, hs, t, noise=True):
    for s, fe, plant in hs:
        base._tick(s, fe, plant, t, noise)
    tw.solved(), tw.handed_over()


def _close(hs):
    for s, fe, plant in hs:
        s.close()
        if plant is not None:
            plant.close()


# ---- 1. the definition
@pytest.mark.parametrize("S,n_fixed,K,sim", [(2, 0, 4, True), (2, 5, 4, False), (3, 0, 4, False), (3, 5, 4, True), (4, 0, 4, True),
                                             (4, 5, 4, False), (3, 30, 20, True)])   # (K = 20: two obstacle chunks)
def test_plans_handle_equals_its_host_fed_twin_bit_for_bit(S, n_fixed, K, sim):
    radius = 0.5 if S != 4 else 0.4
    hs = _pair(S, n_fixed, K, sim, base._scenes(S, n_fixed, 10 * S + n_fixed), radius)
    (sa, fa, pa), (sb, fb, pb) = hs
    tw = _twin(hs, S, n_fixed)
    for t in range(T):
        what = "S %d n_fixed %d K %d tick %d" % (S, n_fixed, K, t)
        p_cv, src = tw.prepare(what)
        if t == 0:
            assert src is None                                   # nothing solved yet: source is all -1 (held inside prepare)
        else:
            fed = (src >= 0).sum(axis=1)
            print("%s: plan-fed slots per instance %d .. %d, failed solves %d" % (what, fed.min(), fed.max(), (sb.get_int("status") != 0).sum()))
            assert (fed >= 1).all(), what + ": an instance without a plan-fed slot"
            assert (sa.get_all("p") != p_cv).any(), what + ": the plans changed nothing"
            assert np.array_equal(sa.get_all("p")[:, 0], p_cv[:, 0]), what + " stage 0"
        _tick(tw, hs, t)
        base._same(sa, fa, sb, fb, what + " after the solve", solved=True)
    never = fb.fleet_plan_state()                                # a handle that never switches plans on
    assert (never["source"] == -1).all() and never["plan_fed"] == 0 and never["plan_launches"] == 0
    assert fa.fleet_plan_state()["plan_launches"] == T - 1
    _close(hs)


# ---- 2. fallbacks
def test_no_mate_among_the_chosen_falls_back():
    """K = 1 and five fixed entries nearer than any scene-mate: the one slot holds a fixed entry, no plan is used, source is -1"""
    S, n_fixed, K = 3, 5, 1
    wps, x0, fixed, fvel = base._scenes(S, n_fixed, 21)
    ang = np.linspace(0.3, 2.8, n_fixed)
    fixed[:, :, 0] = x0[:, None, 10] + 1.0 * np.cos(ang)[None, :] * np.linspace(1.0, 1.3, n_fixed)[None, :]    # 1.0 .. 1.3 m away; mates 1.6 m and more
    fixed[:, :, 1] = x0[:, None, 11] + 1.0 * np.sin(ang)[None, :] * np.linspace(1.0, 1.3, n_fixed)[None, :]
    fixed[:, :, 2] = 0.05
    fvel[:] = 0.0
    hs = _pair(S, n_fixed, K, False, (wps, x0, fixed, fvel), mask=False)
    (sa, fa, pa), (sb, fb, pb) = hs
    for t in range(3):
        fa.prepare(), fb.prepare()
        assert sa.get_all("p").tobytes() == sb.get_all("p").tobytes(), t         # a handle without plans: today's bits
        st = fa.fleet_plan_state()
        assert (st["source"] == -1).all() and st["plan_fed"] == 0 and st["plan_launches"] == t   # (launched from tick 1 on: it found nothing to feed)
        for s, fe, plant in hs:
            base._tick(s, fe, plant, t, False)
        assert sa.get_all("x").tobytes() == sb.get_all("x").tobytes(), t
    _close(hs)


def test_a_mate_whose_mission_ends_falls_back_from_that_prepare_on():
    S, n_fixed, K = 3, 0, 4
    wps, x0, fixed, fvel = base._scenes(S, n_fixed, 4)
    done = np.arange(B) % S == 1
    wps[done, 1, 1], wps[done, 2, 0], wps[done, 2, 1] = -4.6, wps[done, 0, 0], -4.4     # both waypoints within 1 m: over from tick 2
    hs = _pair(S, n_fixed, K, True, (wps, x0, fixed, fvel))
    (sa, fa, pa), (sb, fb, pb) = hs
    tw = _twin(hs, S, n_fixed)
    for t in range(5):
        p_cv, src = tw.prepare("tick %d" % t)
        over = fa.state()["finish_tick"] >= 0
        assert np.array_equal(over, done & (t >= 2)), t
        if t >= 1:
            follows_done = np.isin(src, np.nonzero(done)[0])
            assert follows_done.any() == (t < 2), t                               # tick 1: the mate's plan is used; from tick 2 on: never
            assert (src[over] == -1).all(), t                                     # the finished instance itself does not stream
            assert ((src >= 0).sum(axis=1)[~done] >= 1).all(), t                  # the others still follow each other
        _tick(tw, hs, t)
        base._same(sa, fa, sb, fb, "tick %d after the solve" % t, solved=True)
    _close(hs)


@pytest.mark.parametrize("twice", ["prepare", "advance"])
def test_prepare_twice_and_advance_twice_give_todays_bits(twice):
    """prepare twice with no hand-over / advance twice with no solve: the second prepare / the next prepare is the constant-velocity
    prepare - B's host writes nothing - and plan_launches stays"""
    S, n_fixed, K = 3, 5, 4
    hs = _pair(S, n_fixed, K, False, base._scenes(S, n_fixed, 22))
    (sa, fa, pa), (sb, fb, pb) = hs
    tw = _twin(hs, S, n_fixed)
    for t in range(5):
        p_cv, src = tw.prepare("tick %d" % t)
        assert (src is None) == (t == 0 or (twice == "advance" and t == 3)), t
        if twice == "prepare" and t == 2:
            before = fa.fleet_plan_state()["plan_launches"]
            p_cv, src = tw.prepare("tick %d, second prepare" % t)
            assert src is None and fa.fleet_plan_state()["plan_launches"] == before
            assert sa.get_all("p").tobytes() == p_cv.tobytes()                    # today's bits: what the handle without plans wrote
        _tick(tw, hs, t)
        if twice == "advance" and t == 2:
            for s, fe, plant in hs:
                s.advance(1e-3, 500)
            tw.handed_over()
        base._same(sa, fa, sb, fb, "tick %d after the solve" % t, solved=True)
    assert fa.fleet_plan_state()["plan_launches"] == (4 if twice == "prepare" else 3)
    _close(hs)


# ---- 3. independence and switching
def test_a_scene_alone_equals_the_scene_inside_the_batch():
    S, n_fixed, K = 3, 5, 4
    wps, x0, fixed, fvel = base._scenes(S, n_fixed, 2)
    rows = {}
    for lo, hi in ((0, B), (63, 66), (0, 3)):
        nB = hi - lo
        ocp, s = base._solver(nB, K, x0[lo:hi])
        fe = PathFollowingFrontEnd(s)
        fe.reset(wps[lo:hi])
        fe.set_world(fixed[lo:hi], vel=fvel[lo:hi])
        fe.set_fleet(S, plans=True)
        plant = base._plant(ocp, nB)
        rec = []
        for t in range(T):
            fe.prepare()
            rec.append([s.get("x0", 0), s.get_all("p"), s.get_all("lh"), fe.fleet_plan_state()["source"]])
            base._tick(s, fe, plant, t, False)
            rec[-1] += [s.get_all("u"), s.get_all("x")]
        rows[(lo, hi)] = rec
        s.close(), plant.close()
    assert any((r[3] >= 0).any() for r in rows[(63, 66)])
    for lo, hi in ((63, 66), (0, 3)):
        for t in range(T):
            for k, (full, alone) in enumerate(zip(rows[(0, B)][t], rows[(lo, hi)][t])):
                if k == 3:                                                         # source: vessel numbers count from the batch's first
                    assert np.array_equal(np.where(full[lo:hi] >= 0, full[lo:hi] - lo, -1), alone), (lo, t)
                else:
                    assert np.array_equal(full[lo:hi], alone), (lo, t, k)


def test_plans_switched_off_again_equal_a_handle_that_never_had_them():
    S, n_fixed, K = 3, 5, 4
    hs = _pair(S, n_fixed, K, True, base._scenes(S, n_fixed, 23))
    (sa, fa, pa), (sb, fb, pb) = hs
    tw = _twin(hs, S, n_fixed)
    for t in range(3):
        tw.prepare("tick %d" % t)
        _tick(tw, hs, t)
    launches = fa.fleet_plan_state()["plan_launches"]
    assert launches == 2
    fa.set_fleet(S, plans=False)                                                    # B never had them: from here on its host writes nothing
    for t in range(3, 7):
        p_cv, src = tw.prepare("tick %d, plans off" % t, plans_on=False)
        assert src is None and sa.get_all("p").tobytes() == p_cv.tobytes()
        _tick(tw, hs, t)
        base._same(sa, fa, sb, fb, "tick %d after the solve" % t, solved=True)
    assert fa.fleet_plan_state()["plan_launches"] == launches
    fa.set_fleet(S, plans=True)                                                     # .. and on again: the first plan used is one solved with plans on
    p_cv, src = tw.prepare("tick 7, plans on again: switching on forgets the iterate's age", plans_on=False)
    _tick(tw, hs, 7)
    p_cv, src = tw.prepare("tick 8")
    assert src is not None and (src >= 0).any()
    _close(hs)


# ---- 4. the encounter sweep with plans on against the oracle's own run
def _sweep():
    spec = importlib.util.spec_from_file_location("pf_encounter_sweep", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "pf_encounter_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# The CPU oracle's own run of the same 32 scenes of 2 per kind with plans on (profiles/pf_encounter_plans_oracle.txt: `python
# tools/pf_encounter_oracle.py --scenes 32 --scene-size 2 --ticks 400 --plans`): missions finished, the slowest finish tick, the smallest
# min_separation, the smallest min_clearance.  Never the device's own figures.
ORACLE = {"parallel": (64, 197, 1.6019, 0.6019), "crossing": (64, 339, 1.3402, 0.3402), "head_on": (64, 197, 1.2095, 0.2095)}


@pytest.mark.parametrize("kind", scenario.PF_ENC_KINDS)
def test_encounter_sweep_with_plans_against_the_oracle(kind):
    """examples/pf_encounter_sweep.run(plans=True), device-resident, 1.5 x the oracle's slowest finish tick.  The finished count is the
    oracle's; the separations' margins are those of tests/test_gpu_pf_fleet.py."""
    finished, slowest, min_sep, min_clear = ORACLE[kind]
    r = _sweep().run(32, 2, (3 * slowest) // 2, kind=kind, quiet=True, plans=True)
    ft, ms, mc = r["finish_tick"], r["min_separation"], r["min_clearance"]
    fin = ft >= 0
    print("%s: finished %d of 64 (oracle %d); finish ticks %s" % (kind, fin.sum(), finished, ft.tolist()))
    print("min_separation %.4f (oracle %.4f): %s" % (ms.min(), min_sep, np.round(ms, 4).tolist()))
    print("min_clearance %.4f (oracle %.4f); failed solves %d; plan launches %d, plan-fed pairs %d"
          % (mc.min(), min_clear, r["failures_per_tick"].sum(), r["plan_launches"], r["plan_fed"]))
    assert r["plan_launches"] == (3 * slowest) // 2 - 1 and r["plan_fed"] > 0
    assert fin.sum() == finished
    assert ms.min() >= min_sep - 0.01
    assert mc.min() >= min_clear - 0.01
    assert np.array_equal(ms[0::2], ms[1::2])            # a scene of two: one distance, seen from either side
