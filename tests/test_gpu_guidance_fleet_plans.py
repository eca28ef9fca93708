"""Exchanged plans of the guidance front end on a real MI355X (`pytest -m gpu`): the kernel usv_guidance_fleet_plans, the C ABI
usvmpc_guidance_fleet_plans / _fleet_plan_state and guidance.GuidanceFrontEnd.set_fleet(plans=True) / fleet_plan_state, at the shapes of
tests/test_gpu_guidance_fleet.py (69 instances, S = 3, N = 8: scene 21 straddles two workgroups of usv_guidance_tick; 70 and 68 for S = 2, 4).

1. a handle with plans on == its twin with plans off whose host builds p with scenario.fleet_plan_stages every tick, bit for bit;
2. fallbacks: no mate chosen; a mate whose mission ends; prepare twice; advance twice;
3. a scene alone == the scene inside the batch; plans switched off again == never on; a handle that never switches them on;
4. the pipelined lineariser keeps running across ticks with plans on, 16 384 instances;
5. the encounter sweep with plans on against the CPU oracle's own run (profiles/guidance_encounter_plans_oracle.txt).
"""
import importlib.util
import os

import numpy as np
import pytest

from mpc_collisionavoidance_amd import scenario
from tests import test_gpu_guidance_fleet as base
from tests.fleet_plans_twin import Twin

pytestmark = pytest.mark.gpu

N, T = 8, 10
R_SENSE = base.R_SENSE
POS = scenario.FLEET_PLAN_POS["usv_model_guidance_ca1"]
NB = {2: 70, 3: 69, 4: 68}


def _pair(nB, S, n_fixed, K, sim, scenes, radius=0.5, noise=True):
    """(handle A: plans on, handle B: plans off), each (solver, front end, plant or None)"""
    wps, x0, fixed, fvel = scenes
    hs = []
    for plans in (True, False):
        ocp, s, fe = base._solver(nB, N, K, x0)
        if noise:
            s.set_option("disturbance_mask", (1 << 0) | (1 << 1) | (1 << 7))
        fe.reset(wps, x0[:, 7])
        fe.set_world(fixed, max_radius=R_SENSE, vel=fvel if n_fixed else None)
        fe.set_fleet(S, radius, plans=plans)
        hs.append((s, fe, base._plant(ocp, nB) if sim else None))
    return hs


def _twin(hs, S, n_fixed):
    (sa, fa, pa), (sb, fb, pb) = hs
    return Twin((sa, fa), (sb, fb), dict(S=S, n_fixed=n_fixed, pos=POS, tol=1e-4, finish=lambda fe: fe.mission_state()["finish_tick"],
                                         streams_before=True))


def _tick(tw, hs, t, noise=True):
    outs = [base._tick(s, fe, plant, t, noise) for s, fe, plant in hs]
    tw.solved(), tw.handed_over()
    for f in outs[0]:
        assert outs[0][f].tobytes() == outs[1][f].tobytes(), (t, "published", f)


def _close(hs):
    for s, fe, plant in hs:
        s.close()
        if plant is not None:
            plant.close()


# ---- 1. the definition
@pytest.mark.parametrize("S,n_fixed,sim", [(2, 0, True), (2, 5, False), (3, 0, False), (3, 5, True), (4, 0, True), (4, 5, False)])
def test_plans_handle_equals_its_host_fed_twin_bit_for_bit(S, n_fixed, sim):
    nB, K, radius = NB[S], 4, 0.5 if S != 4 else 0.4
    hs = _pair(nB, S, n_fixed, K, sim, base._scenes(nB, S, n_fixed, 10 * S + n_fixed), radius)
    (sa, fa, pa), (sb, fb, pb) = hs
    tw = _twin(hs, S, n_fixed)
    for t in range(T):
        what = "S %d n_fixed %d tick %d" % (S, n_fixed, t)
        p_cv, src = tw.prepare(what)
        if t == 0:
            assert src is None                                   # nothing solved yet: source is all -1 (held inside prepare)
        else:
            fed = (src >= 0).sum(axis=1)
            print("%s: plan-fed slots per instance %d .. %d, failed solves %d" % (what, fed.min(), fed.max(), (sb.get_int("status") != 0).sum()))
            assert (fed >= 1).all(), what + ": an instance without a plan-fed slot"
            assert (sa.get_all("p") != p_cv).any(), what + ": the plans changed nothing"
            assert sa.get_all("p")[:, 0].tobytes() == p_cv[:, 0].tobytes(), what + " stage 0"
        _tick(tw, hs, t)
        base._same(sa, fa, sb, fb, what + " after the solve", solved=True)
    never = fb.fleet_plan_state()                                # a handle that never switches plans on
    assert (never["source"] == -1).all() and never["plan_fed"] == 0 and never["plan_launches"] == 0
    assert fa.fleet_plan_state()["plan_launches"] == T - 1
    _close(hs)


# ---- 2. fallbacks
def test_no_mate_among_the_chosen_falls_back():
    """K = 1 and five fixed entries nearer than any scene-mate: the one slot holds a fixed entry, no plan is used, source is -1"""
    nB, S, n_fixed, K = 69, 3, 5, 1
    wps, x0, fixed, fvel = base._scenes(nB, S, n_fixed, 21)
    ang = np.linspace(0.3, 2.8, n_fixed)
    fixed[:, :, 0] = x0[:, None, 5] + np.cos(ang)[None, :] * np.linspace(1.0, 1.3, n_fixed)[None, :]    # 1.0 .. 1.3 m away; mates 1.6 m and more
    fixed[:, :, 1] = x0[:, None, 6] + np.sin(ang)[None, :] * np.linspace(1.0, 1.3, n_fixed)[None, :]
    fixed[:, :, 2] = 0.05
    fvel[:] = 0.0
    hs = _pair(nB, S, n_fixed, K, False, (wps, x0, fixed, fvel), noise=False)
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
    nB, S, n_fixed, K = 69, 3, 0, 4
    wps, x0, fixed, fvel = base._scenes(nB, S, n_fixed, 4)
    done = np.arange(nB) % S == 1
    wps[done, 1], wps[done, 2] = x0[done, 5:7] + [0.0, 0.3], x0[done, 5:7] + [0.0, 0.6]   # both within 1 m: a switch tick, then over
    hs = _pair(nB, S, n_fixed, K, False, (wps, x0, fixed, fvel), noise=False)
    (sa, fa, pa), (sb, fb, pb) = hs
    tw = _twin(hs, S, n_fixed)
    seen = []
    for t in range(5):
        p_cv, src = tw.prepare("tick %d" % t)
        over = fa.mission_state()["finish_tick"] >= 0
        assert np.array_equal(over, done & (t >= 1)), t
        if t >= 1:
            assert not np.isin(src, np.nonzero(done)[0]).any(), t                 # over from the prepare of tick 1 on: never followed
            assert ((src >= 0).sum(axis=1)[~done] >= 1).all(), t                  # the others still follow each other
            if t >= 2:
                assert (src[done] == -1).all(), t                                 # the finished instance does not stream (tick 1 was its last)
            seen.append(src)
        _tick(tw, hs, t, False)
        base._same(sa, fa, sb, fb, "tick %d after the solve" % t, solved=True)
    assert (seen[0][done] >= 0).any()                                             # (on the tick that ended its mission it still followed its mates)
    _close(hs)


@pytest.mark.parametrize("twice", ["prepare", "advance"])
def test_prepare_twice_and_advance_twice_give_todays_bits(twice):
    """prepare twice with no hand-over / advance twice with no solve: the second prepare / the next prepare is the constant-velocity
    prepare - B's host writes nothing - and plan_launches stays"""
    nB, S, n_fixed, K = 69, 3, 5, 4
    hs = _pair(nB, S, n_fixed, K, False, base._scenes(nB, S, n_fixed, 22))
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
    nB, S, n_fixed, K = 69, 3, 5, 4
    wps, x0, fixed, fvel = base._scenes(nB, S, n_fixed, 2)
    rows = {}
    for lo, hi in ((0, nB), (63, 66), (0, 3)):
        n = hi - lo
        ocp, s, fe = base._solver(n, N, K, x0[lo:hi])
        fe.reset(wps[lo:hi], x0[lo:hi, 7])
        fe.set_world(fixed[lo:hi], max_radius=R_SENSE, vel=fvel[lo:hi])
        fe.set_fleet(S, plans=True)
        rec = []
        for t in range(T):
            fe.prepare()
            rec.append([s.get("x0", 0), s.get_all("p"), s.get_all("lh"), fe.fleet_plan_state()["source"]])
            base._tick(s, fe, None, t, False)
            rec[-1] += [s.get_all("u"), s.get_all("x")]
        rows[(lo, hi)] = rec
        s.close()
    assert any((r[3] >= 0).any() for r in rows[(63, 66)])
    for lo, hi in ((63, 66), (0, 3)):
        for t in range(T):
            for k, (full, alone) in enumerate(zip(rows[(0, nB)][t], rows[(lo, hi)][t])):
                if k == 3:                                                         # source: vessel numbers count from the batch's first
                    assert np.array_equal(np.where(full[lo:hi] >= 0, full[lo:hi] - lo, -1), alone), (lo, t)
                else:
                    assert full[lo:hi].tobytes() == alone.tobytes(), (lo, t, k)


def test_plans_switched_off_again_equal_a_handle_that_never_had_them():
    nB, S, n_fixed, K = 69, 3, 5, 4
    hs = _pair(nB, S, n_fixed, K, True, base._scenes(nB, S, n_fixed, 23))
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
    tw.prepare("tick 7, plans on again: switching on forgets the iterate's age", plans_on=False)
    _tick(tw, hs, 7)
    p_cv, src = tw.prepare("tick 8")
    assert src is not None and (src >= 0).any()
    _close(hs)


# ---- 4. the pipelined lineariser
def test_pipelined_lineariser_survives_ticks_with_plans():
    """as tests/test_gpu_guidance_fleet.py::test_pipelined_lineariser_survives_fleet_ticks, plans on: the plan kernel writes p only - nothing
    a lineariser reads - so the linearisation made a tick ahead stands"""
    nB, Nh, K, L, Tn, S = 16384, 20, 8, 5, 8, 2
    m = scenario.make_ca_missions(nB, L, seed=3)
    x0 = np.zeros((nB, 8))
    x0[:, 0:2], x0[:, 5:8] = m["vel"], m["pose"]
    x0[1::2, 5] += 2.5                                                            # (a scene's two vessels side by side, not on one spot)
    runs = {}
    for pipe in (1, 0):
        ocp, s, fe = base._solver(nB, Nh, K, x0)
        s.set_option("pipeline_linearize", pipe)
        fe.reset(m["waypoints"], m["pose"][:, 2])
        fe.set_world(m["world"])
        fe.set_fleet(S, plans=True)
        rec = []
        for i in range(Tn):
            fe.prepare()
            s.solve_async()
            fe.publish(fetch=False)
            s.advance(0.0, i)
            s.sync()
            rec.append((s.get_all("x"), s.get_all("u"), s.get("x0", 0)))
        runs[pipe] = (rec, s.pipeline_stats(), fe.fleet_plan_state())
        s.close()
    for i in range(Tn):
        for a, b in zip(runs[1][0][i], runs[0][0][i]):
            assert a.tobytes() == b.tobytes(), i
    used, discarded = runs[1][1]
    assert used >= 5 and discarded == 0, (used, discarded)
    assert runs[0][1] == (0, 0)
    for pipe in (1, 0):
        st = runs[pipe][2]
        assert st["plan_launches"] == Tn - 1 and st["plan_fed"] > 0 and (st["source"] >= 0).any()      # (plans were on and fed slots)


# ---- 5. the encounter sweep with plans on against the oracle's own run
def _sweep():
    spec = importlib.util.spec_from_file_location("ca_encounter_sweep", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "ca_encounter_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# The CPU oracle's own run of the same 32 scenes of 2 per kind with plans on (profiles/guidance_encounter_plans_oracle.txt: `python
# tools/guidance_encounter_oracle.py --scenes 32 --scene-size 2 --ticks 400 --plans`): missions finished, the slowest finish tick, the smallest
# min_separation, the smallest min_clearance, failed solves.  Never the device's own figures.
ORACLE = {"parallel": (64, 196, 1.5983, 0.6132, 0), "crossing": (64, 338, 1.3755, 0.3755, 0), "head_on": (64, 196, 1.2916, 0.2916, 0)}


@pytest.mark.parametrize("kind", scenario.CA_ENC_KINDS)
def test_encounter_sweep_with_plans_against_the_oracle(kind):
    """examples/ca_encounter_sweep.run(plans=True), device-resident, N = 100, K = 8, 1.5 x the oracle's slowest finish tick.  The finished
    count is the oracle's; the separations' margins are those of tests/test_gpu_guidance_fleet.py."""
    finished, slowest, min_sep, min_clear, failed = ORACLE[kind]
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
