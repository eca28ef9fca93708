"""Vessel encounters on a real MI355X (`pytest -m gpu`): the kernel usv_pf_fleet_gather, the C ABI usvmpc_pf_fleet / _fleet_state and
guidance.PathFollowingFrontEnd.set_fleet / fleet_state.

1. a fleet handle == a handle without one whose host rebuilds the scene every tick (scenario.fleet_world), bit for bit: the definition;
2. a scene run alone == the same scene inside a batch of 72;
3. "pf_predict" 0: stage 0 only, == a twin whose host re-uploads a world at rest every tick;
4. a finished instance keeps p / lh and is still seen by its scene-mates; set_fleet(0) == a handle that never had a fleet;
5. refusals;
6. the encounter sweep of examples/pf_encounter_sweep.py against the CPU oracle's own run (profiles/pf_encounter_oracle.txt).
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from mpc_collisionavoidance_amd import AcadosSim, BatchOcpSolver, BatchSimSolver, scenario, usv_models
from mpc_collisionavoidance_amd.guidance import PathFollowingFrontEnd

pytestmark = pytest.mark.gpu

M1, M2 = "usv_model_guidance_ca1", "usv_model_pf_ca"
DT, STEPS = 0.05, 5
B, N, T = 72, 6, 10        # (S = 3: scene 21 = instances 63, 64, 65 straddles usv_pf_prepare's 64-instance group)
LANE = 2.0
# a state the model can be linearised at: heading up leg 1 at 0.7 m/s (tests/test_gpu_pf_moving.py)
GENERIC = np.array([np.pi / 2, 1.0, 0.0, 0.7, 0.0, 0.0, 0.0, 4.0, -5.0, np.pi / 2, 4.0, -4.5, 0.0, 0.0])


def _solver(nB, K, x0):
    ocp = usv_models.make_ocp(M2, N * DT, N, K)
    ocp.solver_options.sim_method_num_steps = STEPS
    s = BatchOcpSolver(ocp, nB)
    s.set("x0", 0, x0)
    s.set_all("x", np.tile(x0[:, None, :], (1, N + 1, 1)))
    s.set_all("u", np.zeros((nB, N, 2)))
    s.set_all("yref", np.zeros((nB, N, 16)))
    s.set("yref", N, np.zeros((nB, 14)))
    return ocp, s


def _plant(ocp, nB):
    sim = AcadosSim()
    sim.model = ocp.model
    sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = DT, STEPS, False
    return BatchSimSolver(sim, nB)


def _scenes(S, n_fixed, seed):
    """72 vessels in scenes of S on neighbouring lanes LANE apart (+- 0.2 each: scene-mates 1.6 .. 2.4 m from their neighbour, inside
    max_radius and nearer than any fixed entry), all heading up their own leg 1; every scene is drawn from a stream of its own.  The fixed
    entries lie 3 m and more ahead and drift slowly."""
    wps, x0 = np.zeros((B, 3, 2)), np.tile(GENERIC, (B, 1))
    fixed, fvel = np.zeros((B, n_fixed, 3)), np.zeros((B, n_fixed, 2))
    for s in range(B // S):
        rng = np.random.default_rng([seed, s])
        for a in range(S):
            b = s * S + a
            x = 4.0 + a * LANE
            wps[b] = [[x, -5.0], [x, 1.0], [x + 4.0, 5.0]]
            x0[b, 7] = x
            x0[b, 10] = x + rng.uniform(-0.2, 0.2)
            x0[b, 11] = -4.5 + rng.uniform(-0.3, 0.3)
            x0[b, 0] += rng.uniform(-0.2, 0.2)
            x0[b, 4] = rng.uniform(-0.02, 0.02)
            fixed[b] = np.column_stack([x + rng.uniform(-4.0, 4.0, n_fixed), rng.uniform(-1.0, 0.5, n_fixed), rng.uniform(0.1, 0.3, n_fixed)])
            fvel[b] = rng.uniform(-0.1, 0.1, (n_fixed, 2))
    return wps, x0, fixed, fvel


def _parked(fixed, fvel, S):
    nB = fixed.shape[0]
    return (np.concatenate([fixed, np.tile([1000.0, 1000.0, 0.0], (nB, S - 1, 1))], axis=1),
            np.concatenate([fvel, np.zeros((nB, S - 1, 2))], axis=1))


def _host_scene(s, fe, S, n_fixed, radius):
    """What a handle without the fleet needs every tick: synchronise, read x0 and the world back, rebuild the trailing S - 1 entries and
    velocities in numpy, upload.  -> the separations [B, S-1]"""
    x0 = s.get("x0", 0)
    w, v = fe.world()
    ent, vel, sep = scenario.fleet_world(x0, S, radius)
    w[:, n_fixed:], v[:, n_fixed:] = ent, vel
    fe.set_world(w, vel=v)
    return sep


def _tick(s, fe, plant, t, noise):
    s.solve_async()
    fe.publish(fetch=False)
    if plant is None:
        s.advance(1e-3 if noise else 0.0, 100 + t)
    else:
        s.advance_sim(plant, 1e-3 if noise else 0.0, 100 + t)


def _same(sa, fa, sb, fb, what, solved):
    fields = ("x0", "p", "lh") + (("u", "x") if solved else ())
    for f in fields:
        a, b = (sa.get("x0", 0), sb.get("x0", 0)) if f == "x0" else (sa.get_all(f), sb.get_all(f))
        assert np.array_equal(a, b), (what, f)
    if solved:
        assert np.array_equal(sa.get_int("status"), sb.get_int("status")), (what, "status")
    sta, stb = fa.state(), fb.state()
    for k in sta:
        assert np.array_equal(sta[k], stb[k]), (what, k)


def _has_fleet_entry(p0, ent):
    """[B]: stage 0 of p holds at least one of the instance's fleet entries (X, Y)"""
    K = p0.shape[1] // 2
    slots = p0.reshape(p0.shape[0], K, 2)
    return (slots[:, :, None, :] == ent[:, None, :, :2]).all(axis=3).any(axis=(1, 2))


# ---- 1. the definition
@pytest.mark.parametrize("S,n_fixed,K,sim", [(2, 0, 4, True), (2, 5, 4, False), (3, 0, 4, False), (3, 5, 4, True), (4, 0, 4, True),
                                             (4, 5, 4, False), (3, 30, 20, True)])   # (K = 20: two obstacle chunks)
def test_fleet_handle_equals_its_host_fed_twin_bit_for_bit(S, n_fixed, K, sim):
    radius = 0.5 if S != 4 else 0.4
    wps, x0, fixed, fvel = _scenes(S, n_fixed, 10 * S + n_fixed)
    hs = []
    for fleet in (True, False):
        ocp, s = _solver(B, K, x0)
        s.set_option("disturbance_mask", (1 << 3) | (1 << 5))
        fe = PathFollowingFrontEnd(s)
        fe.reset(wps)
        if fleet:
            fe.set_world(fixed, vel=fvel if n_fixed else None)
            fe.set_fleet(S, radius)
        else:
            fe.set_world(_parked(fixed, fvel, S)[0], vel=_parked(fixed, fvel, S)[1])
        hs.append((s, fe, _plant(ocp, B) if sim else None))
    (sa, fa, pa), (sb, fb, pb) = hs
    w0, v0 = fa.world()
    assert np.array_equal(w0, _parked(fixed, fvel, S)[0]) and np.array_equal(v0, _parked(fixed, fvel, S)[1])   # fixed first, fleet parked
    ms, st = np.full(B, 1e300), np.full(B, -1)
    moved = False
    for t in range(T):
        sep = _host_scene(sb, fb, S, n_fixed, radius)
        for e in range(S - 1):
            win = sep[:, e] < ms
            ms[win], st[win] = sep[win, e], t
        fa.prepare(), fb.prepare()
        what = "S %d n_fixed %d K %d tick %d" % (S, n_fixed, K, t)
        _same(sa, fa, sb, fb, what, solved=False)
        (wa, va), (wb, vb) = fa.world(), fb.world()
        assert np.array_equal(wa, wb) and np.array_equal(va, vb), what + " world"
        assert np.array_equal(wa[:, :n_fixed, 2], fixed[:, :, 2]) and np.array_equal(va[:, :n_fixed], fvel), what + " fixed entries"
        p = sa.get_all("p")
        assert _has_fleet_entry(p[:, 0], wa[:, n_fixed:]).all(), what + ": an instance without a fleet entry among its K slots"
        moved |= bool((p[:, N] != p[:, 0]).any())
        fl = fa.fleet_state()
        assert np.array_equal(fl["min_separation"], ms) and np.array_equal(fl["separation_tick"], st), what + " fleet_state"
        _tick(sa, fa, pa, t, True), _tick(sb, fb, pb, t, True)
        _same(sa, fa, sb, fb, what + " after the solve", solved=True)
    assert moved, "the predicted stages never moved"
    assert (ms > 1.2).all() and (ms < 3 * LANE).all() and (st >= 0).all()
    for s, fe, plant in hs:
        s.close()
        if plant is not None:
            plant.close()


# ---- 2. a scene does not depend on its batch
def test_a_scene_alone_equals_the_scene_inside_the_batch():
    S, n_fixed, K = 3, 5, 4
    wps, x0, fixed, fvel = _scenes(S, n_fixed, 2)
    rows = {}
    for lo, hi in ((0, B), (63, 66), (0, 3)):
        nB = hi - lo
        ocp, s = _solver(nB, K, x0[lo:hi])
        fe = PathFollowingFrontEnd(s)
        fe.reset(wps[lo:hi])
        fe.set_world(fixed[lo:hi], vel=fvel[lo:hi])
        fe.set_fleet(S)
        plant = _plant(ocp, nB)
        rec = []
        for t in range(T):
            fe.prepare()
            rec.append([s.get("x0", 0), s.get_all("p"), s.get_all("lh"), *fe.world()])
            _tick(s, fe, plant, t, False)
            rec[-1] += [s.get_all("u"), fe.fleet_state()["min_separation"]]
        rows[(lo, hi)] = rec
        s.close(), plant.close()
    for lo, hi in ((63, 66), (0, 3)):
        for t in range(T):
            for full, alone in zip(rows[(0, B)][t], rows[(lo, hi)][t]):
                assert np.array_equal(full[lo:hi], alone), (lo, t)


# ---- 3. "pf_predict" 0
def test_pf_predict_0_holds_the_scene_still_inside_the_horizon():
    S, n_fixed, K = 3, 5, 4
    wps, x0, fixed, fvel = _scenes(S, n_fixed, 3)
    ocp, sa = _solver(B, K, x0)
    sa.set_option("pf_predict", 0)
    fa = PathFollowingFrontEnd(sa)
    fa.reset(wps)
    fa.set_world(fixed, vel=fvel)
    fa.set_fleet(S)
    ocp, sb = _solver(B, K, x0)
    fb = PathFollowingFrontEnd(sb)
    fb.reset(wps)
    w = fixed.copy()
    p_init = sa.get_all("p")
    for t in range(4):
        ent = scenario.fleet_world(sb.get("x0", 0), S, 0.5)[0]
        fb.set_world(np.concatenate([w, ent], axis=1))             # a world at rest, uploaded anew
        fa.prepare(), fb.prepare()
        pa = sa.get_all("p")
        assert np.array_equal(pa, sb.get_all("p")) and np.array_equal(sa.get_all("lh"), sb.get_all("lh")), t
        assert np.array_equal(pa[:, 1:], p_init[:, 1:]) and (pa[:, 0] != 0.0).all()      # stage 0 only
        assert _has_fleet_entry(pa[:, 0], ent).all()
        _tick(sa, fa, None, t, False), _tick(sb, fb, None, t, False)
        assert np.array_equal(sa.get_all("x"), sb.get_all("x")) and np.array_equal(sa.get_all("u"), sb.get_all("u")), t
        w[:, :, :2] = w[:, :, :2] + sa.dt * fvel
        assert np.array_equal(fa.world()[0][:, :n_fixed], w), t
    sa.close(), sb.close()


# ---- 4. untouched paths
def test_a_finished_instance_keeps_p_and_lh_and_is_still_seen():
    S, n_fixed, K = 3, 0, 4
    wps, x0, fixed, fvel = _scenes(S, n_fixed, 4)
    done = np.arange(B) % S == 1
    wps[done, 1, 1], wps[done, 2, 0], wps[done, 2, 1] = -4.6, wps[done, 0, 0], -4.4     # both waypoints within 1 m: over from tick 2
    ocp, s = _solver(B, K, x0)
    fe = PathFollowingFrontEnd(s)
    fe.reset(wps)
    fe.set_world(fixed)
    fe.set_fleet(S)
    plant = _plant(ocp, B)
    ms = np.full(B, 1e300)
    for t in range(5):
        if t >= 2:
            s.set_all("p", np.full((B, N + 1, 2 * K), -7.0 - t))
            s.set_all("lh", np.full((B, N, K), -3.0 - t))
        xb = s.get("x0", 0)
        ent, vel, sep = scenario.fleet_world(xb, S, 0.5)
        ms = np.minimum(ms, sep.min(axis=1))
        fe.prepare()
        p, lh = s.get_all("p"), s.get_all("lh")
        over = fe.state()["finish_tick"] >= 0
        assert np.array_equal(over, done & (t >= 2)), t
        if t >= 2:
            assert (p[over] == -7.0 - t).all() and (lh[over] == -3.0 - t).all(), t       # its own rows stay
        w, v = fe.world()
        assert np.array_equal(w, ent) and np.array_equal(v, vel), t                        # everybody is gathered, the finished one included
        assert _has_fleet_entry(p[~over, 0], ent[~over]).all()
        for i in np.nonzero(~done)[0]:                                                     # ... and every scene-mate has it among its K slots
            assert (p[i, 0].reshape(K, 2) == xb[i - i % S + 1, 10:12]).all(axis=1).any(), (t, i)
        assert np.array_equal(fe.fleet_state()["min_separation"], ms), t                   # the bookkeeping goes on for the finished ones too
        _tick(s, fe, plant, t, False)
    s.close(), plant.close()


def test_set_fleet_0_returns_to_a_handle_that_never_had_a_fleet():
    S, n_fixed, K = 3, 5, 4
    wps, x0, fixed, fvel = _scenes(S, n_fixed, 5)
    hs = []
    for fleet in (True, False):
        ocp, s = _solver(B, K, x0)
        fe = PathFollowingFrontEnd(s)
        fe.reset(wps)
        if fleet:
            fe.set_world(fixed, vel=fvel)
            fe.set_fleet(S)
        else:
            fe.set_world(_parked(fixed, fvel, S)[0], vel=_parked(fixed, fvel, S)[1])
        hs.append((s, fe, _plant(ocp, B)))
    (sa, fa, pa), (sb, fb, pb) = hs
    for t in range(3):
        _host_scene(sb, fb, S, n_fixed, 0.5)
        fa.prepare(), fb.prepare()
        _tick(sa, fa, pa, t, False), _tick(sb, fb, pb, t, False)
    wb, vb = fb.world()
    fa.set_fleet(0)
    fb.set_world(np.ascontiguousarray(wb[:, :n_fixed]), vel=np.ascontiguousarray(vb[:, :n_fixed]))   # what never having had one looks like
    wa, va = fa.world()
    assert wa.shape == (B, n_fixed, 3) and np.array_equal(wa, wb[:, :n_fixed]) and np.array_equal(va, fvel)   # the velocities are kept
    sep = fa.fleet_state()
    for t in range(3, 7):
        fa.prepare(), fb.prepare()
        _same(sa, fa, sb, fb, "tick %d" % t, solved=False)
        _tick(sa, fa, pa, t, False), _tick(sb, fb, pb, t, False)
        _same(sa, fa, sb, fb, "tick %d after the solve" % t, solved=True)
        assert np.array_equal(fa.world()[0], fb.world()[0]), t
    after = fa.fleet_state()
    assert np.array_equal(after["min_separation"], sep["min_separation"]) and np.array_equal(after["separation_tick"], sep["separation_tick"])
    fa.set_world(fixed)                       # and the world can be put at rest as ever
    assert np.array_equal(fa.world()[1], np.zeros((B, n_fixed, 2)))
    for s, fe, plant in hs:
        s.close(), plant.close()


# ---- 5. refusals
def test_refusals():
    nB, K, S, n_fixed = 12, 4, 3, 5
    E_ARG = -1
    dp = C.POINTER(C.c_double)
    wps, x0, fixed, fvel = _scenes(S, n_fixed, 6)
    wps, x0, fixed, fvel = wps[:nB], x0[:nB], np.ascontiguousarray(fixed[:nB]), np.ascontiguousarray(fvel[:nB])

    def err(s):
        return s._lib.usvmpc_last_error(s._h).decode()

    # another model
    s1 = BatchOcpSolver(usv_models.make_ocp(M1, N * DT, N, 8), nB)
    lib = s1._lib
    assert lib.usvmpc_pf_fleet(s1._h, S, 0.5) == E_ARG and "usv_model_pf_ca" in err(s1)
    assert lib.usvmpc_pf_fleet_state(s1._h, None, None) == E_ARG and "usv_model_pf_ca" in err(s1)
    s1.close()
    ocp, s = _solver(nB, K, x0)
    fe = PathFollowingFrontEnd(s)
    # no reset, no world list yet
    assert lib.usvmpc_pf_fleet(s._h, S, 0.5) == E_ARG and "come first" in err(s)
    fe.reset(wps)
    assert lib.usvmpc_pf_fleet(s._h, S, 0.5) == E_ARG and "come first" in err(s)
    fe.set_world(None)                        # an empty list will do
    fe.set_fleet(S)
    assert fe.world()[0].shape == (nB, S - 1, 3)
    fe.set_fleet(0)
    fe.set_world(fixed, vel=fvel)

    def unchanged():
        w, v = fe.world()
        return w.shape == (nB, n_fixed, 3) and np.array_equal(w, fixed) and np.array_equal(v, fvel)
    # the batch is not a whole number of scenes; too many entries; the radius
    assert lib.usvmpc_pf_fleet(s._h, 5, 0.5) == E_ARG and "whole number of scenes" in err(s) and unchanged()
    assert lib.usvmpc_pf_fleet(s._h, -2, 0.5) == E_ARG and "negative" in err(s) and unchanged()
    for bad in (-0.1, np.nan, np.inf):
        assert lib.usvmpc_pf_fleet(s._h, S, bad) == E_ARG and "radius" in err(s) and unchanged()
    big = np.ascontiguousarray(np.tile(fixed[:, :1], (1, 63, 1)))
    fe.set_world(big)
    assert lib.usvmpc_pf_fleet(s._h, S, 0.5) == E_ARG and "exceed the 64" in err(s) and fe.world()[0].shape == (nB, 63, 3)
    fe.set_world(fixed, vel=fvel)
    # the fleet is on
    fe.set_fleet(S)
    full = fe.world()
    assert full[0].shape == (nB, n_fixed + S - 1, 3)

    def fleet_unchanged():
        w, v = fe.world()
        return np.array_equal(w, full[0]) and np.array_equal(v, full[1])
    assert lib.usvmpc_pf_world(s._h, big.ctypes.data_as(dp), 63, 100.0) == E_ARG and "a fleet is on" in err(s) and fleet_unchanged()
    assert lib.usvmpc_pf_world_vel(s._h, None) == E_ARG and "a fleet is on" in err(s) and fleet_unchanged()
    vel_t, pose_t = np.tile([0.7, 0.0, 0.0], (nB, 1)), np.tile([4.0, -4.5, np.pi / 2], (nB, 1))
    before = (s.get("x0", 0), s.get_all("p"), fe.state()["wp_index"])
    with pytest.raises(Exception, match="on the device only"):
        fe.prepare(vel_t, pose_t)             # host-fed: the scene exists on the device only
    assert np.array_equal(s.get("x0", 0), before[0]) and np.array_equal(s.get_all("p"), before[1]) and fleet_unchanged()
    assert np.array_equal(fe.state()["wp_index"], before[2])
    s.set("obs_pos", 0, np.zeros((nB, K, 2)) + 50.0)
    with pytest.raises(Exception, match="a fleet is on"):
        s.set_option("obstacle_tracks", 1)
    assert fleet_unchanged()
    # what the fleet allows: new fixed entries (their velocities kept with the same count), new velocities, a step of every entry
    shifted, faster = fixed + 0.25, 2 * fvel
    assert lib.usvmpc_pf_world(s._h, shifted.ctypes.data_as(dp), n_fixed, 100.0) == 0
    w, v = fe.world()
    assert np.array_equal(w[:, :n_fixed], shifted) and np.array_equal(w[:, n_fixed:], full[0][:, n_fixed:]) and np.array_equal(v, full[1])
    assert lib.usvmpc_pf_world_vel(s._h, faster.ctypes.data_as(dp)) == 0
    assert np.array_equal(fe.world()[1][:, :n_fixed], faster) and np.array_equal(fe.world()[1][:, n_fixed:], full[1][:, n_fixed:])
    fe.prepare()
    w, v = fe.world()
    ent, vel, _ = scenario.fleet_world(s.get("x0", 0), S, 0.5)     # (x0[10], x0[11], u, v: prepare leaves them as they were)
    assert np.array_equal(w[:, n_fixed:, :2], ent[:, :, :2]) and (w[:, n_fixed:, 2] == 0.5).all()
    fe.step_world(0.1)
    w2 = fe.world()[0]
    assert np.array_equal(w2[:, :, :2], w[:, :, :2] + 0.1 * v) and np.array_equal(w2[:, :, 2], w[:, :, 2])
    fe.set_world(fixed[:, :2])                # another count of fixed entries: at rest, the fleet's slots stay
    w3, v3 = fe.world()
    assert w3.shape == (nB, 2 + S - 1, 3) and np.array_equal(w3[:, 2:], w2[:, n_fixed:]) and (v3[:, :2] == 0.0).all()
    # scene_size 1 is a fleet switched off
    ocp, s2 = _solver(nB, K, x0)
    f2 = PathFollowingFrontEnd(s2)
    f2.reset(wps)
    f2.set_world(fixed)
    f2.set_fleet(S, 0.3)
    f2.set_fleet(1)                           # scene_size 1: off
    assert f2.world()[0].shape == (nB, n_fixed, 3)
    s.close(), s2.close()


# ---- 6. the encounter sweep against the oracle's own run
def _sweep():
    spec = importlib.util.spec_from_file_location("pf_encounter_sweep", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "pf_encounter_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# The CPU oracle's own run of the same 32 scenes of 2 per kind (profiles/pf_encounter_oracle.txt: `python tools/pf_encounter_oracle.py
# --scenes 32 --scene-size 2 --ticks 400`): missions finished, the slowest finish tick, the smallest min_separation, the smallest
# min_clearance.  Never the device's own figures.  (The oracle alone finishes at least 48 of the 64 and keeps every separation above 1.0 m.)
ORACLE = {"parallel": (64, 197, 1.6019, 0.6019), "crossing": (64, 339, 1.3402, 0.3402), "head_on": (64, 197, 1.2857, 0.2857)}


@pytest.mark.parametrize("kind", scenario.PF_ENC_KINDS)
def test_encounter_sweep_against_the_oracle(kind):
    """examples/pf_encounter_sweep.run, device-resident, 1.5 x the oracle's slowest finish tick.  The margins are those of the two mission
    sweeps (tests/test_gpu_pf_frontend.py, tests/test_gpu_pf_moving.py): two instances at the edge of a hard row can fall either way inside
    the QP's exit tolerance."""
    finished, slowest, min_sep, min_clear = ORACLE[kind]
    assert finished >= 48 and min_sep > 1.0
    r = _sweep().run(32, 2, (3 * slowest) // 2, kind=kind, quiet=True)
    ft, ms, mc = r["finish_tick"], r["min_separation"], r["min_clearance"]
    fin = ft >= 0
    print("%s: finished %d of 64 (oracle %d); finish ticks %s" % (kind, fin.sum(), finished, ft.tolist()))
    print("min_separation %.4f (oracle %.4f): %s" % (ms.min(), min_sep, np.round(ms, 4).tolist()))
    print("min_clearance %.4f (oracle %.4f); failed solves %d" % (mc.min(), min_clear, r["failures_per_tick"].sum()))
    assert fin.sum() >= finished - 2
    assert ms.min() >= min_sep - 0.01
    assert mc.min() >= min_clear - 0.01
    assert np.array_equal(ms[0::2], ms[1::2])            # a scene of two: one distance, seen from either side
