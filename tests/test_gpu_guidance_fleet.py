"""Vessel encounters of the guidance front end on a real MI355X (`pytest -m gpu`): the kernel usv_guidance_fleet_gather, the C ABI
usvmpc_guidance_fleet / _fleet_state and guidance.GuidanceFrontEnd.set_fleet / fleet_state.

1. the gather against numpy (scenario.ca_fleet_world): positions and R bit for bit, velocities within 8 * 2^-52 * (|u| + |v|);
2. a fleet handle == a handle without one whose host uploads the fleet handle's world every tick, bit for bit;
3. predict 0: stage 0 only - the QP sees every stage of a fleet slot where stage 0 has it;
4. a finished instance keeps p / lh and is still seen by its scene-mates;
5. set_fleet(0) == a handle that never had a fleet;
6. a scene run alone == the same scene inside a batch;
7. the pipelined lineariser keeps running across fleet ticks;
8. refusals;
9. the encounter sweep of examples/ca_encounter_sweep.py against the CPU oracle's own run (profiles/guidance_encounter_oracle.txt).
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from mpc_collisionavoidance_amd import AcadosSim, BatchOcpSolver, BatchSimSolver, scenario, usv_models
from mpc_collisionavoidance_amd.guidance import GuidanceFrontEnd

pytestmark = pytest.mark.gpu

M1, M2 = "usv_model_guidance_ca1", "usv_model_pf_ca"
DT = 0.05
LANE = 2.0
R_SENSE = 18.0


def _solver(nB, N, K, x0):
    ocp = usv_models.make_ocp(M1, N * DT, N, K)
    s = BatchOcpSolver(ocp, nB)
    s.set("x0", 0, x0)
    s.set_all("x", np.tile(x0[:, None, :], (1, N + 1, 1)))
    s.set_all("u", np.zeros((nB, N, 1)))
    return ocp, s, GuidanceFrontEnd(s)


def _plant(ocp, nB):
    sim = AcadosSim()
    sim.model = ocp.model
    sim.solver_options.T, sim.solver_options.num_steps, sim.solver_options.sens_forw = DT, 4, False
    return BatchSimSolver(sim, nB)


def _scenes(nB, S, n_fixed, seed, any_heading=False):
    """nB vessels in scenes of S on neighbouring lanes LANE apart (+- 0.2 each: scene-mates 1.6 .. 2.4 m from their neighbour, inside
    R_SENSE and nearer than any fixed entry), heading up their own leg 1 (+- 0.3 rad) at about 0.7 m/s with a little sway; every scene is
    drawn from a stream of its own.  any_heading: psi anywhere in [-pi, pi], the first vessels on the quadrants' borders and at +-pi.  The
    fixed entries lie 3 m and more ahead and drift slowly."""
    wps, x0 = np.zeros((nB, 3, 2)), np.zeros((nB, 8))
    fixed, fvel = np.zeros((nB, n_fixed, 3)), np.zeros((nB, n_fixed, 2))
    edges = [np.pi, -np.pi, np.pi / 2, -np.pi / 2, 0.0, 3 * np.pi / 4, -3 * np.pi / 4, np.pi / 4, -np.pi / 4]
    for s in range(nB // S):
        rng = np.random.default_rng([seed, s])
        for a in range(S):
            b = s * S + a
            x = 4.0 + a * LANE
            wps[b] = [[x, -5.0], [x, 25.0], [x + 6.0, 30.0]]
            psi = np.pi / 2 + rng.uniform(-0.3, 0.3)
            if any_heading:
                psi = edges[b] if b < len(edges) else rng.uniform(-np.pi, np.pi)
            x0[b] = [0.7 + rng.uniform(-0.2, 0.2), rng.uniform(-0.05, 0.05), 0.0, 0.0, 0.0, x + rng.uniform(-0.2, 0.2), -4.5 + rng.uniform(-0.3, 0.3), psi]
            fixed[b] = np.column_stack([x + rng.uniform(-4.0, 4.0, n_fixed), rng.uniform(-1.0, 0.5, n_fixed), rng.uniform(0.1, 0.3, n_fixed)])
            fvel[b] = rng.uniform(-0.1, 0.1, (n_fixed, 2))
    return wps, x0, fixed, fvel


def _parked(fixed, fvel, S):
    nB = fixed.shape[0]
    return (np.concatenate([fixed, np.tile([1000.0, 1000.0, 0.0], (nB, S - 1, 1))], axis=1),
            np.concatenate([fvel, np.zeros((nB, S - 1, 2))], axis=1))


def _vel_bound(x0, S):
    xj = x0[scenario.fleet_vessels(x0.shape[0], S)]
    return (8 * 2.0 ** -52 * (np.abs(xj[..., 0]) + np.abs(xj[..., 1])))[..., None]


def _tick(s, fe, plant, t, noise):
    s.solve_async()
    out = fe.publish()
    if plant is None:
        s.advance(1e-3 if noise else 0.0, 100 + t)
    else:
        s.advance_sim(plant, 1e-3 if noise else 0.0, 100 + t)
    return out


def _same(sa, fa, sb, fb, what, solved):
    fields = ("x0", "p", "lh") + (("u", "x") if solved else ())
    for f in fields:
        a, b = (sa.get("x0", 0), sb.get("x0", 0)) if f == "x0" else (sa.get_all(f), sb.get_all(f))
        assert a.tobytes() == b.tobytes(), (what, f)
    if solved:
        assert np.array_equal(sa.get_int("status"), sb.get_int("status")), (what, "status")
    sta, stb = fa.mission_state(), fb.mission_state()
    for k in sta:
        assert sta[k].tobytes() == stb[k].tobytes(), (what, k)


def _holds(p0, xy, tol=1e-4):
    """[n]: stage 0 of p ([n, 2K]) holds the position xy ([n, 2]) in one of its slots (the front end rounds positions through float32)"""
    slots = p0.reshape(p0.shape[0], -1, 2)
    return (np.abs(slots - xy[:, None, :]).max(axis=2) < tol).any(axis=1)


# ---- 1. the gather against numpy
@pytest.mark.parametrize("nB,S,n_fixed", [(69, 3, 0),     # scene 21 = instances 63, 64, 65 straddles two workgroups of usv_guidance_tick
                                          (258, 3, 0),    # scene 42 = instances 126, 127, 128 straddles two 256-thread blocks of the gather
                                          (70, 2, 5), (68, 4, 0), (68, 4, 5)])
def test_gather_against_numpy(nB, S, n_fixed):
    N, K, radius = 8, 4, 0.5 if S != 4 else 0.4
    wps, x0, fixed, fvel = _scenes(nB, S, n_fixed, 100 * S + n_fixed, any_heading=True)
    ocp, s, fe = _solver(nB, N, K, x0)
    fe.reset(wps, x0[:, 7])
    fe.set_world(fixed, max_radius=R_SENSE, vel=fvel if n_fixed else None)
    fe.set_fleet(S, radius)
    w0, v0 = fe.world()
    assert np.array_equal(w0, _parked(fixed, fvel, S)[0]) and np.array_equal(v0, _parked(fixed, fvel, S)[1])   # fixed first, fleet parked
    st = fe.fleet_state()
    assert (st["min_separation"] == 1e300).all() and (st["separation_tick"] == -1).all()
    ms, wfix = np.full(nB, 1e300), fixed.copy()
    for t in range(2):
        xb = s.get("x0", 0)                                                       # read back just before
        ent, vel, sep = scenario.ca_fleet_world(xb, S, radius)
        ms = np.minimum(ms, sep.min(axis=1))
        fe.prepare()
        w, v = fe.world()
        assert w[:, n_fixed:].tobytes() == ent.tobytes(), t                       # positions and R: bit for bit
        dv = np.abs(v[:, n_fixed:] - vel)
        print("tick %d: largest velocity difference %.3g, in units of the bound %.3g" % (t, dv.max(), (dv / _vel_bound(xb, S)).max()))
        assert (dv <= _vel_bound(xb, S)).all(), t
        assert np.array_equal(w[:, :n_fixed], wfix) and np.array_equal(v[:, :n_fixed], fvel), t               # the fixed entries are left alone
        st = fe.fleet_state()
        assert st["min_separation"].tobytes() == ms.tobytes() and (st["separation_tick"] <= t).all() and (st["separation_tick"] >= 0).all(), t
        # prepare leaves what the gather reads as it was
        xa = s.get("x0", 0)
        assert np.array_equal(xa[:, [0, 1, 5, 6, 7]], xb[:, [0, 1, 5, 6, 7]])
        s.solve_async()
        s.advance(0.0, t)
        wfix[:, :, :2] = wfix[:, :, :2] + DT * fvel                               # (they move with advance, as any moving entry)
    s.close()


# ---- 2. the definition
@pytest.mark.parametrize("K,sim", [(4, False), (8, True)])   # 7 entries: K = 4 - the ranking chooses; K = 8 - some slots stay parked
def test_fleet_handle_equals_its_host_fed_twin_bit_for_bit(K, sim):
    nB, S, n_fixed, N, T, radius = 69, 3, 5, 12, 30, 0.5
    wps, x0, fixed, fvel = _scenes(nB, S, n_fixed, 7 + K)
    hs = []
    for fleet in (True, False):
        ocp, s, fe = _solver(nB, N, K, x0)
        if sim:
            s.set_option("disturbance_mask", (1 << 0) | (1 << 1) | (1 << 7))
        fe.reset(wps, x0[:, 7])
        if fleet:
            fe.set_world(fixed, max_radius=R_SENSE, vel=fvel)
            fe.set_fleet(S, radius)
        else:
            fe.set_world(_parked(fixed, fvel, S)[0], max_radius=R_SENSE, vel=_parked(fixed, fvel, S)[1])
        hs.append((s, fe, _plant(ocp, nB) if sim else None))
    (sa, fa, pa), (sb, fb, pb) = hs
    ms, st = np.full(nB, 1e300), np.full(nB, -1)
    moved = parked = ranked = False
    for t in range(T):
        what = "K %d tick %d" % (K, t)
        xb = sa.get("x0", 0)
        assert xb.tobytes() == sb.get("x0", 0).tobytes(), what + " x0 before prepare"
        dx, dy = xb[scenario.fleet_vessels(nB, S)][..., 5] - xb[:, None, 5], xb[scenario.fleet_vessels(nB, S)][..., 6] - xb[:, None, 6]
        sep = np.sqrt(dx * dx + dy * dy)                                          # numpy, over the read-back positions
        for e in range(S - 1):
            win = sep[:, e] < ms
            ms[win], st[win] = sep[win, e], t
        fa.prepare()
        w, v = fa.world()                                                         # the twin's host: the fleet handle's world, uploaded
        fb.set_world(w, max_radius=R_SENSE, vel=v)
        fb.prepare()
        _same(sa, fa, sb, fb, what, solved=False)
        assert np.array_equal(w[:, :n_fixed, 2], fixed[:, :, 2]) and np.array_equal(v[:, :n_fixed], fvel), what + " fixed entries"
        assert w[:, n_fixed:, :2].tobytes() == xb[scenario.fleet_vessels(nB, S)][..., 5:7].tobytes(), what + " fleet entries"
        p, lh = sa.get_all("p"), sa.get_all("lh")
        moved |= bool((p[:, N] != p[:, 0]).any())
        parked |= bool((lh[:, 0] == 0.0).any())
        ranked |= bool((lh[:, 0] != 0.0).all(axis=1).any())
        fl = fa.fleet_state()
        assert fl["min_separation"].tobytes() == ms.tobytes() and np.array_equal(fl["separation_tick"], st), what + " fleet_state"
        oa, ob = _tick(sa, fa, pa, t, sim), _tick(sb, fb, pb, t, sim)
        for f in oa:
            assert oa[f].tobytes() == ob[f].tobytes(), (what, "published", f)
        _same(sa, fa, sb, fb, what + " after the solve", solved=True)
    assert moved, "the predicted stages never moved"
    assert parked if K == 8 else ranked
    assert (ms > 0.5).all() and (ms < 3 * LANE).all() and (st >= 0).all()
    for s, fe, plant in hs:
        s.close()
        if plant is not None:
            plant.close()


# ---- 3. predict 0
def test_predict_0_holds_the_scene_still_inside_the_horizon():
    nB, S, n_fixed, N, K = 69, 3, 0, 8, 4
    wps, x0, fixed, fvel = _scenes(nB, S, n_fixed, 3)
    ocp, sa, fa = _solver(nB, N, K, x0)
    fa.reset(wps, x0[:, 7])
    fa.set_world(fixed, max_radius=R_SENSE)
    fa.set_fleet(S)
    fa.set_world(fixed, max_radius=R_SENSE, predict=False)
    ocp, sb, _ = _solver(nB, N, K, x0)                                            # a plain solver: stage 0 on every stage
    for t in range(3):
        sa.set_all("p", np.full((nB, N + 1, 2 * K), -5.0))
        sa.set_all("lh", np.full((nB, N, K), -6.0))
        xb = sa.get("x0", 0)
        fa.prepare()
        p, lh = sa.get_all("p"), sa.get_all("lh")
        assert (p[:, 1:] == -5.0).all() and (lh[:, 1:] == -6.0).all(), t          # stage 0 only
        for e in range(S - 1):
            assert _holds(p[:, 0], xb[scenario.fleet_vessels(nB, S)[:, e], 5:7]).all(), (t, e)
        assert (fa.world()[1] != 0.0).any()                                       # (the entries do have velocities: they are not used)
        sb.set("x0", 0, sa.get("x0", 0))
        sb.set_all("x", sa.get_all("x"))
        sb.set_all("u", sa.get_all("u"))
        sb.set_all("p", np.tile(p[:, :1], (1, N + 1, 1)))
        sb.set_all("lh", np.tile(lh[:, :1], (1, N, 1)))
        sa.solve(), sb.solve()
        assert sa.get_all("x").tobytes() == sb.get_all("x").tobytes() and sa.get_all("u").tobytes() == sb.get_all("u").tobytes(), t
        sa.advance(0.0, t)
    # ... and with predict 1 the same scene moves inside the horizon
    fa.set_world(fixed, max_radius=R_SENSE, predict=True)
    fa.prepare()
    p = sa.get_all("p").reshape(nB, N + 1, K, 2)
    assert (p[:, N, 0] != p[:, 0, 0]).any(axis=1).all()
    sa.close(), sb.close()


# ---- 4. a finished instance
def test_a_finished_instance_keeps_p_and_lh_and_is_still_seen():
    nB, S, n_fixed, N, K = 69, 3, 0, 8, 4
    wps, x0, fixed, fvel = _scenes(nB, S, n_fixed, 4)
    done = np.arange(nB) % S == 1
    wps[done, 1], wps[done, 2] = x0[done, 5:7] + [0.0, 0.3], x0[done, 5:7] + [0.0, 0.6]   # both within 1 m: a switch tick, then over
    ocp, s, fe = _solver(nB, N, K, x0)
    fe.reset(wps, x0[:, 7])
    fe.set_world(fixed, max_radius=R_SENSE)
    fe.set_fleet(S)
    ms = np.full(nB, 1e300)
    for t in range(5):
        if t >= 2:
            s.set_all("p", np.full((nB, N + 1, 2 * K), -7.0 - t))
            s.set_all("lh", np.full((nB, N, K), -3.0 - t))
        xb = s.get("x0", 0)
        ent, vel, sep = scenario.ca_fleet_world(xb, S, 0.5)
        ms = np.minimum(ms, sep.min(axis=1))
        fe.prepare()
        p, lh = s.get_all("p"), s.get_all("lh")
        over = fe.mission_state()["finish_tick"] >= 0
        assert np.array_equal(over, done & (t >= 1)), t
        if t >= 2:
            assert (p[over] == -7.0 - t).all() and (lh[over] == -3.0 - t).all(), t       # its own rows stay
            assert s.get("x0", 0)[over].tobytes() == xb[over].tobytes()                   # ... and its x0
        w, v = fe.world()
        assert w.tobytes() == ent.tobytes() and (np.abs(v - vel) <= _vel_bound(xb, S)).all(), t   # everybody is gathered, the finished one too
        for i in np.nonzero(~done)[0]:                                                     # ... and every scene-mate has it among its K slots
            assert _holds(p[i:i + 1, 0], xb[i - i % S + 1:i - i % S + 2, 5:7]).all(), (t, i)
        assert fe.fleet_state()["min_separation"].tobytes() == ms.tobytes(), t            # the bookkeeping goes on for the finished ones too
        _tick(s, fe, None, t, False)
    s.close()


# ---- 5. set_fleet(0)
def test_set_fleet_0_returns_to_a_handle_that_never_had_a_fleet():
    nB, S, n_fixed, N, K = 69, 3, 5, 8, 4
    wps, x0, fixed, fvel = _scenes(nB, S, n_fixed, 5)
    hs = []
    for fleet in (True, False):
        ocp, s, fe = _solver(nB, N, K, x0)
        fe.reset(wps, x0[:, 7])
        if fleet:
            fe.set_world(fixed, max_radius=R_SENSE, vel=fvel)
            fe.set_fleet(S)
        else:
            fe.set_world(_parked(fixed, fvel, S)[0], max_radius=R_SENSE, vel=_parked(fixed, fvel, S)[1])
        hs.append((s, fe))
    (sa, fa), (sb, fb) = hs
    for t in range(3):
        fa.prepare()
        w, v = fa.world()
        fb.set_world(w, max_radius=R_SENSE, vel=v)
        fb.prepare()
        _tick(sa, fa, None, t, False), _tick(sb, fb, None, t, False)
    wb, vb = fb.world()
    fa.set_fleet(0)
    fb.set_world(np.ascontiguousarray(wb[:, :n_fixed]), max_radius=R_SENSE, vel=np.ascontiguousarray(vb[:, :n_fixed]))   # never having had one
    wa, va = fa.world()
    assert wa.shape == (nB, n_fixed, 3) and np.array_equal(wa, wb[:, :n_fixed]) and np.array_equal(va, fvel)   # the velocities are kept
    sep = fa.fleet_state()
    for t in range(3, 7):
        fa.prepare(), fb.prepare()
        _same(sa, fa, sb, fb, "tick %d" % t, solved=False)
        _tick(sa, fa, None, t, False), _tick(sb, fb, None, t, False)
        _same(sa, fa, sb, fb, "tick %d after the solve" % t, solved=True)
        assert np.array_equal(fa.world()[0], fb.world()[0]), t
    after = fa.fleet_state()
    assert np.array_equal(after["min_separation"], sep["min_separation"]) and np.array_equal(after["separation_tick"], sep["separation_tick"])
    fa.sense(sa.get("x0", 0)[:, 5:8], fixed, max_radius=R_SENSE)                  # host-fed calls are allowed again
    fa.set_world(fixed, max_radius=R_SENSE)   # and the world can be put at rest as ever
    assert np.array_equal(fa.world()[1], np.zeros((nB, n_fixed, 2)))
    sa.close(), sb.close()


# ---- 6. a scene does not depend on its batch
def test_a_scene_alone_equals_the_scene_inside_the_batch():
    nB, S, n_fixed, N, K, T = 69, 3, 5, 8, 4, 8
    wps, x0, fixed, fvel = _scenes(nB, S, n_fixed, 2)
    rows = {}
    for lo, hi in ((0, nB), (63, 66), (0, 3)):
        n = hi - lo
        ocp, s, fe = _solver(n, N, K, x0[lo:hi])
        fe.reset(wps[lo:hi], x0[lo:hi, 7])
        fe.set_world(fixed[lo:hi], max_radius=R_SENSE, vel=fvel[lo:hi])
        fe.set_fleet(S)
        rec = []
        for t in range(T):
            fe.prepare()
            rec.append([s.get("x0", 0), s.get_all("p"), s.get_all("lh"), *fe.world()])
            _tick(s, fe, None, t, False)
            rec[-1] += [s.get_all("u"), s.get_all("x"), fe.fleet_state()["min_separation"]]
        rows[(lo, hi)] = rec
        s.close()
    for lo, hi in ((63, 66), (0, 3)):
        for t in range(T):
            for full, alone in zip(rows[(0, nB)][t], rows[(lo, hi)][t]):
                assert full[lo:hi].tobytes() == alone.tobytes(), (lo, t)


# ---- 7. the pipelined lineariser
def test_pipelined_lineariser_survives_fleet_ticks():
    nB, N, K, L, T, S = 16384, 20, 8, 5, 8, 2
    m = scenario.make_ca_missions(nB, L, seed=3)
    x0 = np.zeros((nB, 8))
    x0[:, 0:2], x0[:, 5:8] = m["vel"], m["pose"]
    x0[1::2, 5] += 2.5                                                            # (a scene's two vessels side by side, not on one spot)
    runs = {}
    for pipe in (1, 0):
        ocp, s, fe = _solver(nB, N, K, x0)
        s.set_option("pipeline_linearize", pipe)
        fe.reset(m["waypoints"], m["pose"][:, 2])
        fe.set_world(m["world"])
        fe.set_fleet(S)
        rec = []
        for i in range(T):
            fe.prepare()
            s.solve_async()
            fe.publish(fetch=False)
            s.advance(0.0, i)
            s.sync()
            rec.append((s.get_all("x"), s.get_all("u"), s.get("x0", 0)))
        runs[pipe] = (rec, s.pipeline_stats(), fe.world()[0])
        s.close()
    for i in range(T):
        for a, b in zip(runs[1][0][i], runs[0][0][i]):
            assert a.tobytes() == b.tobytes(), i
    used, discarded = runs[1][1]
    assert used >= 5 and discarded == 0, (used, discarded)
    assert runs[0][1] == (0, 0)
    assert (runs[1][2][:, L, 2] == 0.5).all() and (runs[1][2][:, L, 0] != 1000.0).all()   # (the fleet was on: the slot is gathered)


# ---- 8. refusals
def test_refusals():
    nB, N, K, S, n_fixed = 12, 8, 4, 3, 5
    E_ARG = -1
    dp = C.POINTER(C.c_double)
    wps, x0, fixed, fvel = _scenes(nB, S, n_fixed, 6)

    def err(s):
        return s._lib.usvmpc_last_error(s._h).decode()

    # another model
    s1 = BatchOcpSolver(usv_models.make_ocp(M2, N * 0.01, N, 4), nB)
    lib = s1._lib
    assert lib.usvmpc_guidance_fleet(s1._h, S, 0.5) == E_ARG and M1 in err(s1)
    assert lib.usvmpc_guidance_fleet_state(s1._h, None, None) == E_ARG and M1 in err(s1)
    s1.close()
    ocp, s, fe = _solver(nB, N, K, x0)
    # no reset, no world list yet
    assert lib.usvmpc_guidance_fleet(s._h, S, 0.5) == E_ARG and "usvmpc_guidance_reset" in err(s)
    fe.reset(wps, x0[:, 7])
    assert lib.usvmpc_guidance_fleet(s._h, S, 0.5) == E_ARG and "no world list yet" in err(s)
    fe.set_world(None)                        # an empty list will do
    fe.set_fleet(S)
    assert fe.world()[0].shape == (nB, S - 1, 3)
    fe.set_fleet(0)
    fe.set_world(fixed, max_radius=R_SENSE, vel=fvel)

    def works(n_entries):
        """the handle still prepares and solves, on a list of n_entries"""
        fe.prepare()
        st = s.solve()
        assert (st == 0).all() and np.isfinite(s.get_all("u")).all() and fe.world()[0].shape == (nB, n_entries, 3)
        s.set("x0", 0, x0)
        return True

    def unchanged():
        w, v = fe.world()
        return w.shape == (nB, n_fixed, 3) and np.array_equal(w, fixed) and np.array_equal(v, fvel) and works(n_fixed)
    # the batch is not a whole number of scenes; too many entries; the radius
    assert lib.usvmpc_guidance_fleet(s._h, 5, 0.5) == E_ARG and "whole number of scenes" in err(s) and unchanged()
    assert lib.usvmpc_guidance_fleet(s._h, -2, 0.5) == E_ARG and "negative" in err(s) and unchanged()
    for bad in (-0.1, np.nan, np.inf):
        assert lib.usvmpc_guidance_fleet(s._h, S, bad) == E_ARG and "radius" in err(s) and unchanged()
    big = np.ascontiguousarray(np.tile(fixed[:, :1], (1, 63, 1)))
    fe.set_world(big, max_radius=R_SENSE)
    assert lib.usvmpc_guidance_fleet(s._h, S, 0.5) == E_ARG and "exceed the 64" in err(s) and works(63)
    fe.set_world(fixed, max_radius=R_SENSE, vel=fvel)
    # the fleet is on
    fe.set_fleet(S)
    full = fe.world()
    assert full[0].shape == (nB, n_fixed + S - 1, 3)

    def fleet_unchanged():
        w, v = fe.world()
        return np.array_equal(w, full[0]) and np.array_equal(v, full[1])
    assert lib.usvmpc_guidance_world(s._h, big.ctypes.data_as(dp), 63, 100.0) == E_ARG and "a fleet is on" in err(s) and fleet_unchanged()
    assert lib.usvmpc_guidance_world_vel(s._h, None, 1) == E_ARG and "a fleet is on" in err(s) and fleet_unchanged()
    vel_t, pose_t = np.ascontiguousarray(x0[:, 0:2]), np.ascontiguousarray(x0[:, 5:8])
    before = (s.get("x0", 0), s.get_all("p"), fe.mission_state()["wp_index"])
    with pytest.raises(Exception, match="on the device only"):
        fe.prepare(vel_t, pose_t)             # host-fed: the scene exists on the device only
    with pytest.raises(Exception, match="on the device only"):
        fe.sense(pose_t, fixed, max_radius=R_SENSE)
    assert np.array_equal(s.get("x0", 0), before[0]) and np.array_equal(s.get_all("p"), before[1]) and fleet_unchanged()
    assert np.array_equal(fe.mission_state()["wp_index"], before[2])
    s.set("obs_pos", 0, np.zeros((nB, K, 2)) + 50.0)
    with pytest.raises(Exception, match="world moves"):
        s.set_option("obstacle_tracks", 1)
    assert fleet_unchanged()
    # what the fleet allows: new fixed entries (their velocities kept with the same count), new velocities, a step of every entry
    shifted, faster = fixed + 0.25, 2 * fvel
    assert lib.usvmpc_guidance_world(s._h, shifted.ctypes.data_as(dp), n_fixed, R_SENSE) == 0
    w, v = fe.world()
    assert np.array_equal(w[:, :n_fixed], shifted) and np.array_equal(w[:, n_fixed:], full[0][:, n_fixed:]) and np.array_equal(v, full[1])
    assert lib.usvmpc_guidance_world_vel(s._h, faster.ctypes.data_as(dp), 1) == 0
    assert np.array_equal(fe.world()[1][:, :n_fixed], faster) and np.array_equal(fe.world()[1][:, n_fixed:], full[1][:, n_fixed:])
    fe.prepare()                              # the handle works: the scene is gathered
    assert (s.solve() == 0).all()
    w, v = fe.world()
    ent = scenario.ca_fleet_world(s.get("x0", 0), S, 0.5)[0]     # (x0[5], x0[6]: prepare leaves them as they were)
    assert w[:, n_fixed:].tobytes() == ent.tobytes()
    fe.step_world(0.1)
    w2 = fe.world()[0]
    assert np.array_equal(w2[:, :, :2], w[:, :, :2] + 0.1 * v) and np.array_equal(w2[:, :, 2], w[:, :, 2])
    fe.set_world(fixed[:, :2], max_radius=R_SENSE)   # another count of fixed entries: at rest, the fleet's slots stay
    w3, v3 = fe.world()
    assert w3.shape == (nB, 2 + S - 1, 3) and np.array_equal(w3[:, 2:], w2[:, n_fixed:]) and (v3[:, :2] == 0.0).all()
    # scene_size 1 is a fleet switched off
    ocp, s2, f2 = _solver(nB, N, K, x0)
    f2.reset(wps, x0[:, 7])
    f2.set_world(fixed)
    f2.set_fleet(S, 0.3)
    f2.set_fleet(1)                           # scene_size 1: off
    assert f2.world()[0].shape == (nB, n_fixed, 3)
    s.close(), s2.close()


# ---- 9. the encounter sweep against the oracle's own run
def _sweep():
    spec = importlib.util.spec_from_file_location("ca_encounter_sweep", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "ca_encounter_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# The CPU oracle's own run of the same 32 scenes of 2 per kind (profiles/guidance_encounter_oracle.txt: `python
# tools/guidance_encounter_oracle.py --scenes 32 --scene-size 2 --ticks 400`): missions finished, the slowest finish tick, the smallest
# min_separation, the smallest min_clearance, failed solves.  Never the device's own figures.
ORACLE = {"parallel": (64, 196, 1.6094, 0.7412, 0), "crossing": (64, 338, 1.3755, 0.3755, 0), "head_on": (64, 196, 1.2738, 0.2738, 0)}


@pytest.mark.parametrize("kind", scenario.CA_ENC_KINDS)
def test_encounter_sweep_against_the_oracle(kind):
    """examples/ca_encounter_sweep.run, device-resident, N = 100, K = 8, 1.5 x the oracle's slowest finish tick.  The margins are those of
    the path-following sweeps (tests/test_gpu_pf_fleet.py): two instances at the edge of a row can fall either way inside the QP's exit
    tolerance."""
    finished, slowest, min_sep, min_clear, failed = ORACLE[kind]
    assert finished == 64 and failed == 0 and min_sep > 1.0 and slowest <= 400       # the condition the generator's constants were settled by
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
