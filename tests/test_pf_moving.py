"""The path-following front end over a moving world, without a device: the moving-world arithmetic of csrc/pf_guidance.hpp (selection with
slot tracks, the per-stage obstacle set, the world step) compiled with the host compiler against its numpy restatement
(tests/pf_moving_ref.py, on tests/pf_frontend_ref.PfRef), the mission generator's velocities, scenario.predict_world, and the Python class's
refusals and shape helpers."""
import os
import subprocess
import types

import numpy as np
import pytest

from mpc_collisionavoidance_amd import scenario, usv_models
from mpc_collisionavoidance_amd.guidance import PathFollowingFrontEnd, _as_world_vel
from tests import pf_frontend_ref as R
from tests import pf_moving_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
B, N, T, DT = 37, 6, 12, 0.05
CASES = [(4, 0), (4, 3), (4, 9), (20, 30)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pf_moving") / "pf_moving_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "pf_moving_harness.cpp")])
    return exe


def run_harness(exe, tmp, wps, world, wvel, vel, pose, K, max_radius=12.0, margin=0.2):
    """-> list (per tick) of dicts of per-instance arrays"""
    nT, nB = vel.shape[0], vel.shape[1]
    npts, L = wps.shape[1], world.shape[1]
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    per_tick = np.concatenate([np.concatenate([vel[t].ravel(), pose[t].ravel()]) for t in range(nT)])
    np.concatenate([wps.ravel(), world.ravel(), wvel.ravel(), per_tick]).tofile(fin)
    r = subprocess.run([exe, str(nB), str(npts), str(L), str(K), str(N), str(nT), repr(float(max_radius)), repr(float(margin)), repr(DT), fin, fout],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok %d" % nB, r.stdout + r.stderr
    np_, nl = (N + 1) * 2 * K, N * K
    rec = np.fromfile(fout).reshape(nT, nB, 1 + K + 1 + np_ + nl + 3 * L)
    out = []
    for t in range(nT):
        a, o = rec[t], K + 2
        out.append(dict(phase=a[:, 0].astype(int), chosen=a[:, 1:1 + K].astype(int), min_clearance=a[:, 1 + K],
                        p=a[:, o:o + np_].reshape(nB, N + 1, 2 * K), lh=a[:, o + np_:o + np_ + nl].reshape(nB, N, K),
                        world=a[:, o + np_ + nl:].reshape(nB, L, 3)))
    return out


@pytest.fixture(scope="module")
def runs(harness, tmp_path_factory):
    """(K, L) -> (harness ticks, reference snapshots per tick, world, wvel): computed once, shared, left unchanged"""
    out = {}
    for K, L in CASES:
        rng = np.random.default_rng(140 + L)
        wps, vel, pose = R.scripted_sequence(B, T)
        world, wvel = MR.make_world(B, L, rng)
        got = run_harness(harness, tmp_path_factory.mktemp("run"), wps, world, wvel, vel, pose, K)
        ref = MR.PfMovingRef(B, N, K, DT)
        ref.reset(wps)
        ref.set_world(world, 12.0, wvel)
        snaps = []
        for t in range(T):
            ref.prepare(vel[t], pose[t])
            ref.step_world(DT)
            snaps.append(dict(phase=ref.phase.copy(), chosen=ref.chosen.copy(), p=ref.p.copy(), lh=ref.lh.copy(), world=ref.world.copy(),
                              min_clearance=ref.min_clearance.copy()))
        out[(K, L)] = (got, snaps, world, wvel)
    return out


# ---- 1. header == numpy, bit for bit
@pytest.mark.parametrize("K,L", CASES)
def test_header_equals_numpy_bit_for_bit(runs, K, L):
    got, snaps, world, wvel = runs[(K, L)]
    seen, moved = set(), False
    for t in range(T):
        g, r = got[t], snaps[t]
        for nm in ("phase", "chosen", "p", "lh", "world", "min_clearance"):
            assert np.array_equal(g[nm], r[nm]), (t, nm)
        seen |= set(r["phase"].tolist())
        live = r["phase"] != R.OVER
        assert np.array_equal(g["p"][live][:, 0].reshape(-1, K, 2)[r["chosen"][live] < 0], np.full(((r["chosen"][live] < 0).sum(), 2), 1000.0))
        if L:
            moved |= bool((g["p"][live][:, N] != g["p"][live][:, 0]).any())
    assert seen == {R.OVER, R.ACTIVE, R.SWITCH}
    assert moved == (L > 0)
    if L > K:
        assert any((got[t]["chosen"] != got[t + 1]["chosen"]).any() for t in range(T - 1))     # the selection changes as the world moves
    assert np.array_equal(got[-1]["world"][:, :, 2], world[:, :, 2])                             # R untouched


# ---- 2. consistency across ticks
@pytest.mark.parametrize("K,L", [(4, 9), (20, 30)])
def test_stage_1_is_the_next_ticks_stage_0(runs, K, L):
    got = runs[(K, L)][0]
    n = 0
    for t in range(T - 1):
        a, b = got[t], got[t + 1]
        same = (a["chosen"] == b["chosen"]).all(axis=1) & (a["phase"] != R.OVER) & (b["phase"] != R.OVER)
        assert np.array_equal(a["p"][same, 1], b["p"][same, 0]), t
        n += int(same.sum())
    assert n > B


# ---- 3. zero velocities == a world at rest
@pytest.mark.parametrize("K,L", [(4, 9), (20, 30)])
def test_zero_velocities_are_a_world_at_rest(harness, tmp_path, K, L):
    rng = np.random.default_rng(30 + L)
    wps, vel, pose = R.scripted_sequence(B, T)
    world, _ = MR.make_world(B, L, rng)
    got = run_harness(harness, tmp_path, wps, world, np.zeros((B, L, 2)), vel, pose, K)
    ref = R.PfRef(B, N, K)
    ref.reset(wps)
    ref.set_world(world, 12.0)
    p0, lh0 = np.zeros((B, 2 * K)), np.zeros((B, K))
    for t in range(T):
        ref.prepare(vel[t], pose[t])
        g = got[t]
        live = ref.phase != R.OVER
        p0[live], lh0[live] = ref.p0[live], ref.lh0[live]
        assert np.array_equal(g["p"], np.tile(p0[:, None], (1, N + 1, 1))) and np.array_equal(g["lh"], np.tile(lh0[:, None], (1, N, 1))), t
        assert np.array_equal(g["chosen"], ref.chosen) and np.array_equal(g["min_clearance"], ref.min_clearance), t
        assert np.array_equal(g["world"], world), t


# ---- 4. the generator, and scenario.predict_world
def test_generator_velocities_come_from_a_stream_of_their_own():
    a, m = scenario.make_pf_missions(5, seed=0), scenario.make_pf_missions(5, seed=0, moving=True)
    assert set(a) == {"waypoints", "world", "x0"} and set(m) == set(a) | {"world_vel"}
    for nm in a:
        assert np.array_equal(a[nm], m[nm]), nm
    # today's arrays, by the recorded values of tests/test_pf_frontend.py
    assert np.allclose(a["world"][0, 0], [2.911149300365291, -1.398026431839201, 0.10495829065855873], rtol=0, atol=1e-14)
    v = m["world_vel"]
    assert v.shape == (5, 4, 2) and np.isfinite(v).all() and (v != 0.0).all()
    assert np.array_equal(scenario.make_pf_missions(1, seed=2, moving=True)["world_vel"][0], v[2])      # seed + b: not the batch
    assert not np.array_equal(v[0], v[1])
    big = scenario.make_pf_missions(64, seed=0, moving=True)["world_vel"]
    w = scenario.PF_MISSION_WAYPOINTS
    for i in range(4):
        d = w[i % 2 + 1] - w[i % 2]
        e = d / np.hypot(*d)
        along, across = big[:, i] @ e, big[:, i] @ np.array([-e[1], e[0]])
        assert (np.abs(along) <= scenario.PF_DRIFT_ALONG + 1e-12).all() and (np.abs(across) <= scenario.PF_DRIFT_ACROSS + 1e-12).all()
        assert along.min() < 0 < along.max() and across.min() < 0 < across.max()


@pytest.mark.parametrize("K,L", [(4, 3), (20, 30)])
def test_predict_world_is_the_reference(runs, K, L):
    got, snaps, world, wvel = runs[(K, L)]
    p, lh = scenario.predict_world(world, wvel, snaps[0]["chosen"], N, DT, margin=0.2)
    live = snaps[0]["phase"] != R.OVER
    assert live.any() and (snaps[0]["chosen"] >= 0).any() and ((snaps[0]["chosen"] < 0).any() or L > K)     # (4, 3): parked slots
    assert np.array_equal(p[live], snaps[0]["p"][live]) and np.array_equal(lh[live], snaps[0]["lh"][live])


# ---- 5. the Python class on a stub solver
def test_python_class_checks_shapes_before_it_calls_the_library():
    nB = 3
    m2 = types.SimpleNamespace(ocp=usv_models.make_ocp("usv_model_pf_ca", 1.0, 20, 4), B=nB, _lib=None, generated=False)
    fe = PathFollowingFrontEnd(m2)
    w = np.arange(12, dtype=float).reshape(4, 3)
    v = np.arange(8, dtype=float).reshape(4, 2) / 10
    assert _as_world_vel(v, nB, 4).shape == (nB, 4, 2) and np.array_equal(_as_world_vel(v, nB, 4)[2], v) and _as_world_vel(v, nB, 4).flags.c_contiguous
    per = np.arange(nB * 8, dtype=float).reshape(nB, 4, 2)
    assert np.array_equal(_as_world_vel(per, nB, 4), per)
    assert _as_world_vel(np.zeros((0, 2)), nB, 0).shape == (nB, 0, 2)
    with pytest.raises(Exception, match="4 obstacles per instance, got 3"):
        fe.set_world(w, vel=v[:3])
    with pytest.raises(Exception, match="world velocities"):
        fe.set_world(w, vel=np.zeros((4, 3)))
    with pytest.raises(Exception, match="expected 3 instances"):
        fe.set_world(w, vel=np.zeros((nB + 1, 4, 2)))
    bad = v.copy()
    bad[1, 0] = np.inf
    with pytest.raises(Exception, match="NaN or infinity"):
        fe.set_world(w, vel=bad)
    with pytest.raises(Exception, match="set_world first"):
        fe.world()
    import inspect
    assert list(inspect.signature(fe.set_world).parameters) == ["world", "max_radius", "margin", "vel"]
    assert inspect.signature(fe.set_world).parameters["vel"].default is None
