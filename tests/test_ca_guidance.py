"""The guidance front end without a device: the arithmetic of csrc/ca_guidance.hpp compiled with the host compiler
(tests/ca_guidance_harness.cpp, a stand-alone program; built a second time with -fsanitize=address,undefined and run as a program)
against the restatement of the node in oracle/usv_guidance_oracle.c, and the device-resident tick (the sequence of the kernel
usv_guidance_tick, one instance) against the composition "oracle obstacle_sim -> oracle guidance_prepare" on the same pose, numpy's
clearance expression of examples/scenario_sweep.py and numpy's P + (k dt) v.

Both sides are host code built without contraction (-ffp-contract=off here, the oracle's Makefile likewise), so they are compared BIT FOR
BIT; the tolerances tests/test_guidance.py uses for the device against this oracle are asserted as well, as the bound that holds for any
build of the header."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
LM, W = 64, 4
WPS = np.array([[4.0, -5.0], [4.0, 25.0], [10.0, 30.0]])


def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra +
                          ["-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "ca_guidance_harness.cpp")])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """(plain build, sanitized build): every case runs through both and their outputs must be the same bytes"""
    tmp = tmp_path_factory.mktemp("ca_guidance")
    return _build(tmp, "ca_guidance_harness", []), _build(tmp, "ca_guidance_harness_san", ["-g", "-fsanitize=address,undefined",
                                                                                          "-fno-sanitize-recover=all"])


def call(harness, tmp_path, mode, records, nout, K=8, N=4, dt=0.05):
    rec = np.ascontiguousarray(records, dtype=np.float64)
    fin = str(tmp_path / "in.bin")
    rec.tofile(fin)
    outs = []
    for i, exe in enumerate(harness):
        fout = str(tmp_path / ("out%d.bin" % i))
        r = subprocess.run([exe, mode, str(K), str(N), repr(float(dt)), fin, fout], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok %d" % rec.shape[0], r.stdout + r.stderr
        outs.append(np.fromfile(fout).reshape(rec.shape[0], nout))
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


def pad_list(a, width):
    out = np.zeros((LM, width))
    a = np.asarray(a, dtype=float).reshape(-1, width)
    out[:len(a)] = a
    return out.ravel()


def pad_wp(w):
    out = np.zeros(2 * W)
    w = np.asarray(w, dtype=float).ravel()
    out[:w.size] = w
    return out


def body_lists(rng, K):
    """body-frame lists: every n of the issue (0, 1, K, K + 1, 64), n <= K and n > K at random, ten identical entries (ties)"""
    lists = []
    for n in [0, 1, K, K + 1, LM] + list(rng.integers(0, 30, 20)):
        lists.append(np.column_stack([rng.uniform(-15, 15, (n, 2)), rng.uniform(0.1, 1.5, n)]))
    lists.append(np.array([[1.0, 0.0, 0.2]] * 10))
    tie = np.column_stack([rng.uniform(-15, 15, (14, 2)), rng.uniform(0.1, 1.5, 14)])
    tie[3:13] = [2.0, -1.0, 0.4]                      # ten identical among others
    lists.append(tie)
    return lists


@pytest.mark.parametrize("K", [8, 3])
def test_selection_and_body2ned_are_the_oracles(harness, tmp_path, oracle, K):
    rng = np.random.default_rng(5 + K)
    lists = body_lists(rng, K)
    poses = np.column_stack([rng.uniform(-3.2, 3.2, len(lists)), rng.uniform(-20, 20, len(lists)), rng.uniform(-20, 20, len(lists))])
    rec = [np.concatenate([poses[i], [len(ob)], pad_list(ob, 3)]) for i, ob in enumerate(lists)]
    got = call(harness, tmp_path, "obstacles", rec, 4 * K, K=K)
    for i, ob in enumerate(lists):
        p, r, ch = oracle.guidance_obstacles(K, poses[i, 0], poses[i, 1], poses[i, 2], ob)
        assert list(got[i, 3 * K:].astype(int)) == list(ch), i                      # chosen indices: exact
        assert np.array_equal(got[i, 2 * K:3 * K], r), i                            # radii: exact
        assert np.allclose(got[i, :2 * K], p, rtol=2e-7, atol=2e-6), i              # positions: tests/test_guidance.py's bound
        assert got[i, :2 * K].tobytes() == p.tobytes(), i                           # ... and, host against host, the same bits
    assert list(got[-2, 3 * K:].astype(int)) == list(range(K))                      # ties: by list index


def test_simulator_is_the_oracles(harness, tmp_path, oracle):
    rng = np.random.default_rng(4)
    rec, cases = [], []
    for t, L in enumerate([0, 1, 8, 9, 64, 30, 30, 30, 30, 30]):
        world = np.column_stack([rng.uniform(-60, 60, L), rng.uniform(-60, 60, L), rng.uniform(0.2, 1.5, L)])
        pose = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-3.2, 3.2)])
        R = 100.0 if t % 2 else 35.0
        cases.append((pose, world, R))
        rec.append(np.concatenate([pose, [R, L], pad_list(world, 3)]))
    got = call(harness, tmp_path, "sim", rec, 1 + 3 * LM)
    for i, (pose, world, R) in enumerate(cases):
        want, n = oracle.obstacle_sim(pose, world, R)
        assert int(got[i, 0]) == n
        assert got[i, 1:1 + 3 * n].tobytes() == want.tobytes()


def prepare_cases(rng, K):
    """(vel, pose, k, past_psied, wps, obs): far from the switch, u = 0, inside the 1 m switch radius, the last segment (mission over
    at the switch, and k >= npts on entry), |chie| > pi, a two-point list"""
    obs = lambda n: np.column_stack([rng.uniform(-15, 15, (n, 2)), rng.uniform(0.1, 1.5, n)])
    c = [([0.7, 0.02], [1.0, 2.0, 0.4], 1, np.float32(0.3), WPS, obs(3)),
         ([0.0, 0.0], [1.0, 2.0, 0.4], 1, np.float32(0.3), WPS, obs(K)),
         ([0.7, 0.0], [4.2, 24.5, 1.5], 1, np.float32(-0.2), WPS, obs(K + 1)),
         ([0.7, 0.0], [4.2, 24.5, 1.5], 1, np.float32(3.0), WPS, obs(20)),             # re-referenced past_psied wraps
         ([0.7, 0.0], [10.2, 29.5, 0.0], 2, np.float32(0.1), WPS, obs(0)),             # the last segment ends: mission over
         ([0.7, 0.0], [10.0, 30.0, 0.0], 3, np.float32(0.1), WPS, obs(2)),             # over on entry
         ([-0.7, 0.0], [1.0, 2.0, 3.0], 1, np.float32(0.0), WPS, obs(LM)),             # |chie| > pi
         ([0.7, 0.0], [4.0, 24.5, 1.5], 1, np.float32(0.0), WPS[:2], obs(1))]          # two points, inside the radius: over
    for _ in range(40):
        pose = [rng.uniform(2, 6), rng.uniform(-5, 26), rng.uniform(-3.2, 3.2)]
        if rng.uniform() < 0.3:
            pose[0], pose[1] = 4.0 + rng.uniform(-0.9, 0.9), 25.0 + rng.uniform(-0.9, 0.9)
        c.append(([rng.uniform(-1.2, 1.2), rng.uniform(-0.1, 0.1)], pose, 1, np.float32(rng.uniform(-3.1, 3.1)), WPS, obs(int(rng.integers(0, 30)))))
    return c


@pytest.mark.parametrize("K", [8, 3])
def test_prepare_is_the_oracles(harness, tmp_path, oracle, K):
    rng = np.random.default_rng(17 + K)
    cases = prepare_cases(rng, K)
    rec = [np.concatenate([v, p, [k, pp, len(w)], pad_wp(w), [len(ob)], pad_list(ob, 3)]) for v, p, k, pp, w, ob in cases]
    got = call(harness, tmp_path, "prepare", rec, 13 + 3 * K, K=K)
    seen = set()
    for i, (v, p, k, pp, w, ob) in enumerate(cases):
        r = oracle.guidance_prepare(K, v, p, w.ravel(), ob, k, pp)
        g = got[i]
        assert int(g[0]) == r["active"] and int(g[1]) == r["k"], i                  # active, k: exact
        assert np.array_equal(g[13 + 2 * K:], r["r_obs"]) and g[13:13 + 2 * K].tobytes() == r["p_obs"].tobytes(), i
        seen.add((r["active"], r["k"]))
        if r["active"]:
            assert abs(g[2] - r["past_psied"]) <= 2.4e-7 and np.allclose(g[5:13], r["x0"], rtol=0, atol=3e-7), i   # tests/test_guidance.py's bounds
            assert np.float32(g[2]) == np.float32(r["past_psied"]) and g[5:13].tobytes() == r["x0"].tobytes(), i   # host against host: bits
            assert g[3] == r["ak"] and g[4] == r["ye"], i
    assert {(1, 1), (1, 2), (0, 3), (0, 2)} <= seen
    assert got[1, 5] == 0.001                                                        # u == 0 -> 0.001


def test_reset_and_publish_are_the_oracles(harness, tmp_path, oracle):
    rng = np.random.default_rng(2)
    psi = rng.uniform(-3.2, 3.2, 30)
    got = call(harness, tmp_path, "reset", [np.concatenate([WPS[:2].ravel(), [a]]) for a in psi], 2)
    for i, a in enumerate(psi):
        k, pp = oracle.guidance_reset(WPS.ravel(), a)
        assert int(got[i, 0]) == k and np.float32(got[i, 1]) == np.float32(pp)
    rec = np.column_stack([rng.uniform(-3.2, 3.2, 50), rng.uniform(-0.5, 0.5, 50), rng.uniform(-3.2, 3.2, 50)])
    rec[0] = [2.5, 0.0, np.pi / 2]                                                    # |psid| > pi
    got = call(harness, tmp_path, "publish", rec, 4)
    for i, (x1, u0, ak) in enumerate(rec):
        o = oracle.guidance_publish(x1, u0, ak, 0.0)
        assert got[i, 0] == o["heading"] and got[i, 1] == o["r"] and got[i, 2] == 0.7 and np.float32(got[i, 3]) == np.float32(o["past_psied"])


def tick_record(x0, k, pp, wps, world, wvel, max_radius, predict, min_clear, finish, tick, p, lh):
    return np.concatenate([x0, [k, pp, len(wps)], pad_wp(wps), [len(world), max_radius, predict, min_clear, finish, tick],
                           pad_list(world, 3), pad_list(wvel, 2), p.ravel(), lh.ravel()])


@pytest.mark.parametrize("K,L", [(8, 0), (8, 1), (8, 8), (8, 9), (8, 12), (3, 64)])
def test_resident_tick_is_simulator_then_prepare(harness, tmp_path, oracle, K, L):
    """x0 carries the state; the tick = oracle obstacle_sim at x0's pose -> oracle guidance_prepare; min_clearance = numpy's expression of
    examples/scenario_sweep.py over the visible entries, bit for bit; a predicted moving world = numpy's P + (k dt) v, bit for bit."""
    N, dt, max_radius = 4, 0.05, 18.0
    rng = np.random.default_rng(100 * K + L)
    cases = prepare_cases(rng, K)
    nin_p, nin_lh = (N + 1) * 2 * K, N * K
    rec, meta = [], []
    for j, (v, pose, k, pp, w, _) in enumerate(cases):
        far = 10.0 if j % 4 < 2 else 25.0                                              # (every entry visible / some beyond max_radius)
        world = np.column_stack([pose[0] + rng.uniform(-far, far, L), pose[1] + rng.uniform(-far, far, L), rng.uniform(0.2, 1.5, L)])
        if L >= 12:
            world[1:11] = [pose[0] + 3.0, pose[1] - 2.0, 0.4]                         # ten identical entries, visible
        wvel = rng.uniform(-0.3, 0.3, (L, 2))
        x0 = np.array([v[0], v[1], 9.0, 9.0, 9.0, pose[0], pose[1], pose[2]])          # (ye, chie, psied: whatever advance left)
        predict = j % 2
        mc0 = 1e300 if j % 3 else 0.05
        p, lh = rng.uniform(-1, 1, nin_p), rng.uniform(-1, 1, nin_lh)                  # sentinels
        rec.append(tick_record(x0, k, pp, w, world, wvel, max_radius, predict, mc0, -1, 7, p, lh))
        meta.append((x0, k, pp, w, world, wvel, predict, mc0, p, lh))
    nout = 15 + K + nin_p + nin_lh
    got = call(harness, tmp_path, "tick", rec, nout, K=K, N=N, dt=dt)
    some_more, some_fewer = False, False
    for j, (x0, k, pp, w, world, wvel, predict, mc0, p_in, lh_in) in enumerate(meta):
        g = got[j]
        gx0, gk, gpp, gact, gmc, gfin = g[:8], int(g[8]), np.float32(g[9]), int(g[10]), g[13], int(g[14])
        chosen = g[15:15 + K].astype(int)
        gp = g[15 + K:15 + K + nin_p].reshape(N + 1, 2 * K)
        glh = g[15 + K + nin_p:].reshape(N, K)
        if k >= len(w):                                                              # over on entry: everything is kept
            assert gx0.tobytes() == x0.tobytes() and gp.tobytes() == p_in.tobytes() and glh.tobytes() == lh_in.tobytes()
            assert gfin == 7 and gmc == mc0 and gk == k
            continue
        pose = x0[5:8]
        body, n = oracle.obstacle_sim(pose, world, max_radius)
        some_more |= n > K
        some_fewer |= 0 < n <= K
        r = oracle.guidance_prepare(K, x0[0:2], pose, w.ravel(), body, k, pp)
        assert gact == r["active"] and gk == r["k"], j
        assert gp[0].tobytes() == r["p_obs"].tobytes() and glh[0].tobytes() == r["r_obs"].tobytes(), j
        if r["active"]:
            assert gx0.tobytes() == r["x0"].tobytes() and gpp == np.float32(r["past_psied"]), j
            assert gfin == -1
        else:
            assert gx0.tobytes() == x0.tobytes() and gfin == 7, j
        # the chosen WORLD indices: the visible ones in list order, then the oracle's choice among them
        d = np.sqrt((pose[0] - world[:, 0]) ** 2 + (pose[1] - world[:, 1]) ** 2) - (world[:, 2] + 0.5)
        vis = np.nonzero(np.sqrt((world[:, 0] - pose[0]) ** 2 + (world[:, 1] - pose[1]) ** 2) < max_radius)[0]
        assert len(vis) == n
        _, _, ch = oracle.guidance_obstacles(K, pose[2], pose[0], pose[1], body)
        assert list(chosen) == [vis[c] if c >= 0 else -1 for c in ch], j
        want_mc = min(mc0, d[vis].min()) if n else mc0
        assert gmc == want_mc, j                                                      # numpy's bits
        if predict:
            P = r["p_obs"].reshape(K, 2)
            v = np.array([wvel[c] if c >= 0 else (0.0, 0.0) for c in chosen]).reshape(K, 2)
            kdt = (np.arange(N + 1, dtype=float) * dt)[:, None, None]
            want = (P[None] + kdt * v[None]).reshape(N + 1, 2 * K)
            assert gp.tobytes() == want.tobytes(), j
            assert glh.tobytes() == np.tile(r["r_obs"][None], (N, 1)).tobytes(), j
            parked = chosen < 0
            assert np.all(gp.reshape(N + 1, K, 2)[:, parked] == 1000.0) and np.all(glh[:, parked] == 0.0)
        else:
            assert gp[1:].tobytes() == p_in.reshape(N + 1, 2 * K)[1:].tobytes() and glh[1:].tobytes() == lh_in.reshape(N, K)[1:].tobytes(), j
    if L > K:
        assert some_more
    if 0 < L:
        assert some_fewer or L > K
