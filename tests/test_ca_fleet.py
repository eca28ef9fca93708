"""Vessel encounters of the guidance front end without a device: the arithmetic of csrc/ca_fleet_world.hpp (the gather of a scene's vessels
into fleet entries, the separation bookkeeping) compiled with the host compiler - plain, and under the address and undefined-behaviour
sanitizers - against its numpy restatement scenario.ca_fleet_world, the encounter generator, and the Python class's bookkeeping.

Indices, positions, radius, separations, the running minimum and its tick: bit for bit.  Velocities: two libraries' sin / cos stand behind
them, each within 4 ulp of the true value (OpenCL's bound, the widest of the libraries in play), so each product u cos, v sin, ... is off by
at most 4 ulp of its factor plus its own rounding, and the sum adds one more: |vX - numpy's|, |vY - numpy's| <= 8 * 2^-52 * (|u| + |v|)."""
import os
import subprocess
import types

import numpy as np
import pytest

from mpc_collisionavoidance_amd import _capi, scenario
from mpc_collisionavoidance_amd.guidance import GuidanceFrontEnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
T = 6
CASES = [(2, 70, 0), (3, 69, 5), (4, 68, 0), (5, 70, 3), (2, 2, 1), (3, 3, 0), (5, 5, 59)]   # (S, B, n_fixed)
PSI_EDGES = [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, np.nextafter(np.pi, 0.0), -np.nextafter(np.pi, 0.0), 3 * np.pi / 4, -3 * np.pi / 4,
             np.pi / 4, -np.pi / 4, 1e-300, -0.0, 7.5, -12.0]          # the four quadrants, their borders, +-pi, and an unwrapped heading


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ca_fleet") / ("ca_fleet_world_harness_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "ca_fleet_world_harness.cpp")])
    return exe


def call(exe, tmp, args, data=None):
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    argv = [exe] + [str(a) for a in args]
    if data is not None:
        np.ascontiguousarray(data, dtype=np.float64).tofile(fin)
        argv.append(fin)
    r = subprocess.run(argv + [fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    return np.fromfile(fout)


def random_states(B, rng):
    """[T, B, 8] vessel states (u, v, ye, chie, psied, xned, yned, psi): speeds of either sign, u = v = 0, headings in every quadrant and
    on the quadrants' borders, a NaN state, two vessels on one spot"""
    x = rng.normal(0.0, 3.0, (T, B, 8))
    x[:, :, 0] = rng.uniform(-1.0, 1.0, (T, B))
    x[:, :, 1] = rng.uniform(-0.3, 0.3, (T, B))
    x[:, :, 7] = rng.uniform(-np.pi, np.pi, (T, B))
    x[0, :, 7] = np.resize(PSI_EDGES, B)
    x[1, 0::5, 0] = x[1, 0::5, 1] = 0.0              # at rest
    x[2, 1::7, 0] = -0.7                             # astern
    if B > 4:
        x[3, 4] = np.nan                             # a NaN state: its scene-mates' entries are NaN, no minimum is taken from it
        x[4, B - 1, 5:7] = x[4, B - 2, 5:7]          # separation 0
    return x


def vel_bound(x, S):
    """[B, S-1, 1]: 8 * 2^-52 * (|u| + |v|) of the vessel behind each fleet slot"""
    xj = x[scenario.fleet_vessels(x.shape[0], S)]
    return (8 * 2.0 ** -52 * (np.abs(xj[..., 0]) + np.abs(xj[..., 1])))[..., None]


def numpy_run(x, S, n_fixed, radius):
    """per tick (world, wvel, min_sep, sep_tick) by scenario.ca_fleet_world and the running minimum's rule, the lists starting as 7.0"""
    B = x.shape[1]
    world, wvel = np.full((B, n_fixed + S - 1, 3), 7.0), np.full((B, n_fixed + S - 1, 2), 7.0)
    ms, st = np.full(B, 1e300), np.full(B, -1)
    out = []
    for t in range(x.shape[0]):
        ent, vel, sep = scenario.ca_fleet_world(x[t], S, radius)
        world[:, n_fixed:], wvel[:, n_fixed:] = ent, vel
        for e in range(S - 1):
            for i in range(B):
                if sep[i, e] < ms[i]:
                    ms[i], st[i] = sep[i, e], t
        out.append((world.copy(), wvel.copy(), ms.copy(), st.copy()))
    return out


@pytest.mark.parametrize("S,B,n_fixed", CASES)
def test_gather_matches_numpy(harness, tmp_path, S, B, n_fixed):
    x = random_states(B, np.random.default_rng(100 * S + B))
    radius = 0.5 if S != 3 else 0.37
    got = call(harness, tmp_path, ["gather", B, S, n_fixed, repr(radius), T], x).reshape(T, -1)
    nw = n_fixed + S - 1
    for t, (world, wvel, ms, st) in enumerate(numpy_run(x, S, n_fixed, radius)):
        g = got[t]
        gw, gv = g[:B * nw * 3].reshape(B, nw, 3), g[B * nw * 3:B * nw * 5].reshape(B, nw, 2)
        gms, gst = g[B * nw * 5:B * nw * 5 + B], g[B * nw * 5 + B:]
        assert gw.tobytes() == world.tobytes(), "world, tick %d" % t            # (bytes: NaN entries and signed zeros included)
        dv = np.abs(gv[:, n_fixed:] - wvel[:, n_fixed:])
        nan = np.isnan(wvel[:, n_fixed:])
        assert np.array_equal(np.isnan(gv[:, n_fixed:]), nan), "velocities' NaNs, tick %d" % t
        assert (dv[~nan] <= np.broadcast_to(vel_bound(x[t], S), dv.shape)[~nan]).all(), "velocities, tick %d" % t
        assert gms.tobytes() == ms.tobytes(), "min_separation, tick %d" % t
        assert np.array_equal(gst.astype(int), st), "separation_tick, tick %d" % t
        assert (gw[:, :n_fixed] == 7.0).all() and (gv[:, :n_fixed] == 7.0).all()   # the layout: fixed entries first, left alone
    if B > 4:
        assert not np.isnan(gms).any()                    # a NaN never wins
        assert np.isnan(got[3][:B * nw * 3]).any()        # (the NaN state did reach its scene-mates' lists)
        assert gms[B - 1] == 0.0 and gst[B - 1] == 4


def test_ca_fleet_world_restates_the_issue():
    """scenario.ca_fleet_world against the formulas written out per instance, in Python floats; first, middle and last of a scene"""
    S, B = 5, 10
    x = random_states(B, np.random.default_rng(3))[0]
    ent, vel, sep = scenario.ca_fleet_world(x, S, 0.5)
    assert ent.shape == (B, S - 1, 3) and vel.shape == (B, S - 1, 2) and sep.shape == (B, S - 1)
    for i in range(B):
        s, a = divmod(i, S)
        for e in range(S - 1):
            xj = x[s * S + (e if e < a else e + 1)]
            c, sn = np.cos(xj[7]), np.sin(xj[7])
            assert ent[i, e].tolist() == [xj[5], xj[6], 0.5]
            assert vel[i, e].tolist() == [xj[0] * c - xj[1] * sn, xj[0] * sn + xj[1] * c]
            dx, dy = xj[5] - x[i, 5], xj[6] - x[i, 6]
            assert sep[i, e] == np.sqrt(dx * dx + dy * dy)
    # a vessel sailing ahead at 0.7 m/s moves where its bow points
    y = np.zeros((2, 8))
    y[:, 0], y[:, 7] = 0.7, [np.pi / 2, np.pi]
    v = scenario.ca_fleet_world(y, 2, 0.5)[1][:, 0]
    assert np.allclose(v, [[-0.7, 0.0], [0.0, 0.7]], atol=1e-15)
    with pytest.raises(ValueError):
        scenario.ca_fleet_world(x, 4, 0.5)


@pytest.mark.parametrize("S,B", [(2, 6), (3, 9), (4, 8), (5, 15)])
def test_slot_to_vessel_map(harness, tmp_path, S, B):
    got = call(harness, tmp_path, ["map", B, S]).reshape(B, S - 1).astype(int)
    assert np.array_equal(got, scenario.fleet_vessels(B, S))
    for i in range(B):
        s = i // S
        assert got[i].tolist() == [j for j in range(s * S, s * S + S) if j != i]      # the scene's vessels in order, itself left out


def test_min_separation_is_symmetric_in_a_scene_of_two():
    x = random_states(8, np.random.default_rng(9))[0]
    sep = scenario.ca_fleet_world(x, 2, 0.5)[2][:, 0]
    assert sep[0::2].tobytes() == sep[1::2].tobytes()


@pytest.mark.parametrize("kind", scenario.CA_ENC_KINDS)
def test_encounters_do_not_depend_on_the_batch(kind):
    a = scenario.make_ca_encounters(6, 2, seed=3, kind=kind)
    assert a["waypoints"].shape == (12, 3, 2) and a["pose"].shape == (12, 3) and a["x0"].shape == (12, 8) and a["world"].shape == (12, 0, 3)
    for s in (0, 4):
        one = scenario.make_ca_encounters(1, 2, seed=3 + s, kind=kind)
        for f in ("waypoints", "pose", "vel", "x0"):
            assert np.array_equal(one[f], a[f][2 * s:2 * s + 2]), f
    x0 = a["x0"]
    assert np.array_equal(x0[:, 5:8], a["pose"]) and np.array_equal(x0[:, 0:2], a["vel"]) and (x0[:, 0] == 0.7).all() and (x0[:, 2:5] == 0).all()
    # nobody starts inside a scene-mate's keep-out circle (hulls of 0.5 m: 1.0 m between centres), and everybody starts on its first leg
    assert scenario.ca_fleet_world(x0, 2, 0.5)[2].min() > 1.0
    three = scenario.make_ca_encounters(2, 3, seed=0, kind=kind)
    assert scenario.ca_fleet_world(three["x0"], 3, 0.5)[2].min() > 1.0
    leg = a["waypoints"][:, 1] - a["waypoints"][:, 0]
    assert np.allclose(np.arctan2(leg[:, 1], leg[:, 0]), a["pose"][:, 2])
    with pytest.raises(ValueError):
        scenario.make_ca_encounters(1, 2, kind="overtaking")


def test_each_kind_has_its_shape():
    """headings of vessel 0 and vessel 1 of a scene, and where their first legs lie"""
    want = {"parallel": (np.pi / 2, np.pi / 2), "crossing": (np.pi / 2, np.pi), "head_on": (np.pi / 2, -np.pi / 2)}
    for kind, (h0, h1) in want.items():
        m = scenario.make_ca_encounters(8, 2, seed=1, kind=kind)
        wp, pose = m["waypoints"], m["pose"]
        assert (pose[0::2, 2] == h0).all() and (pose[1::2, 2] == h1).all(), kind
        dx = wp[1::2, 0, 0] - wp[0::2, 0, 0]
        if kind == "parallel":                            # side by side, one lane apart
            assert (np.abs(dx - scenario.CA_ENC_LANE) <= 2 * scenario.CA_ENC_LANE_JITTER + 1e-12).all()
        elif kind == "crossing":                          # the westbound leg cuts the northbound one, and is reached later
            y = wp[1::2, 0, 1]
            assert ((wp[0::2, 0, 1] < y) & (y < wp[0::2, 1, 1])).all() and ((wp[1::2, 1, 0] < wp[0::2, 0, 0]) & (wp[0::2, 0, 0] < wp[1::2, 0, 0])).all()
            reach0, reach1 = y - pose[0::2, 1], pose[1::2, 0] - wp[0::2, 0, 0]
            assert (reach1 - reach0 >= scenario.CA_ENC_CROSS_OFFSET - 2 * scenario.CA_ENC_STAGGER - 2 * scenario.CA_ENC_LANE_JITTER - 1e-9).all()
        else:                                             # opposing lanes closer than the keep-out distance would like: both swerve
            assert (np.abs(-dx - scenario.CA_ENC_HEAD_ON_LATERAL) <= 2 * scenario.CA_ENC_LANE_JITTER + 1e-12).all()
            assert (pose[1::2, 1] > pose[0::2, 1] + 6.0).all()


def test_python_front_end_bookkeeping():
    """set_fleet / set_world / world / fleet_state pass the right shapes to the C ABI (a recording stand-in for the library)"""
    calls = []

    class Lib:
        def __getattr__(self, name):
            def f(*a):
                calls.append((name, a))
                return 0
            return f
    fe = GuidanceFrontEnd.__new__(GuidanceFrontEnd)
    fe.s = types.SimpleNamespace(_h=None, _check=lambda rc: None, set_option=lambda *a: None)
    fe.B, fe._lib = 6, Lib()
    fe.set_world(np.zeros((5, 3)))
    assert calls[-1][0] == "usvmpc_guidance_world_vel" and calls[-1][1][1] is None          # no fleet: a world at rest, as ever
    fe.set_fleet(3, radius=0.4)
    assert calls[-1][0] == "usvmpc_guidance_fleet" and calls[-1][1][1:] == (3, 0.4)
    w, v = fe.world()
    assert w.shape == (6, 7, 3) and v.shape == (6, 7, 2)                       # the full list: 5 fixed + 2 fleet entries
    fe.set_world(np.zeros((4, 3)), predict=False)                               # the fixed entries; velocities given (zero), never NULL
    assert calls[-2][0] == "usvmpc_guidance_world" and calls[-2][1][2] == 4
    assert calls[-1][0] == "usvmpc_guidance_world_vel" and calls[-1][1][1] is not None and calls[-1][1][2] == 0
    assert fe.world()[0].shape == (6, 6, 3)
    with pytest.raises(Exception, match="at most 62"):
        fe.set_world(np.zeros((63, 3)))
    st = fe.fleet_state()
    assert st["min_separation"].shape == (6,) and st["separation_tick"].dtype == np.int32
    fe.set_fleet(0)
    assert fe.world()[0].shape == (6, 4, 3)
    assert "usvmpc_guidance_fleet" in _capi.EXPORTS and "usvmpc_guidance_fleet_state" in _capi.EXPORTS
