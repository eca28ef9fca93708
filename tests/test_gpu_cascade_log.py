"""The cascade's log and the realised cost of its two layers on a real MI355X (`pytest -m gpu`): kernel usv_cascade_record through
usvmpc_cascade_log_* and guidance.Cascade.start_log / read_log / log_info / stop_log; usvmpc_cost_track_now through
BatchOcpSolver.track_cost_now and Cascade.track_cost / tracked_cost (include/usvmpc.h, "Cascade log" and "Objective value").

The yardstick is always a TWIN stack without a log or tracking, driven by the manual loop of tests/test_gpu_cascade.py's `trace` fixture;
at every tick the host reads back what the log should hold - cas.state()["state"] before the step, ["thrust"] after it, the fetched
publish() pair, scenario.cascade_ll_outputs' (e_u, e_psi), get_int("status") / get_int("qp_iter") of both solvers - and, for the cost, x0, u,
yref, sl, su of stage 0 behind either solve.  Every comparison is bit for bit (uint64 / uint32 views).  Shapes: those of
tests/test_gpu_cascade.py - guidance N = 40 / K = 8, low level N = 20 at T = 0.01, ratio 5."""
import ctypes as C

import numpy as np
import pytest

from mpc_collisionavoidance_amd import _capi, scenario, usv_models
from tests import cost_numpy as cn
from tests.test_gpu_cascade import BT, FROZEN, GDT, GN, K, LL, LN, M1, NT, RATIO, T, _close_all, _stack

pytestmark = pytest.mark.gpu

E_ARG = -1
CHANNELS = ("state", "thrust", "ref", "err")
WORDS = ("ll_status", "ll_qp_iter", "g_status", "g_qp_iter")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _missions(B, frozen):
    m = scenario.make_ca_missions(B, 6, seed=0)
    wps = None
    if frozen:      # (the `trace` fixture's instance 66: its mission is over at the second guidance tick, its set-points go to (0, 0))
        wps = np.tile(m["waypoints"][None], (B, 1, 1))
        wps[FROZEN] = [[4.0, -8.0], [4.0, -5.5], [4.0, -5.6]]
        m["pose"][FROZEN, 0] = 4.2
    return m, wps


def _final(g, ll, cas):
    st = cas.state()
    return dict(state=st["state"], thrust=st["thrust"], past=st["past_thrust"], sums=st["err_sums"], gx=g.get_all("x"), gu=g.get_all("u"),
                lx=ll.get_all("x"), lu=ll.get_all("u"), gx0=g.get("x0", 0))


def _twin(B, nt, frozen=False, sigma=0.0, seed0=100):
    """The yardstick: a stack without a log or tracking, the manual loop, everything read back by the host.  dict of per-tick arrays
    [nt][B][..] (the log is compared tick-major) plus `final` and the sequential numpy sums of the stage-0 cost of either layer."""
    m, wps = _missions(B, frozen)
    g, fe, ll, cas = _stack(m, B, wps=wps)
    tab_g = cn.tab_of_ocp(usv_models.make_ocp(M1, GN * GDT, GN, K), K, True)      # soft rows for the guidance layer
    tab_l = cn.tab_of_ocp(usv_models.make_ocp(LL, LN * T, LN), 0, False)          # none for the low level
    rec = {k: [] for k in CHANNELS + WORDS}
    cost_g, cost_l, n_g, n_l = np.zeros(B), np.zeros(B), 0, 0
    none = np.zeros((B, 0))
    pub = None
    for t in range(nt):
        if cas.guidance_tick():
            fe.prepare(); g.solve_async()
            c0, _, _ = cn.stage(tab_g, g.dt, g.get("u", 0), g.get("x0", 0), g.get("yref", 0), g.get("sl", 0), g.get("su", 0))
            cost_g, n_g = cost_g + c0, n_g + 1
            pub = fe.publish()
        cas.refs()
        ll.solve_async()
        c0, _, _ = cn.stage(tab_l, ll.dt, ll.get("u", 0), ll.get("x0", 0), ll.get("yref", 0), none, none)
        cost_l, n_l = cost_l + c0, n_l + 1
        s0 = cas.state()["state"]
        _, _, eu, epsi = scenario.cascade_ll_outputs(ll.get("x", 1), pub["heading"], pub["speed"], s0)
        rec["state"].append(s0)
        rec["ref"].append(np.column_stack([pub["heading"], pub["speed"]]))
        rec["err"].append(np.column_stack([eu, epsi]))
        for name, s, f in (("ll_status", ll, "status"), ("ll_qp_iter", ll, "qp_iter"), ("g_status", g, "status"), ("g_qp_iter", g, "qp_iter")):
            rec[name].append(s.get_int(f).astype(np.int32))
        cas.step(sigma, seed0 + t)
        rec["thrust"].append(cas.state()["thrust"])
    out = {k: np.array(v) for k, v in rec.items()}
    assert out["err"].dtype == np.float32 and out["state"].shape == (nt, B, 6)
    out["final"] = _final(g, ll, cas)
    out["cost"] = dict(guidance=(cost_g, n_g), low_level=(cost_l, n_l))
    _close_all(cas, ll, g)
    return out


@pytest.fixture(scope="module")
def twin():
    """12 ticks over B = 67 with the frozen instance 66: the yardstick of tests 1, 2, 3, 5 (computed once, never changed)"""
    return _twin(BT, NT, frozen=True)


def _logged(B, nt, frozen=False, sigma=0.0, seed0=100, sl=slice(None), offset=0, track=False, **log):
    """A stack of its own driven by tick() with a log (and tracking): (read_log(), log_info(), final, tracked cost, device-byte figures)"""
    m, wps = _missions(B, frozen)
    n = len(range(*sl.indices(B)))
    g, fe, ll, cas = _stack(m, n, wps=wps, offset=offset, sl=sl)
    bytes0 = g.device_bytes()
    if log:
        cas.start_log(**log)
    bytes1 = g.device_bytes()
    if track:
        cas.track_cost()
    for t in range(nt):
        cas.tick(sigma, seed0 + t)
    out = dict(log=cas.read_log() if log else None, info=cas.log_info() if log else None, final=_final(g, ll, cas),
               cost=cas.tracked_cost() if track else None, bytes=(bytes0, bytes1))
    return out, (g, fe, ll, cas)


def _close(objs):
    g, fe, ll, cas = objs
    _close_all(cas, ll, g)


def _same_final(a, b):
    return all(same(a[k], b[k]) for k in a)


def _check_against(twin, lg, ticks, states=range(6), what=CHANNELS + WORDS):
    """the log's records are the twin's read-backs of `ticks`, bit for bit; instance-major against tick-major"""
    ticks, states = list(ticks), list(states)
    assert list(lg["tick"]) == ticks
    for name in what:
        want = twin[name][ticks]
        if name == "state":
            want = want[:, :, states]
            assert lg["states"] == states
        got = lg[name]
        assert same(np.swapaxes(got, 0, 1), want), name


# ------------------------------------------------------------------ 1. every channel, bit for bit
def test_every_channel_bit_for_bit(twin):
    r, objs = _logged(BT, NT, frozen=True, capacity=NT, err=True)
    lg, info = r["log"], r["info"]
    assert info == dict(records=NT, ticks=NT, missed=0, nsel=6)
    assert lg["state"].shape == (BT, NT, 6) and lg["thrust"].shape == lg["ref"].shape == lg["err"].shape == (BT, NT, 2)
    assert lg["err"].dtype == np.float32 and lg["ll_status"].shape == (BT, NT)
    _check_against(twin, lg, range(NT))
    # the frozen instance: its set-points go to (0, 0) at the second guidance tick - the thrust record is zero from there on although the
    # low-level iterate (and the past thrust with it) keeps moving
    assert (lg["ref"][FROZEN, RATIO:] == 0.0).all() and (lg["thrust"][FROZEN, RATIO:] == 0.0).all()
    assert np.abs(lg["thrust"][FROZEN, :RATIO]).max() > 0.0 and np.abs(r["final"]["past"][FROZEN]).max() > 0.0
    assert np.abs(lg["thrust"][:FROZEN, -1]).max() > 0.1
    assert (lg["ll_status"] == 0).all() and lg["ll_qp_iter"].max() > 0 and lg["g_qp_iter"].max() > 0     # (no field of the word is idle)
    # logging changes no result
    assert _same_final(r["final"], twin["final"])
    _close(objs)


# ------------------------------------------------------------------ 2. the schedule on the device
@pytest.mark.parametrize("every,first,capacity,ticks,missed", [
    (3, 2, 8, [2, 5, 8, 11], 0),          # not aligned with the ratio
    (5, 0, 8, [0, 5, 10], 0),             # the guidance ticks only: g_status is fresh in every record
    (2, 1, 3, [1, 3, 5], 3),              # fewer slots than due ticks (1, 3, 5, 7, 9, 11): the first three stay, three are missed
])
def test_schedule_on_the_device(twin, every, first, capacity, ticks, missed):
    m, wps = _missions(BT, True)
    g, fe, ll, cas = _stack(m, BT, wps=wps)
    cas.start_log(capacity, every=every, first=first, err=True)
    early = None
    for t in range(NT):
        cas.tick()
        if t == ticks[-1]:
            early = cas.read_log()          # (as soon as the last record exists)
            assert cas.log_info()["records"] == len(ticks) and cas.log_info()["missed"] == 0
    lg, info = cas.read_log(), cas.log_info()
    assert info == dict(records=len(ticks), ticks=NT, missed=missed, nsel=6)
    _check_against(twin, lg, ticks)
    for name in CHANNELS + WORDS:         # the records made are unchanged by the ticks that came after, missed ones included
        assert same(lg[name], early[name]), name
    assert _same_final(_final(g, ll, cas), twin["final"])
    _close_all(cas, ll, g)


# ------------------------------------------------------------------ 3. selection and windows
NT3 = 7     # (two guidance ticks: the frozen instance's set-points change at tick 5)


@pytest.mark.parametrize("kw,what", [
    (dict(states=(0, 2, 5), thrust=False, ref=False, err=False, status=False), ("state",)),      # a strict subset: (nedx, psi, r)
    (dict(states=(), thrust=True, ref=False, err=False, status=False), ("thrust",)),
    (dict(states=(), thrust=False, ref=True, err=False, status=False), ("ref",)),
    (dict(states=(), thrust=False, ref=False, err=True, status=False), ("err",)),
    (dict(states=(), thrust=False, ref=False, err=False, status=True), WORDS),
])
def test_one_channel_at_a_time(twin, kw, what):
    r, objs = _logged(BT, NT3, frozen=True, capacity=NT3, **kw)
    lg = r["log"]
    assert set(lg) == set(what) | {"tick", "states"}
    _check_against(twin, lg, range(NT3), states=kw["states"], what=what)
    g, fe, ll, cas = objs
    width = dict(state=8 * len(kw["states"]), thrust=16, ref=16, err=8, ll_status=4)[what[0]]
    assert r["bytes"][1] - r["bytes"][0] == NT3 * BT * width
    for name in ("state", "thrust", "ref", "err", "status"):
        on = name in what or (name == "status" and what is WORDS)
        rc = cas._lib.usvmpc_cascade_log_read(cas._c, name.encode(), 0, 1, 0, 1, None, 0)
        msg = cas._lib.usvmpc_cascade_last_error(cas._c).decode()
        assert rc == E_ARG and ("out must hold exactly" in msg if on else msg == "log: this channel is not recorded"), (name, msg)
        assert bool(on) == (cas._lib.usvmpc_cascade_log_device_ptr(cas._c, name.encode(), C.byref(C.c_void_p())) == 0)
    _close_all(cas, ll, g)


def test_windows(twin):
    r, (g, fe, ll, cas) = _logged(BT, NT, frozen=True, capacity=NT, states=(1, 3, 4), err=True)
    full = r["log"]
    _check_against(twin, full, range(NT), states=(1, 3, 4))
    for recs, inst in (((3, 9), (60, 67)), (range(11, 12), range(0, 1)), ((0, NT), (64, 66)), (None, (66, 67)), ((5, 6), None)):
        w = cas.read_log(records=recs, instances=inst)
        r0, r1 = (0, NT) if recs is None else (recs[0], recs[-1] + 1) if isinstance(recs, range) else recs
        b0, b1 = (0, BT) if inst is None else (inst[0], inst[-1] + 1) if isinstance(inst, range) else inst
        assert list(w["tick"]) == list(range(r0, r1)) and w["states"] == [1, 3, 4]
        for name in CHANNELS + WORDS:
            assert same(w[name], full[name][b0:b1, r0:r1]), (name, recs, inst)
            assert w[name].shape[:2] == (b1 - b0, r1 - r0)
    _close_all(cas, ll, g)


# ------------------------------------------------------------------ 4. disturbance and shards
def test_disturbance_and_shards():
    B, H, NTK, SIG = 64, 32, 10, 1e-3
    kw = dict(sigma=SIG, capacity=NTK, err=True)
    whole, objs = _logged(B, NTK, **kw)
    _close(objs)
    halves = []
    for sl, off in ((slice(0, H), 0), (slice(H, B), H)):
        r, objs = _logged(B, NTK, sl=sl, offset=off, **kw)
        _close(objs)
        halves.append(r)
    for name in CHANNELS + WORDS:
        assert same(np.concatenate([halves[0]["log"][name], halves[1]["log"][name]]), whole["log"][name]), name
    # ... and the whole batch's log is what a twin's host read, tick by tick, under the same draws
    tw = _twin(B, NTK, sigma=SIG)
    _check_against(tw, whole["log"], range(NTK))
    assert _same_final(whole["final"], tw["final"])
    # the draws are in the log: (u, v, r) of record 1 are off the undisturbed plant period from record 0 under record 0's thrusts
    lg = whole["log"]
    d = lg["state"][:, 1, 3:] - scenario.cascade_plant_step(lg["state"][:, 0], lg["thrust"][:, 0], T, 1, 0.78)[:, 3:]
    assert (np.abs(d) > 1e-9).all() and np.abs(d).max() < 6 * SIG


# ------------------------------------------------------------------ 5. the tracked cost of both layers
def test_tracked_cost(twin):
    m, wps = _missions(BT, True)
    g, fe, ll, cas = _stack(m, BT, wps=wps)
    for s in (g, ll):
        with pytest.raises(Exception, match="cost_track_now: no tracking is running"):
            s.track_cost_now()
    assert g._lib.usvmpc_cost_track_now(None) == E_ARG
    cas.track_cost()
    for t in range(NT):
        cas.tick()
    got = cas.tracked_cost()
    for layer, count in (("guidance", 3), ("low_level", NT)):
        want, n = twin["cost"][layer]
        assert n == count and got[layer][1] == count
        assert cn.same_bits(got[layer][0], want), (layer, np.abs(got[layer][0] - want).max())
        assert np.isfinite(want).all() and (want != 0.0).any()
    assert _same_final(_final(g, ll, cas), twin["final"])       # tracking changes no result
    cas.track_cost(False)
    for s in (g, ll):
        with pytest.raises(Exception, match="no tracking is running"):
            s.track_cost_now()
    cas.tick()                                                  # ... and a tick without tracking runs as before
    with pytest.raises(Exception, match="no tracking is running"):
        cas.tracked_cost()
    _close_all(cas, ll, g)


# ------------------------------------------------------------------ 6. refusals and lifetime
def test_refusals_and_lifetime():
    B = 8
    m, _ = _missions(B, False)
    g, fe, ll, cas = _stack(m, B)
    lib, c = cas._lib, cas._c
    st, qi = (C.c_void_p(ll.device_ptr(f)) for f in ("status", "qp_iter"))
    err = lambda: lib.usvmpc_cascade_last_error(c).decode()

    def desc(capacity=4, every=1, first=0, mask=63, thrust=1, ref=1, e=1, status=1):
        d = _capi.CascadeLogDesc()
        d.capacity, d.every, d.first, d.state_mask = capacity, every, first, mask
        d.record_thrust, d.record_ref, d.record_err, d.record_status = thrust, ref, e, status
        return d

    def refused(text, d, a=st, b=qi):
        before = g.device_bytes()
        rc = lib.usvmpc_cascade_log_start(c, C.byref(d) if d is not None else None, a, b)
        assert rc == E_ARG and text in err(), (rc, err())
        assert g.device_bytes() == before

    cas.tick()                                          # (whatever the solvers allocate at their first solve is there)
    bytes0 = g.device_bytes()
    # no log yet
    for call in (lambda: lib.usvmpc_cascade_log_stop(c), lambda: lib.usvmpc_cascade_log_info(c, None, None, None, None),
                 lambda: lib.usvmpc_cascade_log_read(c, b"state", 0, 1, 0, 1, None, 0),
                 lambda: lib.usvmpc_cascade_log_device_ptr(c, b"state", C.byref(C.c_void_p()))):
        assert call() == E_ARG and "no log is running" in err(), err()
    with pytest.raises(Exception, match="no log is running"):
        cas.read_log()
    # descriptors
    refused("null descriptor", None)
    refused("log: capacity must be at least 1", desc(capacity=0))
    refused("log: every must be at least 1", desc(every=0))
    refused("log: first must not be negative", desc(first=-1))
    refused("log: state_mask names a state the vessel does not have", desc(mask=1 << 6))
    refused("log: the descriptor records nothing", desc(mask=0, thrust=0, ref=0, e=0, status=0))
    refused("status channel needs the low-level solver's device pointers", desc(), a=None)
    refused("status channel needs the low-level solver's device pointers", desc(), b=None)
    assert lib.usvmpc_cascade_log_start(None, C.byref(desc()), st, qi) == E_ARG
    # the status channel off: the pointers are not needed
    assert lib.usvmpc_cascade_log_start(c, C.byref(desc(status=0)), None, None) == 0
    assert g.device_bytes() == bytes0 + 4 * B * (48 + 16 + 16 + 8)
    assert lib.usvmpc_cascade_log_stop(c) == 0 and g.device_bytes() == bytes0
    # a running log
    cas.start_log(4, err=True)
    assert g.device_bytes() == bytes0 + 4 * B * (48 + 16 + 16 + 8 + 4)
    refused("a log is running (usvmpc_cascade_log_stop first)", desc())
    with pytest.raises(Exception, match="cascade_reset: a log is running"):
        cas.reset(m["pose"], np.column_stack([m["vel"], np.zeros(B)]))
    assert cas.log_info() == dict(records=0, ticks=0, missed=0, nsel=6)
    buf = np.zeros((2, B, 6))
    read = lambda ch, r0, nr, b0, nb, a, n: lib.usvmpc_cascade_log_read(c, ch, r0, nr, b0, nb, a.ctypes.data_as(C.c_void_p), n)
    assert read(b"state", 0, 1, 0, B, buf, B * 48) == E_ARG and err() == "log: records outside those made so far"
    cas.tick(); cas.tick()
    assert read(b"state", 0, 2, 0, B, buf, buf.nbytes) == 0
    assert np.isfinite(buf).all() and not same(buf[0], buf[1])
    for r0, nr in ((0, 3), (2, 1), (-1, 1), (0, 0), (1, 2)):
        assert read(b"state", r0, nr, 0, B, buf, buf.nbytes) == E_ARG and err() == "log: records outside those made so far", (r0, nr)
    for b0, nb in ((0, B + 1), (B, 1), (-1, 1), (0, 0), (B - 1, 2)):
        assert read(b"state", 0, 2, b0, nb, buf, buf.nbytes) == E_ARG and err() == "log: instances outside the batch", (b0, nb)
    assert read(b"x", 0, 2, 0, B, buf, buf.nbytes) == E_ARG and "the channels are" in err()
    for n in (buf.nbytes - 8, buf.nbytes + 8, 0):
        assert read(b"state", 0, 2, 0, B, buf, n) == E_ARG and "out must hold exactly %d bytes" % buf.nbytes in err()
    assert lib.usvmpc_cascade_log_read(c, b"state", 0, 2, 0, B, None, buf.nbytes) == E_ARG and "out must hold exactly" in err()
    assert read(b"err", 0, 2, 0, B, buf, 2 * B * 8) == 0 and read(b"status", 0, 2, 0, B, buf, 2 * B * 4) == 0      # float32 pairs, int32
    assert read(b"err", 0, 2, 0, B, buf, 2 * B * 16) == E_ARG
    assert lib.usvmpc_cascade_log_device_ptr(c, b"q", C.byref(C.c_void_p())) == E_ARG and "is no channel of the running log" in err()
    p = C.c_void_p()
    assert lib.usvmpc_cascade_log_device_ptr(c, b"thrust", C.byref(p)) == 0 and p.value == cas.log_device_ptr("thrust") != 0
    first = cas.read_log()
    # stop, then start again: counted from 0, the earlier bytes are back
    before = g.device_bytes()
    cas.stop_log()
    assert g.device_bytes() == before - 4 * B * (48 + 16 + 16 + 8 + 4)
    with pytest.raises(Exception, match="no log is running"):
        cas.log_info()
    cas.tick()                                          # (a tick without a log in between)
    before = g.device_bytes()
    cas.start_log(2, every=2, first=1, states=(0, 1), thrust=False, ref=False, status=False)
    assert g.device_bytes() == before + 2 * B * 16
    for t in range(4):
        cas.tick()
    lg = cas.read_log()
    assert cas.log_info() == dict(records=2, ticks=4, missed=0, nsel=2) and list(lg["tick"]) == [1, 3]
    assert lg["state"].shape == (B, 2, 2) and not same(lg["state"][:, 0], first["state"][:, 1, :2])
    # reset after the stop; close() stops a running log
    before = g.device_bytes()
    cas.stop_log()
    assert g.device_bytes() == before - 2 * B * 16
    cas.reset(m["pose"], np.column_stack([m["vel"], np.zeros(B)]))
    before = g.device_bytes()
    cas.start_log(3)
    cas.tick()
    assert cas.log_info()["records"] == 1 and g.device_bytes() == before + 3 * B * (48 + 16 + 16 + 4)
    cas.close()
    assert g.device_bytes() == before
    _close_all(ll, g)

