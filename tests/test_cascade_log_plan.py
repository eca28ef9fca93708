"""csrc/cascade_log_plan.hpp - the cascade log's descriptor check, byte layout, schedule (CasLogPlan::on_tick), read descriptors and status
word - compiled with the host compiler (CPU only) and driven from a command line (tests/cascade_log_plan_harness.cpp).

Every expected value is worked out by hand from the rule in include/usvmpc.h ("Cascade log"): low-level tick i (from 0 at the start of the
log) makes a record when i >= first, (i - first) % every == 0 and fewer than `capacity` records exist; when it is due and the buffer is full
it is missed.  The layout is [capacity][B][nsel] doubles, three times [capacity][B][2] (thrust and ref doubles, err float32) and
[capacity][B] int32."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cascade_log_plan_harness.cpp")

ALL6 = (1 << 6) - 1
B = 67


def build(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp(name) / "cascade_log_plan_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, "-o", exe, SRC])
    return exe


# every case runs on the plain build and on one with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory, "cascade_log_plan")
    return build(tmp_path_factory, "cascade_log_plan_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, tokens):
    """One dict per printed line; `err` is the text to the end of the line.  A sanitizer report ends the program with a message on stderr
    and a non-zero code."""
    r = subprocess.run([exe] + tokens, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        head, _, err = line.partition(" err=")
        w = head.split()
        d = {"kind": w[0], "err": err}
        d.update((k, int(v)) for k, v in (kv.split("=", 1) for kv in w[1:]))
        out.append(d)
    return out


def desc(capacity=5, every=1, first=0, mask=ALL6, thrust=1, ref=1, err=1, status=1):
    return "desc:%d:%d:%d:%d:%d:%d:%d:%d" % (capacity, every, first, mask, thrust, ref, err, status)


# (first, every, capacity) -> the ticks 0 .. 11 that get slots 0, 1, ..; those that are missed
SCHEDULES = [
    ((0, 1, 5), [0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10, 11]),
    ((2, 3, 8), [2, 5, 8, 11], []),                    # not aligned with a ratio of 5
    ((0, 5, 8), [0, 5, 10], []),                       # the guidance ticks of a ratio of 5
    ((1, 2, 5), [1, 3, 5, 7, 9], [11]),
    ((3, 7, 1), [3], [10]),
    ((2, 3, 2), [2, 5], [8, 11]),
]


@pytest.mark.parametrize("sched,recorded,missed", SCHEDULES)
def test_schedule(harness, sched, recorded, missed):
    first, every, capacity = sched
    out = run(harness, [desc(capacity, every, first), "start", "tick:12", "info"])
    assert out[0]["kind"] == "start" and out[0]["rc"] == 0
    ticks = out[1:13]
    assert [t["i"] for t in ticks] == list(range(12))
    assert [t["i"] for t in ticks if t["slot"] >= 0] == recorded
    assert [t["slot"] for t in ticks if t["slot"] >= 0] == list(range(len(recorded)))
    assert [t["i"] for t in ticks if t["missed"]] == missed
    assert all(not (t["missed"] and t["slot"] >= 0) for t in ticks)
    info = out[13]
    assert (info["on"], info["records"], info["ticks"], info["missed"]) == (1, len(recorded), 12, len(missed))


@pytest.mark.parametrize("only", ["mask", "thrust", "ref", "err", "status"])
def test_the_schedule_runs_whichever_channel_is_on(harness, only):
    kw = dict(mask=0, thrust=0, ref=0, err=0, status=0)
    kw[only] = 0b100 if only == "mask" else 1
    out = run(harness, [desc(3, 2, 1, **kw), "start", "tick:8", "info"])
    assert out[0]["rc"] == 0
    assert [t["slot"] for t in out[1:9]] == [-1, 0, -1, 1, -1, 2, -1, -1]
    assert [t["missed"] for t in out[1:9]] == [0, 0, 0, 0, 0, 0, 0, 1]
    assert (out[9]["records"], out[9]["ticks"], out[9]["missed"]) == (3, 8, 1)


def test_a_log_that_is_full_stays_full(harness):
    out = run(harness, [desc(2, 1, 0), "start", "tick:2", "read:state:0:2:0:67", "tick:40", "info", "read:state:0:2:0:67", "read:state:0:3:0:67"])
    assert [t["slot"] for t in out[1:3]] == [0, 1]
    assert all(t["slot"] == -1 and t["missed"] == 1 for t in out[4:44])          # no ring: never a slot again
    assert (out[44]["records"], out[44]["ticks"], out[44]["missed"]) == (2, 42, 40)
    assert out[3] == out[45] and out[3]["rc"] == 0                               # the same two records, where they were
    assert out[46]["err"] == "log: records outside those made so far"


def test_a_plan_that_was_not_started_or_was_stopped_does_nothing(harness):
    out = run(harness, ["tick:2", "info", "read:state:0:1:0:1"])
    assert [(t["slot"], t["missed"]) for t in out[:2]] == [(-1, 0)] * 2
    assert (out[2]["on"], out[2]["records"], out[2]["ticks"]) == (0, 0, 0)
    assert out[3]["rc"] == -1 and out[3]["err"] == "log: no log is running (usvmpc_cascade_log_start)"
    out = run(harness, [desc(), "start", "tick:2", "stop", "tick:2", "info", "read:thrust:0:1:0:1", "start", "info"])
    assert [t["slot"] for t in out[1:5]] == [0, 1, -1, -1]
    assert (out[5]["on"], out[5]["ticks"]) == (0, 2)
    assert out[6]["err"] == "log: no log is running (usvmpc_cascade_log_start)"
    assert out[7]["rc"] == 0 and (out[8]["on"], out[8]["records"], out[8]["ticks"], out[8]["missed"]) == (1, 0, 0, 0)   # a second log starts from 0


REFUSALS = [
    ([desc(capacity=0)], "log: capacity must be at least 1"),
    ([desc(capacity=-3)], "log: capacity must be at least 1"),
    ([desc(every=0)], "log: every must be at least 1"),
    ([desc(first=-1)], "log: first must not be negative"),
    ([desc(mask=1 << 6)], "log: state_mask names a state the vessel does not have"),
    ([desc(mask=ALL6 | 1 << 31)], "log: state_mask names a state the vessel does not have"),
    ([desc(mask=0, thrust=0, ref=0, err=0, status=0)], "log: the descriptor records nothing"),
    (["batch:0", desc()], "log: a batch of at least 1 is needed"),
    (["batch:2147483647", desc(capacity=2147483647)], "log: the log's size overflows"),
]


@pytest.mark.parametrize("tokens,text", REFUSALS)
def test_refusals(harness, tokens, text):
    out = run(harness, tokens + ["check"])
    assert out[-1]["rc"] == -1 and out[-1]["err"] == text, out


def test_sizes_at_the_edge_of_64_bits(harness):
    big = 2147483647
    # capacity * B * nsel * 8 alone: 2^31 * 2^28 * 8 fits for one state ...
    out = run(harness, ["batch:268435456", desc(capacity=big, mask=1, thrust=0, ref=0, err=0, status=0), "check"])[-1]
    assert out["rc"] == 0 and out["state"] == big * 268435456 * 8 == out["total"] < 2 ** 63
    # ... and no longer for three: the product overflows
    out = run(harness, ["batch:268435456", desc(capacity=big, mask=7, thrust=0, ref=0, err=0, status=0), "check"])[-1]
    assert out["rc"] == -1 and out["err"] == "log: the log's size overflows"
    # every channel fits on its own, their sum does not: 2 * (2^31 - 1) * 2^28 * 8 < 2^63 for thrust and for ref, together not
    out = run(harness, ["batch:268435456", desc(capacity=big, mask=0, thrust=1, ref=0, err=0, status=0), "check"])[-1]
    assert out["rc"] == 0 and out["thrust"] == big * 268435456 * 16 < 2 ** 63
    out = run(harness, ["batch:268435456", desc(capacity=big, mask=0, thrust=1, ref=1, err=0, status=0), "check"])[-1]
    assert out["rc"] == -1 and out["err"] == "log: the log's size overflows"
    # the float32 and int32 channels count 4-byte values
    out = run(harness, ["batch:268435456", desc(capacity=big, mask=0, thrust=0, ref=0, err=1, status=1), "check"])[-1]
    assert out["rc"] == 0 and (out["errs"], out["status"]) == (big * 268435456 * 8, big * 268435456 * 4)


def test_layout_and_read_descriptors(harness):
    cap = 5
    reads = ["read:state:0:5:0:67", "read:thrust:0:5:64:1", "read:ref:1:2:64:3", "read:err:2:1:0:67", "read:err:1:3:66:1",
             "read:status:2:1:0:67", "read:status:3:2:1:64", "read:state:4:1:66:1"]
    bad = ["read:state:4:2:0:67", "read:state:-1:1:0:67", "read:state:5:1:0:67", "read:state:0:0:0:67", "read:state:0:6:0:67",
           "read:err:0:1:66:2", "read:status:0:1:-1:1", "read:ref:0:1:67:1", "read:thrust:0:1:0:0", "read:x:0:1:0:1", "read"]
    out = run(harness, [desc(cap), "start", "read:state:0:1:0:1", "tick:5"] + reads + bad)
    lay = out[0]
    assert (lay["nsel"], lay["state"], lay["thrust"], lay["ref"], lay["errs"], lay["status"]) == (6, 16080, 5360, 5360, 2680, 1340)
    assert (lay["state"], lay["thrust"], lay["errs"], lay["status"]) == (cap * B * 6 * 8, cap * B * 2 * 8, cap * B * 2 * 4, cap * B * 4)
    assert lay["total"] == 16080 + 5360 + 5360 + 2680 + 1340
    assert out[1]["rc"] == -1 and out[1]["err"] == "log: records outside those made so far"    # nothing recorded yet
    r = out[7:15]
    key = lambda d: (d["rc"], d["channel"], d["n"], d["elem"], d["offset"], d["pitch"], d["width"], d["rows"], d["bytes"])
    assert key(r[0]) == (0, 0, 6, 8, 0, 3216, 3216, 5, 16080)           # the whole channel: one contiguous block
    assert key(r[1]) == (0, 1, 2, 8, 1024, 1072, 16, 5, 80)             # one instance: 5 runs of one cell
    assert key(r[2]) == (0, 2, 2, 8, 1072 + 1024, 1072, 48, 2, 96)
    assert key(r[3]) == (0, 3, 2, 4, 1072, 536, 536, 1, 536)            # float32 pairs: a record is 67 * 8 bytes
    assert key(r[4]) == (0, 3, 2, 4, 536 + 528, 536, 8, 3, 24)
    assert key(r[5]) == (0, 4, 1, 4, 536, 268, 268, 1, 268)             # int32: a record is 67 * 4 bytes
    assert key(r[6]) == (0, 4, 1, 4, 3 * 268 + 4, 268, 256, 2, 512)
    assert key(r[7]) == (0, 0, 6, 8, 16032, 3216, 48, 1, 48)            # the last instance of the last record ends at the channel's end
    assert r[7]["offset"] + r[7]["width"] == lay["state"]
    assert r[4]["offset"] + 2 * r[4]["pitch"] + r[4]["width"] <= lay["errs"]
    assert r[6]["offset"] + r[6]["pitch"] + r[6]["width"] <= lay["status"]
    assert [d["err"] for d in out[15:20]] == ["log: records outside those made so far"] * 5
    assert [d["err"] for d in out[20:24]] == ["log: instances outside the batch"] * 4
    assert out[24]["err"] == out[25]["err"] == 'log: the channels are "state", "thrust", "ref", "err" and "status"'
    # a strict subset of the states; the other channels off
    out = run(harness, ["batch:257", desc(3, mask=0b100101, thrust=0, ref=0, err=0, status=0), "start", "tick:1",
                        "read:state:0:1:256:1", "read:thrust:0:1:0:1", "read:ref:0:1:0:1", "read:err:0:1:0:1", "read:status:0:1:0:1"])
    assert (out[0]["nsel"], out[0]["state"], out[0]["total"]) == (3, 3 * 257 * 3 * 8, 3 * 257 * 3 * 8)
    assert (out[2]["n"], out[2]["offset"], out[2]["width"], out[2]["rows"]) == (3, 256 * 24, 24, 1)
    assert [d["err"] for d in out[3:7]] == ["log: this channel is not recorded"] * 4
    # ... and the state channel off
    out = run(harness, [desc(3, mask=0, thrust=0, ref=0, err=1, status=0), "start", "tick:1", "read:state:0:1:0:1", "read:err:0:1:0:67"])
    assert out[2]["err"] == "log: this channel is not recorded" and (out[3]["rc"], out[3]["bytes"]) == (0, 536)


WORDS = [
    ((0, 0, 0, 0), 0),
    ((4, 0, 0, 0), 4),
    ((0, 7, 0, 0), 7 << 8),
    ((0, 0, 3, 0), 3 << 16),
    ((0, 0, 0, 9), 9 << 24),
    ((2, 50, 4, 127), 2 | 50 << 8 | 4 << 16 | 127 << 24),
    ((255, 255, 255, 127), 0x7fffffff),
    # a field wider than its bits is cut, never spilt into its neighbour; bit 31 stays clear
    ((256 + 1, 0, 0, 0), 1),
    ((0, 256 + 2, 0, 0), 2 << 8),
    ((0, 0, 256 + 3, 0), 3 << 16),
    ((0, 0, 0, 128 + 5), 5 << 24),
    ((-1, 0, 0, 0), 255),
    ((0, 0, 0, -1), 127 << 24),
]


@pytest.mark.parametrize("fields,value", WORDS)
def test_status_word(harness, fields, value):
    out = run(harness, ["word:%d:%d:%d:%d" % fields])
    assert out[0]["value"] == value
    ll_status, ll_qp_iter, g_status, g_qp_iter = (f for f in fields)
    w = out[0]["value"]
    assert (w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xff, (w >> 24) & 0x7f) == (ll_status & 0xff, ll_qp_iter & 0xff, g_status & 0xff, g_qp_iter & 0x7f)
