"""csrc/world_plan.hpp - the front ends' resident world list: what each call refuses (and in which order), what the carrier is told to do and
what the list is afterwards - compiled with the host compiler (CPU only) and driven from a command line (tests/world_plan_harness.cpp), for
both front ends.

Every expected value is written out by hand, from include/usvmpc.h and the entry points as they stood before the header: the refusals' words
and the scripted pass through the transitions are in tests/world_calls_ref.py, which tests/test_gpu_world_calls.py holds the library on the
device to as well; the rest is below.  Sizes are in doubles: a list of n entries for a batch of B needs B n 3, its velocities B n 2."""
import os
import subprocess

import pytest

from tests import world_calls_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "world_plan_harness.cpp")


def build(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp(name) / "world_plan_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, "-o", exe, SRC])
    return exe


# every case runs on the plain build and on one with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory, "world_plan")
    return build(tmp_path_factory, "world_plan_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, kind, tokens):
    """One dict per printed line; `err` is the text to the end of the line.  A sanitizer report ends the program with a message on stderr
    and a non-zero code."""
    r = subprocess.run([exe, "kind:" + kind[0]] + tokens, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        head, _, err = line.partition(" err=")
        w = head.split()
        d = {"line": w[0], "err": err}
        d.update((k, float(v) if "." in v or "e" in v else int(v)) for k, v in (kv.split("=", 1) for kv in w[1:]))
        out.append(d)
    return out


def calls(exe, kind, tokens):
    """[(call line, state line after it)] of the calls among `tokens`; a "state" token gives (None, state)"""
    out = run(exe, kind, tokens)
    pairs, i = [], 0
    while i < len(out):
        if out[i]["line"] == "state":
            pairs.append((None, out[i]))
            i += 1
        else:
            assert out[i + 1]["line"] == "state"
            pairs.append((out[i], out[i + 1]))
            i += 2
    return pairs


def token(step):
    c = step["call"]
    if c == "world":
        return "world:%d:%r" % (step["n"], step["radius"])
    if c == "vel":
        return "vel:%d" % step["predict"] if step["given"] else "vel:null:%d" % step["predict"]
    if c == "fleet":
        return "fleet:%d:%r" % (step["S"], step["radius"])
    if c == "step":
        return "step:%r" % step["T"]
    return c


@pytest.mark.parametrize("kind", R.KINDS)
def test_transitions(harness, kind):
    """the scripted pass of world_calls_ref.SCRIPT: every action descriptor and the state after every call"""
    got = calls(harness, kind, ["state"] + [token(s) for s in R.SCRIPT])
    before = got[0][1]
    for i, (step, (line, state)) in enumerate(zip(R.SCRIPT, got[1:])):
        what = "step %d, %s" % (i, token(step))
        if "err" in step:
            key, numbers = step["err"]
            assert line["rc"] == -1 and line["err"] == R.refusal(kind, step["call"], key, **numbers), what
            assert state == before, what                      # nothing changed
            continue
        assert line["rc"] == 0, (what, line["err"])
        for k, v in step["act"].items():
            assert line[k] == R.pick(v, kind), (what, k)
        for k, v in step["state"].items():
            assert state[k] == R.pick(v, kind), (what, k)
        assert state["steps"] == state["moving"], what        # (steps_on_advance, the option on)
        before = state


# ---- every refusal of every call: (set-up, the call, the call's name, the key of the message, its numbers).  A kind of None: both.
LIST2 = ["world:2:50"]
MOVING2 = LIST2 + ["vel:1"]
FLEET3 = LIST2 + ["fleet:3:0.5"]      # (2 fixed entries, 2 slots)
REFUSED = [
    # before a list
    (None, [], "vel:1", "vel", "no_list", {}),
    (None, [], "read", "read", "no_list", {}),
    (None, [], "fleet:3:0.5", "fleet", "fleet_no_list", {}),
    (None, [], "step:0.1", "step", "at_rest", {}),
    # the list
    (None, [], "world:-1:50", "world", "n_world", {}),
    (None, [], "world:65:50", "world", "n_world", {}),
    (None, [], "world:2:50:null", "world", "null_list", {}),
    (None, [], "world:64:50:null", "world", "null_list", {}),
    (None, [], "world:2:nan", "world", "radius_nan", {}),
    ("guidance", [], "world:2:50:nan=7", "world", "entry_nan", dict(i=7)),       # (path-following takes it: below)
    ("guidance", [], "world:3:50:nan=53", "world", "entry_nan", dict(i=53)),     # (the last of 6 * 3 * 3)
    (None, FLEET3, "world:63:50", "world", "fleet_owns", dict(slots=2, most=62)),
    (None, LIST2 + ["fleet:2:0.5"], "world:64:50", "world", "fleet_owns", dict(slots=1, most=63)),
    # the velocities: the message names the first offending index
    (None, LIST2, "vel:1:inf=5", "vel", "not_finite", dict(i=5)),
    (None, LIST2, "vel:1:nan=0", "vel", "not_finite", dict(i=0)),
    (None, LIST2, "vel:1:nan=23", "vel", "not_finite", dict(i=23)),              # (the last of 6 * 2 * 2)
    (None, FLEET3, "vel:1:inf=23", "vel", "not_finite", dict(i=23)),             # (a fleet on: [B][nfixed][2], 24 values)
    (None, ["tracks:1"] + LIST2, "vel:1", "vel", "tracks", {}),
    (None, FLEET3, "vel:null:1", "vel", "vel_null_fleet", {}),
    # the fleet
    (None, LIST2, "fleet:-1:0.5", "fleet", "scene_negative", {}),
    (None, ["tracks:1"] + LIST2, "fleet:3:0.5", "fleet", "tracks", {}),
    (None, ["B:8"] + LIST2, "fleet:3:0.5", "fleet", "scenes", dict(B=8, S=3)),
    (None, LIST2, "fleet:4:0.5", "fleet", "scenes", dict(B=6, S=4)),
    (None, ["world:63:50"], "fleet:3:0.5", "fleet", "fits", dict(n_fixed=63, slots=2)),
    (None, ["world:64:50"], "fleet:2:0.5", "fleet", "fits", dict(n_fixed=64, slots=1)),
    (None, ["world:62:50", "fleet:2:0.5"], "fleet:6:0.5", "fleet", "fits", dict(n_fixed=62, slots=5)),   # (a larger scene: the fixed entries count)
    (None, LIST2, "fleet:3:-0.1", "fleet", "radius", {}),
    (None, LIST2, "fleet:3:nan", "fleet", "radius", {}),
    (None, LIST2, "fleet:3:inf", "fleet", "radius", {}),
    # the step
    (None, LIST2, "step:0.1", "step", "at_rest", {}),
    (None, MOVING2 + ["vel:null:0"], "step:0.1", "step", "at_rest", {}),
    (None, MOVING2, "step:nan", "step", "T", {}),
    (None, MOVING2, "step:inf", "step", "T", {}),
    # which refusal wins.  world: the count before the null list before max_radius before a NaN entry before the fleet's share
    (None, [], "world:65:nan:null", "world", "n_world", {}),
    (None, [], "world:2:nan:null", "world", "null_list", {}),
    (None, [], "world:2:nan:nan=0", "world", "radius_nan", {}),
    ("guidance", FLEET3, "world:63:50:nan=1", "world", "entry_nan", dict(i=1)),
    ("pf", FLEET3, "world:63:50:nan=1", "world", "fleet_owns", dict(slots=2, most=62)),
    # world_vel: NULL with a fleet on before anything; no list before the tracks before finiteness
    (None, FLEET3 + ["tracks:1"], "vel:null:0", "vel", "vel_null_fleet", {}),
    (None, ["tracks:1"], "vel:1:inf=0", "vel", "no_list", {}),
    (None, ["tracks:1"] + LIST2, "vel:1:inf=0", "vel", "tracks", {}),
    # fleet: the list before the scene size before the tracks before whole scenes before the fit before the radius
    (None, ["tracks:1", "B:8"], "fleet:-1:nan", "fleet", "fleet_no_list", {}),
    (None, ["tracks:1", "B:8", "world:63:50"], "fleet:-1:nan", "fleet", "scene_negative", {}),
    (None, ["tracks:1", "B:8", "world:63:50"], "fleet:3:nan", "fleet", "tracks", {}),
    (None, ["B:8", "world:63:50"], "fleet:3:nan", "fleet", "scenes", dict(B=8, S=3)),
    (None, ["world:63:50"], "fleet:3:nan", "fleet", "fits", dict(n_fixed=63, slots=2)),
    (None, ["world:62:50"], "fleet:3:nan", "fleet", "radius", {}),
    # step: at rest before T
    (None, LIST2, "step:nan", "step", "at_rest", {}),
]
ALL_CALLS = [("world:2:50", "world"), ("vel:1", "vel"), ("vel:null:0", "vel"), ("step:0.1", "step"), ("read", "read"), ("fleet:3:0.5", "fleet"),
             ("fstate", "fstate")]


def refused(exe, kind, setup, tok, call, key, numbers):
    got = calls(exe, kind, setup + ["state", tok])
    (_, before), (line, after) = got[-2:]
    assert line["rc"] == -1 and line["err"] == R.refusal(kind, call, key, **numbers), (kind, setup, tok)
    assert after == before, (kind, setup, tok)            # a refused call changes nothing


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_refusal_and_their_order(harness, kind):
    for only, setup, tok, call, key, numbers in REFUSED:
        if only in (None, kind):
            refused(harness, kind, setup, tok, call, key, numbers)


@pytest.mark.parametrize("kind", R.KINDS)
def test_wrong_model_refuses_every_call_first(harness, kind):
    for tok, call in ALL_CALLS:
        refused(harness, kind, ["model:0", "ready:0"], tok, call, "wrong_model", {})
        refused(harness, kind, LIST2 + ["model:0"], tok, call, "wrong_model", {})


def test_guidance_needs_its_reset_for_every_call(harness):
    for tok, call in ALL_CALLS:
        refused(harness, "guidance", ["ready:0"], tok, call, "before_reset", {})


def test_path_following_world_calls_work_before_the_reset(harness):
    """only fleet (one refusal with the missing list) and fleet_state need usvmpc_pf_reset; the world calls work before it and ask for
    "static_obstacles" only once the front end is ready"""
    refused(harness, "pf", ["ready:0"], "fstate", "fstate", "before_reset", {})
    refused(harness, "pf", ["ready:0"], "fleet:3:0.5", "fleet", "fleet_no_list", {})
    refused(harness, "pf", ["ready:0"] + LIST2, "fleet:3:0.5", "fleet", "fleet_no_list", {})     # (a list, no reset)
    refused(harness, "pf", [], "fleet:3:0.5", "fleet", "fleet_no_list", {})                      # (the reset, no list)
    got = calls(harness, "pf", ["ready:0", "world:2:50", "vel:1", "step:0.5", "read", "world:3:50", "vel:null:0", "ready:1", "vel:1", "world:2:50"])
    assert [line["rc"] for line, _ in got] == [0] * 8
    assert [line["apply_static"] for line, _ in got] == [0, 0, 0, 0, 0, 0, 1, 1]
    assert [st["moving"] for _, st in got] == [0, 1, 1, 1, 0, 0, 1, 0]
    assert got[0][0]["make_front_end"] == 1 and got[4][0]["make_front_end"] == 1       # (every fresh list: the call may be the first)
    assert [line["what"] for line, _ in got[2:4]] == [R.STEP, R.READ] and got[2][0]["n"] == 2


def test_path_following_takes_a_nan_entry(harness):
    """inherited, not designed: usvmpc_guidance_world refuses it, usvmpc_pf_world does not"""
    (line, st), = calls(harness, "pf", ["world:2:50:nan=7"])
    assert line["rc"] == 0 and line["what"] == R.UPLOAD_LIST and st["set"] == 1 and st["nworld"] == 2


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_judged_call_that_is_not_committed_changes_nothing(harness, kind):
    toks = ["world:3:50", "vel:1", "vel:null:0", "fleet:3:0.5", "fleet:0:0", "step:0.5", "world:2:50", "read", "fstate"]
    got = calls(harness, kind, LIST2 + ["vel:0", "fleet:2:0.25", "commit:0"] + toks)
    before = got[2][1]
    assert (before["nworld"], before["nfixed"], before["fleet_S"], before["moving"], before["fleet_radius"]) == (3, 2, 2, 1, 0.25)
    for tok, (line, st) in zip(toks, got[3:]):
        assert line["rc"] == 0 or tok == "vel:null:0", tok
        assert st == before, tok
    # ... and, committed, they do what they said
    got = calls(harness, kind, LIST2 + ["vel:0", "fleet:2:0.25", "world:3:50"])
    assert got[-1][1]["nworld"] == 4 and got[-1][1]["nfixed"] == 3


@pytest.mark.parametrize("kind", R.KINDS)
def test_predicted_inside_the_horizon(harness, kind):
    """guidance stores world_vel's flag, and a fleet switched on over a world at rest forces it to 1; path-following reads option
    "pf_predict" at the time of asking.  want_static = not (moving and predicted)."""
    g = kind == "guidance"
    got = calls(harness, kind, ["pfpredict:0"] + LIST2 + ["fleet:3:0.5", "pfpredict:1", "state", "vel:0", "pfpredict:0", "state", "fleet:0:0",
                                                          "vel:null:0", "vel:0", "fleet:3:0.5"])
    (_, on), (_, opt1), (_, held), (_, opt0), _, _, _, (_, again) = got[1:]
    assert (on["moving"], on["predicted"], on["want_static"]) == ((1, 1, 0) if g else (1, 0, 1))    # over rest: guidance predicts
    assert (opt1["predicted"], opt1["want_static"]) == (1, 0)                                       # the option, now 1
    assert (held["predicted"], held["want_static"]) == ((0, 1) if g else (1, 0))                    # world_vel(.., predict 0): guidance only
    assert (opt0["predicted"], opt0["want_static"]) == (0, 1)
    assert (again["moving"], again["predicted"], again["want_static"]) == (1, 0, 1)                 # over a MOVING world: the choice stands


@pytest.mark.parametrize("kind", R.KINDS)
def test_read_and_step_descriptors(harness, kind):
    got = calls(harness, kind, ["world:3:50", "read", "vel:1", "read", "step:0.25", "fleet:2:0.5", "read", "step:0.25", "world:0:50", "read"])
    rest, moving, step, fleet_read, fleet_step, empty = got[1][0], got[3][0], got[4][0], got[6][0], got[7][0], got[9][0]
    assert (rest["what"], rest["n"], rest["vel_on_device"]) == (R.READ, 3, 0)         # a world at rest: the velocities are zero-filled
    assert (moving["what"], moving["n"], moving["vel_on_device"]) == (R.READ, 3, 1)
    assert (step["what"], step["n"]) == (R.STEP, 3)
    assert (fleet_read["n"], fleet_step["n"]) == (4, 4)                               # fixed entries and fleet slots alike
    assert (empty["what"], empty["n"], empty["vel_on_device"]) == (R.READ, 1, 1)      # a fleet's empty fixed list: the slot, still moving


@pytest.mark.parametrize("kind", R.KINDS)
def test_buffers_grow_only_when_they_must(harness, kind):
    """grow: the need exceeds the capacity - and, for velocities, also when no buffer exists yet (an empty list moves too)"""
    got = calls(harness, kind, ["world:0:50", "vel:1", "vel:1", "world:3:50", "world:2:50", "world:3:50", "world:64:50", "vel:1", "world:62:50",
                                "fleet:3:0.5", "fleet:0:0", "world:63:50", "fleet:2:0.5"])
    need = [line["need"] for line, _ in got]
    grow = [line["grow"] for line, _ in got]
    assert need == [0, 0, 0, 54, 36, 54, 1152, 768, 1116, 1152, 1116, 1134, 1152]
    assert grow == [0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0]
    assert [(line["need_vel"], line["grow_vel"]) for line, _ in got[9:11]] == [(768, 0), (744, 0)]
    assert got[-1][0]["grow_vel"] == 0 and got[-1][1]["nworld"] == 64 and got[-1][1]["list_cap"] == 1152 and got[-1][1]["vel_cap"] == 768
    assert got[1][1]["moving"] == 1 and got[1][1]["has_vel"] == 1 and got[1][1]["vel_cap"] == 0     # (the buffer of an empty list)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("Bn,S", [(6, 2), (6, 3), (6, 6)])
def test_fleet_sizes(harness, kind, Bn, S):
    """the fixed entries and S - 1 slots may fill the list of 64 exactly"""
    most = 64 - (S - 1)
    got = calls(harness, kind, ["B:%d" % Bn, "world:%d:50" % most, "fleet:%d:0.5" % S, "world:%d:50" % most, "vel:1", "fleet:0:0"])
    on, again, vel, off = got[1], got[2], got[3], got[4]
    assert (on[0]["what"], on[0]["n0"], on[0]["f0"], on[0]["n1_fixed"], on[0]["f1"], on[0]["new_fixed"]) == (R.RELAYOUT, most, 0, most, S - 1, 0)
    assert (on[1]["nworld"], on[1]["nfixed"], on[1]["fleet_S"]) == (64, most, S)
    assert (again[0]["what"], again[0]["n0"], again[0]["f0"], again[0]["n1_fixed"], again[0]["f1"], again[0]["new_fixed"]) == (R.RELAYOUT, 64, S - 1, most, S - 1, 1)
    assert (vel[0]["what"], vel[0]["nvel"], vel[0]["n"], vel[0]["need"]) == (R.MERGE_VEL, most, 64, Bn * most * 2)
    assert (off[0]["n0"], off[0]["f0"], off[0]["n1_fixed"], off[0]["f1"]) == (64, S - 1, most, 0)
    assert (off[1]["nworld"], off[1]["nfixed"], off[1]["fleet_S"], off[1]["moving"]) == (most, most, 0, 1)
    refused(harness, kind, ["B:%d" % Bn, "world:%d:50" % (most + 1)], "fleet:%d:0.5" % S, "fleet", "fits", dict(n_fixed=most + 1, slots=S - 1))


@pytest.mark.parametrize("kind", R.KINDS)
def test_which_buffers_are_made_first(harness, kind):
    """guidance: the slot tracks with the first list, the separation buffers with the first fleet (the host answers before that);
    path-following: its own buffers (the separations among them) with any fresh list, the tracks with the first velocities or relayout -
    a world that never moves makes none"""
    g = kind == "guidance"
    got = calls(harness, kind, ["fstate", "world:2:50", "world:3:50", "fstate", "fleet:3:0.5", "fstate", "fleet:0:0", "fleet:3:0.5", "vel:1"])
    lines = [line for line, _ in got]
    assert [ln["make_tracks"] for ln in lines] == ([0, 1, 0, 0, 0, 0, 0, 0, 0] if g else [0, 0, 0, 0, 1, 0, 0, 0, 0])
    assert [ln["make_front_end"] for ln in lines] == ([0] * 9 if g else [0, 1, 1, 0, 0, 0, 0, 0, 0])
    assert [ln["make_sep"] for ln in lines] == ([0, 0, 0, 0, 1, 0, 0, 0, 0] if g else [0] * 9)
    assert [lines[i]["host_answer"] for i in (0, 3, 5)] == ([1, 1, 0] if g else [0, 0, 0])
    assert got[3][1]["tracks"] == (1 if g else 0)
    first_vel = calls(harness, kind, ["world:2:50", "vel:1", "vel:1"])
    assert [line["make_tracks"] for line, _ in first_vel] == ([1, 0, 0] if g else [0, 1, 0])
