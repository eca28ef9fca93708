"""csrc/world_plan.hpp for exchanged plans - the judge `plans`, what it refuses and in which order, the three-state member PlanState and every
event that moves it - compiled with the host compiler (CPU only) and driven from a command line (tests/world_plan_plans_harness.cpp), for
both front ends, on a plain build and on one with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded).

Every expected value is written out by hand: the refusals' words in tests/fleet_plans_ref.py (which tests/test_gpu_fleet_plans_refusals.py
holds the library on the device to as well), the states below from the table of include/usvmpc.h."""
import os
import subprocess

import pytest

from tests import fleet_plans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "world_plan_plans_harness.cpp")
NONE, SOLVED, SHIFTED = R.PLAN_NONE, R.PLAN_SOLVED, R.PLAN_SHIFTED
WORLD_PLANS, WORLD_PLAN_STATE = 8, 9       # WorldDo


def build(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp(name) / "world_plan_plans_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory, "world_plan_plans")
    return build(tmp_path_factory, "world_plan_plans_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, kind, tokens):
    """[(call or event line, state line after it)]; `err` is the text to the end of the line"""
    r = subprocess.run([exe, "kind:" + kind[0]] + tokens, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        head, _, err = line.partition(" err=")
        w = head.split()
        d = {"line": w[0], "err": err}
        d.update((k, int(v)) for k, v in (kv.split("=", 1) for kv in w[1:]))
        out.append(d)
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


FLEET_ON = ["world:0", "fleet:2"]


@pytest.mark.parametrize("kind", R.KINDS)
def test_refusals_word_for_word_and_in_order(harness, kind):
    """everything wrong at once, then one thing put right at a time: each refusal is met in the entry point's order, and changes nothing"""
    peel = {"model": ["model:1"], "reset": ["ready:1"], "fleet": FLEET_ON, "N": ["N:6"]}
    tokens, expect = ["model:0", "ready:0", "N:1", "state"], []
    for key, text in R.REFUSALS[kind]:
        tokens += ["plans:1"] + peel[key]
        expect.append(text)
    got = run(harness, kind, tokens + ["plans:1"])
    before = got[0][1]
    assert before["plans"] == 0 and before["plan"] == NONE and before["plan_bufs"] == 0
    calls = [(line, state) for line, state in got if line is not None and line["line"] == "plans"]
    assert len(calls) == len(expect) + 1
    for (line, state), text in zip(calls, expect):
        assert line["rc"] == -1 and line["err"] == text, (line, text)
        assert (state["plans"], state["plan"], state["plan_bufs"]) == (0, NONE, 0), text       # a refused call changes nothing
    line, state = calls[-1]
    assert line["rc"] == 0 and line["what"] == WORLD_PLANS and line["make_plans"] == 1
    assert (state["plans"], state["plan"], state["plan_bufs"], state["records"], state["usable"]) == (1, NONE, 1, 1, 0)


@pytest.mark.parametrize("kind", R.KINDS)
def test_plan_state_refusals_and_answers(harness, kind):
    got = run(harness, kind, ["model:0", "ready:0", "pstate", "model:1", "pstate", "ready:1", "pstate"] + FLEET_ON + ["plans:1", "pstate", "plans:0", "pstate"])
    ps = [line for line, _ in got if line is not None and line["line"] == "pstate"]
    for line, (_, text) in zip(ps, R.STATE_REFUSALS[kind]):
        assert line["rc"] == -1 and line["err"] == text
    assert ps[2]["rc"] == 0 and ps[2]["what"] == WORLD_PLAN_STATE and ps[2]["host_answer"] == 1      # plans were never on: -1, 0 from the host
    assert ps[3]["rc"] == 0 and ps[3]["host_answer"] == 0
    assert ps[4]["rc"] == 0 and ps[4]["host_answer"] == 0                                             # the buffers stay


# (event, plan state afterwards, a prepare launched the plan kernel) - from the table: NONE / SOLVED / SHIFTED and what enters each
SCRIPT = [
    ("plans:1", NONE, 0),
    ("prepare", NONE, 0),          # tick 0: nothing solved yet
    ("solve", SOLVED, 0),
    ("prepare", SOLVED, 0),        # solved but not handed over
    ("advance", SHIFTED, 0),
    ("prepare", NONE, 1),          # the one prepare that launches; it uses the plan up
    ("prepare", NONE, 0),          # prepare twice with no hand-over
    ("solve", SOLVED, 0),
    ("solve", SOLVED, 0),          # solve twice
    ("advance", SHIFTED, 0),
    ("advance", NONE, 0),          # a second hand-over with no solve in between
    ("prepare", NONE, 0),
    ("advance", NONE, 0),          # a hand-over of nothing
    ("solve", SOLVED, 0), ("advance", SHIFTED, 0),
    ("setx", NONE, 0),             # a caller write of x
    ("solve", SOLVED, 0),
    ("setx", NONE, 0),
    ("solve", SOLVED, 0), ("advance", SHIFTED, 0),
    ("reset", NONE, 0),            # the front end's reset
    ("solve", SOLVED, 0), ("advance", SHIFTED, 0),
    ("plans:1", NONE, 0),          # switching plans on (again)
    ("solve", SOLVED, 0), ("advance", SHIFTED, 0),
    ("fleet:0", NONE, 0),          # the fleet switched off
    ("solve", SOLVED, 0), ("advance", SHIFTED, 0),
    ("prepare", SHIFTED, 0),       # no fleet: today's prepare, nothing used
    ("fleet:0", NONE, 0),          # off while off
    ("fleet:2", NONE, 0),
    ("solve", SOLVED, 0), ("advance", SHIFTED, 0),
    ("fleet:3", SHIFTED, 0),       # another scene size: the iterate is what it was
    ("prepare", NONE, 1),
    ("solve", SOLVED, 0), ("advance", SHIFTED, 0),
    ("plans:0", SHIFTED, 0),       # off: the state is kept up, nothing is launched
    ("prepare", SHIFTED, 0),
    ("solve", SOLVED, 0), ("advance", SHIFTED, 0),
    ("prepare", SHIFTED, 0),
    ("plans:1", NONE, 0),
    ("solve", SOLVED, 0), ("advance", SHIFTED, 0),
    ("prepare", NONE, 1),
]


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_transition_of_the_three_states(harness, kind):
    got = run(harness, kind, FLEET_ON + [ev for ev, _, _ in SCRIPT])[len(FLEET_ON):]
    launches = 0
    for i, ((ev, plan, launched), (line, state)) in enumerate(zip(SCRIPT, got)):
        what = "step %d, %s" % (i, ev)
        assert line["line"] == ev.split(":")[0], what
        if "rc" in line:
            assert line["rc"] == 0, (what, line["err"])
        else:
            assert line["launched"] == launched, what
        launches += launched
        assert state["plan"] == plan and state["launches"] == launches, (what, state)
        assert state["usable"] == int(state["plans"] == 1 and state["fleet_S"] >= 2 and plan == SHIFTED), what
    assert launches == 3
    first = run(harness, kind, FLEET_ON + ["plans:1", "plans:0", "plans:1"])
    assert [line["make_plans"] for line, _ in first[2:]] == [1, 0, 0]                # the buffers are made once


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_world_that_is_not_predicted_launches_nothing(harness, kind):
    """"pf_predict" 0 / predict=False: the scene is held still inside the horizon, the plan kernel is not launched and no plan is used up"""
    off = ["pfpredict:0"] if kind == "pf" else ["vel:0"]
    on = ["pfpredict:1"] if kind == "pf" else ["vel:1"]
    got = run(harness, kind, FLEET_ON + ["plans:1", "solve", "advance"] + off + ["prepare"] + on + ["prepare", "prepare"])
    prepares = [(line, state) for line, state in got if line is not None and line["line"] == "prepare"]
    assert [line["launched"] for line, _ in prepares] == [0, 1, 0]
    assert [state["plan"] for _, state in prepares] == [SHIFTED, NONE, NONE]
    assert prepares[0][1]["records"] == 0 and prepares[1][1]["records"] == 1


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_refused_or_failed_call_changes_nothing(harness, kind):
    got = run(harness, kind, FLEET_ON + ["solve", "advance", "state", "N:1", "plans:1", "N:6", "commit:0", "plans:1", "commit:1", "plans:1", "solve",
                                         "advance", "state", "model:0", "plans:0", "model:1", "commit:0", "plans:0", "fleet:0", "commit:1", "state"])
    states = [state for line, state in got if line is None]
    calls = [(line, state) for line, state in got if line is not None and line["line"] in ("plans", "fleet")][1:]
    before = states[0]
    assert (before["plans"], before["plan"], before["plan_bufs"]) == (0, SHIFTED, 0)
    assert calls[0][0]["rc"] == -1 and calls[0][1] == before                       # refused: N = 1
    assert calls[1][0]["rc"] == 0 and calls[1][1] == before                        # judged, the carrier failed: not committed
    assert calls[2][0]["rc"] == 0 and (calls[2][1]["plans"], calls[2][1]["plan"], calls[2][1]["plan_bufs"]) == (1, NONE, 1)
    on = states[1]
    assert (on["plans"], on["plan"], on["usable"]) == (1, SHIFTED, 1)
    assert calls[3][0]["rc"] == -1 and calls[3][1] == on                           # refused: another model
    assert calls[4][0]["rc"] == 0 and calls[4][1] == on                            # plans off, not committed
    assert calls[5][0]["rc"] == 0 and calls[5][1] == on                            # fleet off, not committed
    assert states[2] == on
