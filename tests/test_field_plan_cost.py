"""The three objective-value rows of csrc/field_plan.hpp's field table - "cost", "cost_stage", "cost_parts" - through the harness of
tests/test_field_plan.py (tests/field_plan_harness.cpp, unchanged): get and device-pointer rights only, lengths 1 / 1 / 3, "cost" and
"cost_parts" whole-only (one row per instance whatever the stage), "cost_stage" over stages 0 .. N."""
import pytest

from tests.test_field_plan import MODELS, harness, run, sizes  # noqa: F401  (harness: the fixture, plain and sanitized)

COST = {"cost": (1, 1, 1), "cost_stage": (1, None, 0), "cost_parts": (3, 1, 1)}  # name -> (length, stages or None for N + 1, whole-only)


def test_rights_and_flags(harness):
    rows = {d["name"]: d for d in run(harness, " ".join("row:" + n for n in COST)) if d["kind"] == "row"}
    for n, (_, _, whole) in COST.items():
        r = rows[n]
        assert r["found"] == 1
        assert (r["set"], r["get"], r["get_int"], r["dev"]) == (0, 1, 0, 1), n
        assert (r["slot"], r["int"], r["whole"]) == (-1, 0, whole), n
        assert (r["lin"], r["pf"], r["export"], r["track"]) == (0, 0, 0, 0), n   # no caller write, no front end, no other machinery
    ids = sorted(rows[n]["id"] for n in COST)
    assert ids == list(range(ids[0], ids[0] + 3)) and ids[0] > max(d["id"] for d in run(harness, "row:clearance_min"))  # (appended)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_lengths_stages_and_refusals(harness, model):
    nx, nu, K = MODELS[model]
    N, B = 6, 3
    sz = sizes(nx, nu, K, N=N, B=B)
    for n, (length, stages, whole) in COST.items():
        stages = N + 1 if stages is None else stages
        assert run(harness, sz + " q:set:%s:0 q:set:%s:-1" % (n, n)) == [{"kind": "q", "rc": -2}] * 2, n   # get-only: set is refused
        q = run(harness, sz + " q:get:%s:-1" % n)[0]
        assert (q["rc"], q["as"], q["slot"], q["n"], q["stages"], q["stage_off"], q["check"]) == (0, n, -1, length, stages, 0, 0), n
        # the whole array as one piece
        assert (q["off"], q["width"], q["rows"]) == (0, B * stages * length * 8, 1), n
        if whole:   # whatever stage the caller names, it is the field's only row
            for st in (0, 3, N, N + 5):
                q = run(harness, sz + " q:get:%s:%d" % (n, st))[0]
                assert (q["rc"], q["stage"], q["check"], q["width"], q["rows"]) == (0, 0, 0, B * length * 8, 1), (n, st)
    for st in range(N + 1):   # one stage of every instance: B pieces of 8 bytes, a row of N + 1 apart
        q = run(harness, sz + " q:get:cost_stage:%d" % st)[0]
        assert (q["rc"], q["check"], q["off"], q["pitch"], q["width"], q["rows"]) == (0, 0, 8 * st, 8 * (N + 1), 8, B), st
    q = run(harness, sz + " q:get:cost_stage:%d" % (N + 1))[0]
    assert q["rc"] == 0 and q["check"] == 1   # "stage N + 1 out of range for field 'cost_stage'"
