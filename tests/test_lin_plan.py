"""csrc/lin_plan.hpp, the schedule of the pipelined lineariser, compiled with the host compiler (CPU only) and driven from a command line
(tests/lin_plan_harness.cpp): when a solve pipelines, whether the pass made a tick ahead is used, under which map it runs, which lineariser
launches it makes over which grids, and what the writers of the schedule (caller writes, cancel, sync) do to it.

Every expected value is worked out by hand from usvmpc.hip's launch_solve as it stood before the schedule moved into the header - the
derivation stands next to the case.  That function, in the order it decided (h: the handle, n: h->nsolves):
    pipe      = phase == 0 && pipeline && !mirror && !extern_access && dynamic_rows && B >= 16384 && !(phase == 0 && cond_N2 > 0)
    wait      = spec_outstanding (then cleared), whatever pipe says
    had       = pipe && spec_for == n;  use = had && spec_valid;  had: use ? hits++ : misses++;  spec_valid = false
    map       : use -> spec_perm, map_changed = true;  else if sort_enabled && n > 0 && phase != 2 -> sort into d_perm (A), map_changed = true at
                phase 0 only;  else as it was
    pipe      : spec_quiet++;  spec_next = pipe && spec_quiet >= 2;  epoch on with spec_next, redo on and cleared with pipe
    mode      = use ? (spec_fine ? 4 : 2) : 0;  lin_force != 0 && mode == 0 && phase == 0: MODE 3 then 4 on a private epoch filled with
                n (lin_force 1) or -1 (2), paired launches + 2;  else one launch of `mode`, + 1
    spec_next : sort_enabled -> next map sorted into (perm == d_perm ? d_perm2 : d_perm)
    copy of d_iter_prev: sort_enabled && sort_two && phase == 0
    after the QP launch, spec_next: spec_fine = nothing handed over, MODE spec_fine ? 3 : 1; spec_for = n + 1, valid, outstanding, spec_perm = next map
Writers: a caller write of x / u / yref / yref_e cleared spec_valid and spec_quiet; spec_cancel did the same and synchronised the second
stream if spec_outstanding (then cleared); usvmpc_sync cleared spec_outstanding.
Grids: block 64 for MODE 3, else 256; n = Bp for MODE 4, (N + 1) Bp unpaired, rows of lin_order.hpp paired; per block 256 / 64 groups for
MODE 4, block / 16 else.  Maps below: 0 none, 1 buffer A (d_perm), 2 buffer B (d_perm2)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "lin_plan_harness.cpp")


def build(tmp_path_factory, name, *flags):
    exe = str(tmp_path_factory.mktemp(name) / "lin_plan_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, "-o", exe, SRC])
    return exe


# every case runs on the plain build and on one with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory, "lin_plan")
    return build(tmp_path_factory, "lin_plan_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, tokens):
    """One dict per printed line: the fields, integers where they are integers; `kind` is "solve", "cancel", "grid" or "redo_words"."""
    r = subprocess.run([exe] + tokens.split(), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        d = {"kind": "solve"}
        for w in line.split():
            if "=" in w:
                k, v = w.split("=", 1)
                d[k] = int(v) if v.lstrip("-").isdigit() else v
            else:
                d["kind"] = w
        if "redo_words" in d:
            d["kind"] = "redo_words"
        out.append(d)
    return out


def solves(exe, tokens):
    out = [d for d in run(exe, tokens) if d["kind"] == "solve"]
    assert len(out) == tokens.split().count("solve")
    return out


def check(p, **want):
    got = {k: p.get(k) for k in want}
    assert got == want, p


# ---- the pipeline boundary
def test_pipeline_from_16384_instances(harness):
    # B = 16383: B >= 16384 fails: never pipes - no quiet count, no pass ahead, redo off, however many quiet solves
    for p in solves(harness, "B=16383 solve solve solve solve"):
        check(p, pipe=0, spec_next=0, redo=0, clear_redo=0, ahead=-1, quiet=0, outstanding=0, hits=0, misses=0)
    # B = 16384: pipes from the first solve; the second quiet solve launches ahead
    a, b = solves(harness, "B=16384 solve solve")
    check(a, pipe=1, spec_next=0, redo=1, clear_redo=1, ahead=-1, quiet=1)
    check(b, pipe=1, spec_next=1, redo=1, clear_redo=1, ahead=3, quiet=2, made_for=2, valid=1, outstanding=1)


@pytest.mark.parametrize("off", ["mirror=1", "extern=1", "dynamic_rows=0", "cond=1", "pipeline=0", "phase=1", "phase=2"])
def test_pipeline_switched_off_by_each_condition_alone(harness, off):
    # each factor of `pipe`, alone, at B = 16384: no quiet count, so no pass ahead either
    for p in solves(harness, "B=16384 " + off + " solve solve solve"):
        check(p, pipe=0, spec_next=0, redo=0, clear_redo=0, ahead=-1, quiet=0, valid=0, outstanding=0)


# ---- tests/test_gpu_api.py::test_lineariser_runs_ahead_only_for_callers_that_do_not_write_between_ticks, restated
QUIET6 = "B=16384 N=10 " + "solve " * 6


def test_quiet_loop_uses_every_pass_made_ahead(harness):
    s = solves(harness, QUIET6)
    # solve 0: n = 0 - nothing made ahead, no sort (n > 0 fails), quiet 1 < 2: the whole-batch lineariser alone
    check(s[0], wait=0, use=0, map_from="keep", map=0, map_changed=0, spec_next=0, nlaunch=1, sort_next=0, ahead=-1, quiet=1, hits=0, misses=0)
    assert s[0]["l0"].startswith("0:")
    # solve 1: sorts into A (phase 0: map_changed), quiet 2: launches ahead - next map into the buffer not in use (perm == d_perm -> d_perm2 = B),
    # nothing handed over -> MODE 3; made for solve 2
    check(s[1], wait=0, use=0, map_from="sort", map=1, map_changed=1, spec_next=1, sort_next=1, next_map=2, ahead=3, made_for=2, valid=1,
          outstanding=1, smap=2, fine=1, quiet=2, hits=0, misses=0)
    assert s[1]["l0"].startswith("0:")
    # solves 2 .. 5: wait for the pass, use it (hit), run under its map with the fix-up MODE 4 only, sort the next map into the other buffer
    for t, (cur, nxt) in zip(range(2, 6), [(2, 1), (1, 2), (2, 1), (1, 2)]):
        check(s[t], wait=1, use=1, map_from="ahead", map=cur, map_changed=1, spec_next=1, nlaunch=1, sort_next=1, next_map=nxt, ahead=3,
              made_for=t + 1, valid=1, outstanding=1, smap=nxt, quiet=t + 1, hits=t - 1, misses=0)
        assert s[t]["l0"].startswith("4:")
    check(s[5], hits=4, misses=0)


def test_writing_caller_discards_one_pass_and_causes_no_other(harness):
    # ... then five solves with a write in front of each.  The first: the pass made for solve 6 is outstanding (wait) and was made for it
    # (had) but no longer valid: one miss; sorts into A again; quiet was reset, 1 < 2: nothing ahead.  The others: spec_for = 6 != n: neither
    # hit nor miss, quiet back to 1 each time
    s = solves(harness, QUIET6 + "write solve " * 5)[6:]
    check(s[0], wait=1, use=0, map_from="sort", map=1, map_changed=1, spec_next=0, sort_next=0, ahead=-1, valid=0, outstanding=0, quiet=1, hits=4, misses=1)
    for p in s[1:]:
        check(p, wait=0, use=0, map_from="sort", map=1, spec_next=0, ahead=-1, valid=0, outstanding=0, quiet=1, hits=4, misses=1)
    for p in s:
        assert p["nlaunch"] == 1 and p["l0"].startswith("0:")
    # as the GPU test does it, with a sync in between: the same counts, and the first solve has nothing to wait for
    s = solves(harness, QUIET6 + "sync " + "write solve " * 5)[6:]
    check(s[0], wait=0, use=0, hits=4, misses=1)
    check(s[4], wait=0, use=0, hits=4, misses=1, quiet=1)


def test_write_on_a_handle_with_a_mirror_is_the_same_call(harness):
    # copy_field's mirror path cleared spec_quiet only, its device path spec_valid too.  One call serves both: with a mirror pipe is false, so
    # nothing is ever launched ahead and spec_valid is false wherever the mirror path runs - clearing it changes nothing
    for p in solves(harness, "B=16384 mirror=1 solve solve write solve solve solve"):
        check(p, pipe=0, use=0, valid=0, quiet=0, ahead=-1, hits=0, misses=0)
    # (the mirror given up - option "host_mirror" 0 goes through spec_cancel -: the handle pipelines from then on as any other)
    s = solves(harness, "B=16384 mirror=1 solve write solve mirror=0 cancel solve solve solve")
    check(s[3], pipe=1, spec_next=1, ahead=3, quiet=2)
    check(s[4], use=1, hits=1, misses=0)


# ---- map choice and hand-over
def test_fixup_mode_follows_the_form_of_the_pass(harness):
    # hand = 0: spec_fine -> ahead MODE 3, its fix-up MODE 4; hand = 1: MODE 1, fix-up MODE 2
    s = solves(harness, "B=16384 hand=0 solve solve solve")
    check(s[1], ahead=3, fine=1)
    assert s[2]["l0"].startswith("4:")
    s = solves(harness, "B=16384 hand=1 solve solve solve hand=0 solve")
    check(s[1], ahead=1, fine=0)
    check(s[2], use=1, ahead=1, fine=0)
    assert s[2]["l0"].startswith("2:")
    # (the fix-up belongs to the pass it follows, not to what this solve's own launch hands over)
    check(s[3], use=1, ahead=3, fine=1)
    assert s[3]["l0"].startswith("2:")


def test_sorting_off_runs_ahead_under_the_identity(harness):
    # sort_enabled = 0: no sort ever, the pass ahead gets no map (next_perm stays nullptr); using it still sets map_changed (the quirk kept)
    s = solves(harness, "B=16384 sort=0 solve solve solve solve")
    check(s[0], map_from="keep", map=0, map_changed=0)
    check(s[1], map_from="keep", map=0, map_changed=0, spec_next=1, sort_next=0, next_map=0, ahead=3, smap=0)
    for p in s[2:]:
        check(p, use=1, map_from="ahead", map=0, map_changed=1, sort_next=0, next_map=0, smap=0)


def test_map_by_phase(harness):
    # n = 0: no sort at any phase.  Then phase 2 never sorts, phase 1 sorts into A and leaves map_changed alone, phase 0 sets it
    s = solves(harness, "B=64 phase=1 solve phase=2 solve phase=1 solve phase=2 solve phase=0 solve")
    check(s[0], map_from="keep", map=0, map_changed=0)
    check(s[1], map_from="keep", map=0, map_changed=0)
    check(s[2], map_from="sort", map=1, map_changed=0)
    check(s[3], map_from="keep", map=1, map_changed=0)
    check(s[4], map_from="sort", map=1, map_changed=1)
    # sorting off: the map stays what it is at every phase (usvmpc_set_option has set it to none: map=0)
    for p in solves(harness, "B=64 solve sort=0 map=0 solve phase=1 solve phase=2 solve"):
        check(p, map_from="keep", map=0, map_changed=0)


def test_next_map_goes_into_the_buffer_the_solve_does_not_use(harness):
    # a solve that discards the pass sorts into A itself: the next map then goes into B whatever the discarded pass used
    s = solves(harness, "B=16384 solve solve solve cancel solve solve solve")
    check(s[2], map=2, next_map=1, smap=1)
    check(s[3], use=0, map_from="sort", map=1, spec_next=0, quiet=1, misses=1)
    check(s[4], use=0, map_from="sort", map=1, spec_next=1, next_map=2, smap=2)
    check(s[5], use=1, map_from="ahead", map=2, next_map=1, hits=2, misses=1)


# ---- sort_two
def test_iter_prev_copied_at_phase_0_with_sorting_on_only(harness):
    s = solves(harness, "B=64 sort_two=1 solve solve phase=1 solve phase=2 solve phase=0 sort=0 solve sort=1 sort_two=0 solve")
    assert [p["copy_iter_prev"] for p in s] == [1, 1, 0, 0, 0, 0]  # (the first solve included: no n > 0 in that condition)
    assert solves(harness, "B=16384 sort_two=1 solve solve solve")[2]["copy_iter_prev"] == 1  # (pipelined or not)


# ---- lin_force_modes
@pytest.mark.parametrize("force,fills", [(1, [0, 1, 2, 3]), (2, [-1, -1, -1, -1])])
def test_lin_force_runs_the_pipeline_kernels_in_place(harness, force, fills):
    # B = 1003 (no pipeline): every phase-0 solve has mode 0 -> MODE 3 then MODE 4, epoch filled with the tick (1) or -1 (2), two paired launches
    s = solves(harness, "B=1003 N=12 lin_force=%d solve solve solve solve" % force)
    for p, fill in zip(s, fills):
        check(p, forced=1, nlaunch=2, force_epoch=fill, pair_launches=2, l0="3:1757:64:7028", l1="4:251:256:1004")
    # unpaired: the same launches over the unpaired grids, none counted
    p, = solves(harness, "B=1003 N=12 pairs=0 lin_force=%d solve" % force)
    check(p, forced=1, nlaunch=2, pair_launches=0, l0="3:3263:64:13052", l1="4:251:256:1004")


def test_lin_force_ignored_off_phase_0_and_when_a_pass_is_used(harness):
    # phase != 0: one launch of MODE 0, one paired launch counted
    for p in solves(harness, "B=1003 N=12 lin_force=1 solve phase=1 solve phase=2 solve")[1:]:
        check(p, forced=0, nlaunch=1, pair_launches=1, l0="0:408:256:6528")
    # a pipelining handle: forced while it runs the whole-batch lineariser (solves 0, 1), not when the pass made ahead is used (mode 4)
    s = solves(harness, "B=16384 lin_force=2 solve solve solve pairs=0 solve")
    check(s[0], forced=1, nlaunch=2, force_epoch=-1, pair_launches=2, spec_next=0)
    check(s[1], forced=1, nlaunch=2, force_epoch=-1, pair_launches=2, spec_next=1, ahead=3)
    check(s[2], forced=0, use=1, nlaunch=1, pair_launches=1, l0="4:4096:256:16384")
    check(s[3], forced=0, use=1, nlaunch=1, pair_launches=0, l0="4:4096:256:16384")


# ---- cancel, sync
def test_cancel_asks_for_the_synchronise_once(harness):
    out = run(harness, "B=16384 solve solve cancel cancel solve")
    assert [d["sync"] for d in out if d["kind"] == "cancel"] == [1, 0]
    # the cancelled pass was made for this solve: a miss, nothing to wait for any more, quiet starts again
    check(out[-1], wait=0, use=0, misses=1, hits=0, quiet=1, spec_next=0)
    # nothing outstanding: no synchronise
    assert run(harness, "B=16384 solve cancel")[-1]["sync"] == 0


def test_sync_then_solve_does_not_wait_again(harness):
    s = solves(harness, "B=16384 solve solve sync solve solve")
    check(s[2], wait=0, use=1, hits=1)  # (synchronised, still valid: used)
    check(s[3], wait=1, use=1, hits=2)
    # ... and a cancel after a sync has nothing to synchronise
    assert [d["sync"] for d in run(harness, "B=16384 solve solve sync cancel") if d["kind"] == "cancel"] == [0]


def test_full_sqp_consumes_a_cancelled_pass_without_counting_it(harness):
    # usvmpc_solve_sqp cancels first; its launches do not pipe, so `had` is false: neither hit nor miss; the RTI solve after it (n = 4) finds
    # spec_for = 2: nothing either
    s = solves(harness, "B=16384 solve solve cancel phase=1 solve phase=2 solve phase=0 solve solve")
    for p in s[2:4]:
        check(p, pipe=0, wait=0, use=0, hits=0, misses=0, quiet=0)
    check(s[4], pipe=1, wait=0, use=0, hits=0, misses=0, quiet=1, spec_next=0)
    check(s[5], spec_next=1, quiet=2, made_for=6)


# ---- grids
def grids(exe, tokens):
    out = run(exe, tokens + " grid")
    return {(d["pairs"], d["mode"]): (d["count"], d["blocks"], d["block"]) for d in out if d["kind"] == "grid"}, out[-1]["redo_words"]


def test_grids_even_stage_count(harness):
    # N = 20, Bp = 16392.  Unpaired: n = 21 * 16392 = 344232 pairs; 16 per 256-thread block: 21514.5 -> 21515; MODE 3: 4 items per wave: 86058.
    # MODE 4: n = Bp groups, 4 per block: 4098.  Paired, stage-major: 344232 pairs / 2 = 172116 rows (a multiple of 4 already):
    # 172116 / 16 = 10757.25 -> 10758 blocks; retire order: (20 + 2) / 2 = 11 rows per instance * 16392 = 180312 (a multiple of 4): / 4 = 45078
    g, words = grids(harness, "B=16391 N=20")
    for mode in (0, 1, 2):
        assert g[(0, mode)] == (344232, 21515, 256)
        assert g[(1, mode)] == (172116, 10758, 256)
    assert g[(0, 3)] == (344232, 86058, 64)
    assert g[(1, 3)] == (180312, 45078, 64)
    assert g[(0, 4)] == g[(1, 4)] == (16392, 4098, 256)
    assert words == 1  # 21 stage bits


def test_grids_odd_stage_count(harness):
    # N = 12, Bp = 1004: 13 stages.  Unpaired: 13052 pairs: / 16 = 815.75 -> 816; MODE 3: 3263.  MODE 4: 1004 / 4 = 251.
    # Paired, stage-major: 13052 / 2 = 6526 rows, padded to whole waves of four rows: 6528 -> 408 blocks; retire order: (12 + 2) / 2 = 7 rows
    # per instance (the last one half idle) * 1004 = 7028 = 4 * 1757
    g, words = grids(harness, "B=1003 N=12")
    for mode in (0, 1, 2):
        assert g[(0, mode)] == (13052, 816, 256)
        assert g[(1, mode)] == (6528, 408, 256)
    assert g[(0, 3)] == (13052, 3263, 64)
    assert g[(1, 3)] == (7028, 1757, 64)
    assert g[(0, 4)] == g[(1, 4)] == (1004, 251, 256)
    assert words == 1
    # one bit per stage 0 .. N: 32 stages fit a word, 33 need two
    assert grids(harness, "B=4 N=31")[1] == 1 and grids(harness, "B=4 N=32")[1] == 2 and grids(harness, "B=4 N=100")[1] == 4
