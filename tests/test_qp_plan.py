"""csrc/qp_plan.hpp, the QP launch policy, compiled with the host compiler (CPU only) and run against a device made of numbers
(tests/qp_plan_harness.cpp): which kernel, grid, dynamic LDS and kernel arguments a batch gets, when it hands over, what is probed and when.

Every expected value is worked out by hand from the policy as usvmpc.hip's launch_qp stated it before the policy moved into the header -
the derivation stands next to the case.  The figures below are the ones those derivations use."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")

# The harness' handle: npt = 36 planes per stage, nplw = 28 of them in LDS, exchange areas of 6 (LDS) / 10 (HBM) planes, nu = 2,
# aux_dense4 = 4, one obstacle chunk of hard rows (kch = k_kch = 1, k_soft = 0, K = 3), every kernel in the table, 256 CUs, options at
# their defaults.  Bp = B rounded up to four unless given.
# The device: a CU holds min(max_<slot>, 163840 // (st_<slot> + dynamic bytes)) workgroups; max 8 and static 0 unless set here:
DEV = ["max_qp=2", "st_qp=10240", "max_qp_aux=2", "st_qp_aux=6860"]
# Bytes, by horizon N (one plane row = 128 bytes):
#   P(N)   = (N + 1) * 28 * 128   an instance's planes in LDS          P(10) = 39424  P(20) = 75264  P(40) = 146944  P(100) = 361984
#   b4(N)  = P + 16*6*128 + 128   four waves, planes in LDS            b4(20) = 87680  b4(40) = 159360  b4(100) = 374400
#   x4     = 16*10*128 + 128      four waves, planes in HBM            20608
#   w1(N)  = P + 4*6*128          one wave, planes in LDS (and the follow-up kernel in LDS)   w1(20) = 78336  w1(40) = 150016  w1(100) = 365056
#   xb     = 4*10*128             one wave, planes in HBM (and the follow-up kernel over HBM)  5120
#   inst(N) = (N + 1) * 36 * 128  an instance's workspace              inst(10) = 50688  inst(20) = 96768  inst(40) = 188928
#   aux(N) = 4 * (N + 1) * (4 + 2 + 2*2) * 8                           aux(10) = 3520  aux(20) = 6720  aux(40) = 13120
# What the device then answers (workgroups per CU -> cap):
#   wide_lds4: b4(20), b4(40) -> 1 -> 256 workgroups (one per CU); b4(100) -> 0 -> -1.   wide_hbm4: x4 -> 7 -> 256
#   wide_lds1: w1(20) -> 2 -> 512 waves; w1(40) -> 1 -> 256; w1(100) -> 0 -> -1.          wide_hbm1: xb -> min(8, 32) -> at most 4 -> 1024
#   qp: 10240 static -> min(2, 16) = 2 -> 4 * 2 * 256 = 2048 groups.   qp_aux at N = 40: 6860 + 13120 -> min(2, 8) = 2 -> 2048 >= 2048: taken
#   resume_lds: w1(40) -> 1 -> 256, w1(20) -> 2 -> 512, w1(100) -> 0, then resume: xb -> 8 -> at most 4 -> 1024 over HBM


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qp_plan") / "qp_plan_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "qp_plan_harness.cpp")])
    return exe


def plans(exe, *tokens):
    """One dict per "plan" token (a trailing one is added): the printed fields, integers where they are integers."""
    words = DEV + " ".join(tokens).split()
    if words[-1] != "plan":
        words.append("plan")
    r = subprocess.run([exe] + words, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        d = dict(w.split("=", 1) for w in line.split())
        out.append({k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in d.items()})
    assert len(out) == words.count("plan")
    return out


def check(p, **want):
    got = {k: p[k] for k in want}
    assert got == want, p


NO_HAND = dict(hand=0, hand_iter=0, co=0, co_wgs=0)
THROUGHPUT_PROBES = "wide_lds4:256:159360,wide_lds1:64:150016,static:qp_lds,qp:64:0,qp_aux:64:13120,resume_lds:64:150016"


# ---- the throughput path
def test_throughput_large_batch(harness):
    # N = 40, B = 65536: four waves: cap 256, reach 512 < B, hard rows with K = 3 anyway; one wave: cap 256, B > 512; rows_lds = 163840 // 188928 = 0;
    # qp_cap 2048, aux cap 2048 >= 2048: aux kernel with 13120 bytes, ngroups = q0 = 2048 < Bp, grid = 2048 * 16 / 64; B > 3 * 2048: no hand-over,
    # though the follow-up kernel was probed (in LDS: 256) and its buffers are wanted
    p, = plans(harness, "N=40 B=65536")
    check(p, slot="qp_aux", grid=512, block=64, lds=13120, ngroups=2048, q0=2048, rows=4, mapping=0, hand_ready=1, **NO_HAND)
    check(p, cap_qp=2048, cap_aux=2048, cap_wide4=256, cap_wide=256, cap_wide_hbm=0, cap_wide4_hbm=0, cap_lds=0, cap_resume=256, cap_resume_lds=1,
          cap_lds_static=0, probes=THROUGHPUT_PROBES)


def test_throughput_aux_costs_a_wave(harness):
    # the aux kernel with 80000 bytes static: 163840 // 93120 = 1 -> 1024 < qp_cap: -1, plain qp without dynamic LDS - and not asked again
    p, q = plans(harness, "N=40 B=65536 st_qp_aux=80000 plan plan")
    for r in (p, q):
        check(r, slot="qp", grid=512, lds=0, ngroups=2048, q0=2048, rows=4, mapping=0, cap_aux=-1, cap_qp=2048, **NO_HAND)
    assert "qp_aux:64:13120" in p["probes"] and q["probes"] == ""


def test_throughput_aux_needs_the_queue_and_the_option(harness):
    # aux_in_lds = 0, or dynamic_rows = 0 (qp_cap is then not even asked: ngroups = Bp, no queue): plain qp
    p, = plans(harness, "N=40 B=65536 aux_in_lds=0")
    check(p, slot="qp", lds=0, ngroups=2048, q0=2048, cap_aux=0)
    p, = plans(harness, "N=40 B=65536 dynamic_rows=0")
    check(p, slot="qp", lds=0, ngroups=65536, q0=-1, grid=16384, cap_qp=0, cap_aux=0, **NO_HAND)
    assert "qp:" not in p["probes"]


# ---- hand-over
def test_handover_default_up_to_three_times_the_resident_rows(harness):
    # B = 3 * 2048: small, follow-up in LDS -> past 20 iterations; follow-up launch min(256, B) workgroups of w1(40) bytes; beside the launch
    # min(256, B, one per CU = 256)
    p, = plans(harness, "N=40 B=6144")
    check(p, slot="qp_aux", ngroups=2048, q0=2048, grid=512, mapping=0, hand_ready=1, hand=1, hand_iter=20, hand_lds=1, hand_bytes=150016, hand_wgs=256, co=1, co_wgs=256)
    # one more instance: not small
    p, = plans(harness, "N=40 B=6145")
    check(p, slot="qp_aux", ngroups=2048, q0=2048, hand_ready=1, **NO_HAND)


def test_handover_never_by_default_over_hbm(harness):
    # handover_lds = 0: only the kernel over HBM is probed (xb -> 4 per CU -> 1024), resume_lds false -> default iteration 0
    p, = plans(harness, "N=40 B=6144 handover_lds=0")
    check(p, hand_ready=1, cap_resume=1024, cap_resume_lds=0, **NO_HAND)
    assert p["probes"].endswith("qp_aux:64:13120,resume:64:5120")
    # ... but an explicit handover_iter hands over to it: 5120 bytes, min(1024, B) workgroups, never beside the launch
    p, = plans(harness, "N=40 B=6144 handover_lds=0 handover_iter=25")
    check(p, hand=1, hand_iter=25, hand_lds=0, hand_bytes=5120, hand_wgs=1024, co=0)


def test_handover_explicit_iteration_at_any_size(harness):
    p, = plans(harness, "N=40 B=65536 handover_iter=30")
    check(p, ngroups=2048, q0=2048, hand=1, hand_iter=30, hand_lds=1, hand_bytes=150016, hand_wgs=256, co=1, co_wgs=256)
    # handover_iter = 0: never, and the follow-up kernels are not probed
    p, = plans(harness, "N=40 B=6144 handover_iter=0")
    check(p, hand_ready=0, cap_resume=0, **NO_HAND)
    assert "resume" not in p["probes"]


@pytest.mark.parametrize("opt", ["own_stream=0", "handover_co=0", "has_resume_co=0"])
def test_handover_without_the_co_resident_kernel(harness, opt):
    p, = plans(harness, "N=40 B=6144", opt)
    check(p, hand=1, hand_iter=20, hand_lds=1, hand_wgs=256, co=0, co_wgs=0)


def test_handover_co_workgroups(harness):
    p, = plans(harness, "N=40 B=6144 co_wgs=7")
    check(p, hand=1, co=1, co_wgs=7, hand_wgs=256)
    # more than the follow-up launch has: min(resume_cap, B) stays the ceiling
    p, = plans(harness, "N=40 B=6144 co_wgs=1000")
    check(p, co=1, co_wgs=256)


# ---- one wave per instance, planes in LDS (hard rows, K = 3, N = 20: four waves are probed - cap 256 - and not taken)
def test_one_wave_small_batch(harness):
    p, = plans(harness, "N=20 B=64")
    check(p, slot="wide_lds1", grid=64, block=64, lds=78336, ngroups=64, q0=-1, rows=1, mapping=1, hand_ready=0, cap_wide=512, cap_wide4=256, **NO_HAND)
    assert p["probes"] == "wide_lds4:256:87680,wide_lds1:64:78336"


def test_one_wave_twice_the_resident_waves(harness):
    # B = 2 * 512: the queue hands out the second half
    p, = plans(harness, "N=20 B=1024")
    check(p, slot="wide_lds1", grid=512, ngroups=512, q0=512, rows=1, mapping=1)
    # B = 1025: throughput mapping; rows_lds = 1 but B > 1 * 256; aux(20): 6860 + 6720 -> 2 -> 2048; 2048 is not below Bp = 1028: no queue
    p, = plans(harness, "N=20 B=1025")
    check(p, slot="qp_aux", grid=257, lds=6720, ngroups=1028, q0=-1, rows=4, mapping=0)


def test_one_wave_forced_without_the_queue(harness):
    # wide = 1, dynamic_rows = 0: every instance its workgroup at launch
    p, = plans(harness, "N=20 B=2000 wide=1 dynamic_rows=0")
    check(p, slot="wide_lds1", grid=2000, ngroups=2000, q0=-1, mapping=1)
    # wide = 1 with the queue: capped
    p, = plans(harness, "N=20 B=2000 wide=1")
    check(p, slot="wide_lds1", grid=512, ngroups=512, q0=512, mapping=1)
    # wide = 0: never (nor probed)
    p, = plans(harness, "N=20 B=64 wide=0 lds_workspace=0")
    check(p, slot="qp_aux", mapping=0, cap_wide=0, cap_wide4=0)


# ---- four waves per instance
def test_four_waves_soft_rows(harness):
    # N = 20: reach = cap = 256
    p, = plans(harness, "N=20 B=256 k_soft=1 K=8")
    check(p, slot="wide_lds4", grid=256, block=256, lds=87680, ngroups=256, q0=-1, rows=1, mapping=4, **NO_HAND)
    assert p["probes"] == "wide_lds4:256:87680"
    p, = plans(harness, "N=20 B=257 k_soft=1 K=8")      # one wave: 257 <= 2 * 512
    check(p, slot="wide_lds1", grid=257, q0=-1, mapping=1)
    # N = 40 with the queue: reach = 2 * 256
    p, = plans(harness, "N=40 B=512 k_soft=1 K=8")
    check(p, slot="wide_lds4", grid=256, block=256, lds=159360, ngroups=256, q0=256, mapping=4)
    p, = plans(harness, "N=40 B=513 k_soft=1 K=8")      # one wave at N = 40: cap 256, 513 > 512
    check(p, mapping=0, slot="qp_aux")
    p, = plans(harness, "N=40 B=257 k_soft=1 K=8 dynamic_rows=0")   # without the queue the reach is one cap
    check(p, mapping=1, slot="wide_lds1", grid=257, q0=-1)
    # two obstacle chunks of hard rows count like soft rows
    p, = plans(harness, "N=20 B=256 k_kch=2 kch=2 K=20")
    check(p, slot="wide_lds4", mapping=4)


def test_four_waves_many_hard_rows(harness):
    # one chunk of hard rows: K >= 8 and N >= 40, up to ONE instance per CU (B <= cap, not the reach of 512)
    p, = plans(harness, "N=40 B=256 K=8")
    check(p, slot="wide_lds4", grid=256, q0=-1, mapping=4)
    p, = plans(harness, "N=40 B=257 K=8")
    check(p, slot="wide_lds1", mapping=1)
    p, = plans(harness, "N=40 B=256 K=7")
    check(p, slot="wide_lds1", mapping=1)
    p, = plans(harness, "N=20 B=256 K=8")
    check(p, slot="wide_lds1", mapping=1)


def test_four_waves_option(harness):
    # wide_waves = 1: never four, not probed
    p, = plans(harness, "N=20 B=64 k_soft=1 K=8 wide_waves=1")
    check(p, slot="wide_lds1", mapping=1, cap_wide4=0)
    assert p["probes"] == "wide_lds1:64:78336"
    # wide = 1, wide_waves = 4: hard rows with K = 3 too, at any batch size
    p, = plans(harness, "N=20 B=64 wide=1 wide_waves=4")
    check(p, slot="wide_lds4", grid=64, q0=-1, mapping=4)
    p, = plans(harness, "N=20 B=1000 wide=1 wide_waves=4")
    check(p, slot="wide_lds4", grid=256, ngroups=256, q0=256, mapping=4)
    # a full SQP launch never
    p, = plans(harness, "N=20 B=64 k_soft=1 K=8 phase=1")
    check(p, slot="wide_hbm1", mapping=1, cap_wide4=0)


# ---- max_waves counts wavefronts
def test_max_waves_four_wave_mapping(harness):
    # 8 waves = 2 workgroups of four
    p, = plans(harness, "N=20 B=10 k_soft=1 K=8 wide_waves=4 max_waves=8")
    check(p, slot="wide_lds4", grid=2, ngroups=2, q0=2, mapping=4, cap_wide4=256)
    p, = plans(harness, "N=20 B=2 k_soft=1 K=8 max_waves=8")
    check(p, slot="wide_lds4", grid=2, q0=-1, mapping=4)
    p, = plans(harness, "N=20 B=3 k_soft=1 K=8 max_waves=8")        # reach 2; one wave: cap min(512, 8), 3 <= 16
    check(p, slot="wide_lds1", grid=3, q0=-1, mapping=1, cap_wide=8)
    # floor of one workgroup: 2 // 4 = 0 -> 1
    p, = plans(harness, "N=20 B=1 k_soft=1 K=8 max_waves=2")
    check(p, slot="wide_lds4", grid=1, q0=-1, mapping=4)
    p, = plans(harness, "N=20 B=5 k_soft=1 K=8 wide_waves=4 max_waves=2")
    check(p, slot="wide_lds4", grid=1, ngroups=1, q0=1, mapping=4)


def test_max_waves_one_wave_mapping(harness):
    p, = plans(harness, "N=20 B=16 max_waves=8")
    check(p, slot="wide_lds1", grid=8, ngroups=8, q0=8, mapping=1, cap_wide=8)
    p, = plans(harness, "N=20 B=17 max_waves=8")
    check(p, mapping=0)


def test_max_waves_throughput_mapping(harness):
    # 8 waves of four groups: 32 < 2048; the cap itself stays what the device holds
    p, = plans(harness, "N=40 B=65536 max_waves=8")
    check(p, slot="qp_aux", grid=8, ngroups=32, q0=32, rows=4, mapping=0, cap_qp=2048, cap_aux=2048)
    # the one-wave mapping over planes in HBM is capped like the one in LDS: N = 100, min(1024, 8), reach 16
    p, = plans(harness, "N=100 B=16 max_waves=8")
    check(p, slot="wide_hbm1", grid=8, q0=8, cap_wide_hbm=8)


# ---- a horizon whose planes do not fit LDS (N = 100)
def test_long_horizon_four_waves_over_hbm(harness):
    # the HBM kernel is asked only after the LDS kernel said 0; a -1 is not asked again
    p, q = plans(harness, "N=100 B=256 k_soft=1 K=8 plan plan")
    check(p, slot="wide_hbm4", grid=256, block=256, lds=20608, ngroups=256, q0=-1, rows=1, mapping=4, cap_wide4=-1, cap_wide4_hbm=256)
    assert p["probes"] == "wide_lds4:256:374400,wide_hbm4:256:20608"
    check(q, slot="wide_hbm4", grid=256, mapping=4, cap_wide4=-1, probes="")
    p, = plans(harness, "N=100 B=512 k_soft=1 K=8")     # reach 2 * 256 with the queue
    check(p, slot="wide_hbm4", grid=256, q0=256, mapping=4)
    p, = plans(harness, "N=20 B=256 k_soft=1 K=8")      # ... and never asked when the LDS kernel fits
    check(p, cap_wide4_hbm=0)


def test_long_horizon_window_of_16_stages(harness):
    # 16 stages * Bp * 36 * 128 bytes against 2^32: Bp = 58252 -> 4294803456 (below), 58256 -> 4295098368 (reached): -1 without a probe,
    # on to one wave per instance over HBM (its window has 4 stages: 1073774592)
    p, = plans(harness, "N=100 B=256 Bp=58252 k_soft=1 K=8")
    check(p, slot="wide_hbm4", mapping=4)
    p, = plans(harness, "N=100 B=256 Bp=58256 k_soft=1 K=8")
    check(p, slot="wide_hbm1", grid=256, block=64, lds=5120, ngroups=256, q0=-1, rows=1, mapping=1, cap_wide4=-1, cap_wide4_hbm=-1, cap_wide=-1, cap_wide_hbm=1024)
    assert p["probes"] == "wide_lds4:256:374400,wide_lds1:64:365056,wide_hbm1:64:5120"


def test_long_horizon_window_of_4_stages(harness):
    # 4 stages * Bp * 36 * 128: Bp = 233016 -> 4294950912 (below), 233020 -> 4295024640 (reached): throughput mapping, and no hand-over
    # (the follow-up kernels address the same window)
    p, = plans(harness, "N=100 B=256 Bp=233016")
    check(p, slot="wide_hbm1", mapping=1)
    p, = plans(harness, "N=100 B=256 Bp=233020 handover_iter=30")
    check(p, mapping=0, ngroups=2048, q0=2048, hand_ready=0, cap_wide_hbm=0, cap_resume=0, **NO_HAND)


def test_long_horizon_one_wave_over_hbm(harness):
    # hard rows, K = 3: four waves probed (LDS 0, HBM 256) and not taken; one wave: LDS -1, HBM 1024, with the queue up to 2048
    p, = plans(harness, "N=100 B=2048")
    check(p, slot="wide_hbm1", grid=1024, lds=5120, ngroups=1024, q0=1024, rows=1, mapping=1, cap_wide=-1, cap_wide_hbm=1024, **NO_HAND)
    assert p["probes"] == "wide_lds4:256:374400,wide_hbm4:256:20608,wide_lds1:64:365056,wide_hbm1:64:5120"
    # beyond: throughput mapping (aux(100) = 32320: 6860 + 32320 -> 4 -> min(2, 4): taken); the follow-up kernel over HBM only: no default hand-over
    p, = plans(harness, "N=100 B=2049")
    check(p, slot="qp_aux", lds=32320, ngroups=2048, q0=2048, mapping=0, hand_ready=1, cap_resume=1024, cap_resume_lds=0, **NO_HAND)
    assert p["probes"].endswith("resume_lds:64:365056,resume:64:5120")
    # without the queue once
    p, = plans(harness, "N=100 B=1025 dynamic_rows=0")
    check(p, slot="qp", mapping=0, ngroups=1028, q0=-1)


# ---- the launches of a full SQP
@pytest.mark.parametrize("phase", [1, 2])
def test_full_sqp(harness, phase):
    # up to ONE cap of the one-wave kernel over HBM (1024), one group per workgroup, no queue; no LDS-plane kernel is even probed
    p, = plans(harness, "N=20 B=1024 phase=%d" % phase)
    check(p, slot="wide_hbm1", grid=1024, block=64, lds=5120, ngroups=1024, q0=-1, rows=1, mapping=1, cap_wide=0, cap_wide4=0, **NO_HAND)
    assert p["probes"] == "wide_hbm1:64:5120"
    # above: plain qp over every group, no queue, no aux bytes, no hand-over; qp_cap not asked
    p, = plans(harness, "N=20 B=1025 phase=%d handover_iter=30" % phase)
    check(p, slot="qp", grid=257, block=64, lds=0, ngroups=1028, q0=-1, rows=4, mapping=0, hand_ready=0, cap_qp=0, cap_aux=0, cap_lds=0, cap_resume=0, **NO_HAND)
    assert p["probes"] == "wide_hbm1:64:5120,static:qp_lds"
    # the workspace-in-LDS kernel neither, even when forced
    p, = plans(harness, "N=10 B=64 wide=0 lds_workspace=1 phase=%d" % phase)
    check(p, slot="qp", ngroups=64, q0=-1, cap_lds=0)


# ---- the workspace in LDS (wide = 0; N = 10: rows_lds = 163840 // 50688 = 3)
def test_lds_workspace_one_round(harness):
    # B = 3 * 256: 256 workgroups of three rows; 3 * 50688 bytes -> one workgroup per CU -> cap 256
    p, = plans(harness, "N=10 B=768 wide=0")
    check(p, slot="qp_lds", grid=256, block=64, lds=152064, ngroups=768, q0=-1, rows=3, mapping=0, cap_lds=256, cap_lds_static=0, **NO_HAND)
    assert p["probes"] == "static:qp_lds,qp_lds:64:152064"
    p, = plans(harness, "N=10 B=766 wide=0")            # ceil(766 / 3) = 256 workgroups, the last one with a row to spare
    check(p, slot="qp_lds", grid=256, ngroups=768, rows=3)
    p, = plans(harness, "N=10 B=769 wide=0")            # one more: throughput mapping (aux(10): 6860 + 3520 -> 2: taken)
    check(p, slot="qp_aux", lds=3520, ngroups=772, q0=-1, rows=4, cap_lds=0)


def test_lds_workspace_forced(harness):
    # lds_workspace = 1, B = 4096: ceil(4096 / 3) = 1366 > 256 -> 256 workgroups, the queue starts behind their 768 groups
    p, = plans(harness, "N=10 B=4096 wide=0 lds_workspace=1")
    check(p, slot="qp_lds", grid=256, lds=152064, ngroups=768, q0=768, rows=3)
    p, = plans(harness, "N=10 B=4096 wide=0 lds_workspace=1 dynamic_rows=0")
    check(p, slot="qp_lds", grid=1366, ngroups=4098, q0=-1, rows=3)
    p, = plans(harness, "N=10 B=64 wide=0 lds_workspace=0")
    check(p, slot="qp_aux", cap_lds=0)
    # a horizon of which not one instance fits (N = 40: 188928 bytes)
    p, = plans(harness, "N=40 B=64 wide=0 lds_workspace=1")
    check(p, slot="qp_aux", cap_lds=0)


def test_lds_workspace_shrinks_with_static_lds(harness):
    # 16384 bytes static: (163840 - 16384) // 50688 = 2 rows, 101376 bytes dynamic; one round is 2 * 256
    p, = plans(harness, "N=10 B=512 wide=0 st_qp_lds=16384")
    check(p, slot="qp_lds", grid=256, lds=101376, ngroups=512, q0=-1, rows=2, cap_lds=256, cap_lds_static=16384)
    assert p["probes"] == "static:qp_lds,qp_lds:64:101376"
    p, = plans(harness, "N=10 B=513 wide=0 st_qp_lds=16384")
    check(p, slot="qp_aux", cap_lds=0)


# ---- a table with nothing but the plain kernel
ONLY_QP = " ".join("has_%s=0" % s for s in ("qp_lds", "qp_aux", "wide_lds1", "wide_hbm1", "wide_lds4", "wide_hbm4", "resume", "resume_lds", "resume_co"))


@pytest.mark.parametrize("opts", ["", "wide=1 wide_waves=4", "lds_workspace=1", "handover_iter=30", "N=100", "k_soft=1 K=8"])
def test_table_with_only_qp(harness, opts):
    p, = plans(harness, "N=20", opts, "B=65536", ONLY_QP)
    check(p, slot="qp", grid=512, block=64, lds=0, ngroups=2048, q0=2048, rows=4, mapping=0, hand_ready=0, **NO_HAND)
    assert p["probes"] == "qp:64:0"
    p, = plans(harness, "N=20", opts, "B=64", ONLY_QP)
    check(p, slot="qp", grid=16, lds=0, ngroups=64, q0=-1, rows=4, mapping=0, **NO_HAND)


# ---- the queries are made once
def test_caps_are_asked_once_and_again_after_reset(harness):
    p, q, r = plans(harness, "N=40 B=65536 plan plan reset plan")
    assert p["probes"] == THROUGHPUT_PROBES and q["probes"] == "" and r["probes"] == THROUGHPUT_PROBES
    for k in p:
        if k != "probes":
            assert p[k] == q[k] == r[k], k
    # another batch size on the same handle asks only what the first did not need: here nothing
    p, q = plans(harness, "N=40 B=65536 plan B=6144 plan")
    check(q, hand=1, hand_iter=20, probes="")
    # ... and here the throughput kernels, after a tick that stayed on the one-wave mapping
    p, q = plans(harness, "N=20 B=64 plan B=4096 plan")
    check(q, slot="qp_aux", mapping=0, probes="static:qp_lds,qp:64:0,qp_aux:64:6720,resume_lds:64:78336")
