"""csrc/lin_order.hpp, the work order of the pipelined lineariser, compiled with the host compiler (CPU only): every (group, stage) of
the grid exactly once, padded groups on the last map entry, for identity and permuted maps."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_collisionavoidance_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lin_order") / "lin_order_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "lin_order_harness.cpp")])
    return exe


# (B, Bp, N): batches that fill their last wave and batches that do not (Bp: B rounded up to the QP kernel's four rows - or further),
# a single instance, a one-stage horizon
SHAPES = [(1, 4, 1), (4, 4, 3), (5, 8, 1), (13, 16, 20), (64, 64, 40), (1001, 1004, 40), (1023, 1024, 7), (16385, 16388, 40), (30, 48, 5)]


@pytest.mark.parametrize("B,Bp,N", SHAPES)
@pytest.mark.parametrize("maps", [0, 1, 2, 3], ids=["identity", "cur-permuted", "next-permuted", "both-permuted"])
def test_every_group_stage_once(harness, B, Bp, N, maps):
    r = subprocess.run([harness, str(B), str(Bp), str(N), str(17 + B + maps), str(maps)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok %d" % (Bp * (N + 1))
