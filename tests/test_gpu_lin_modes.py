"""The pipelined lineariser's two kernels against the whole-batch one, on the device (option "lin_force_modes").

No accessor of the library reaches the workspace planes the lineariser writes (P_GQ, P_RB0, P_MAT..: usvmpc_get_device_ptr hands out the
caller-visible arrays only), so the three paths are compared through what the QP launch makes of those planes: it reads every one of them,
and iterates, multipliers, statuses and iteration counts of every tick must be equal to the bit.  The kernel bodies themselves are compared
plane by plane on the lane emulator (tests/test_emu_kernels.py)."""
import numpy as np
import pytest

from mpc_collisionavoidance_amd import BatchOcpSolver, scenario, usv_models

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,N,K,B", [("usv_model_pf_ca", 20, 4, 1003), ("usv_model_guidance_ca1", 10, 3, 2049), ("usv_model_pf_ca", 40, 10, 517)])
def test_forced_modes_equal_the_whole_batch_lineariser(name, N, K, B):
    """B is not a multiple of 16 (the last wave of the grid is partly padded groups, which replay the last map entry), and from the second
    tick on the group -> instance map is the counting sort of the previous tick's iteration counts: not the identity.
    Path 0: MODE 0.  Path 1: the speculative kernel in the retire order (MODE 3) with every epoch final (+ a fix-up pass that finds
    nothing).  Path 2: the same with no epoch final - every (instance, stage) marked - followed by the fix-up by groups (MODE 4)."""
    assert B % 16 != 0
    wl = scenario.make_bench_batch(name, N, K, B, seed=11)
    ocp = usv_models.make_ocp(name, N * scenario.BENCH_DT, N, K)
    ocp.solver_options.sim_method_num_steps = scenario.BENCH_SIM_STEPS[name]

    def run(mode):
        s = BatchOcpSolver(ocp, B)
        scenario.load_into(s, wl)
        s.set_option("static_obstacles", 1)
        s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
        s.set_option("lin_force_modes", mode)
        out = []
        for t in range(4):
            s.solve_async()
            s.advance(1e-3, seed=70 + t)
            s.sync()
            out.append([s.get_all("x"), s.get_all("u"), s.get_all("pi"), s.get_int("status").copy(), s.get_int("qp_status").copy(),
                        s.get_int("qp_iter").copy(), s.get("x0", 0)])
        s.close()
        return out

    ref = run(0)
    it0 = ref[0][5]
    assert np.any(np.diff(it0) > 0), "the iteration counts of tick 0 are already in queue order: the next map would be the identity"
    assert (ref[-1][3] == 0).mean() > 0.9
    for mode in (1, 2):
        got = run(mode)
        for t, (a, b) in enumerate(zip(ref, got)):
            for i, (p, q) in enumerate(zip(a, b)):
                assert np.array_equal(p, q), (mode, t, i)


def test_pipeline_in_retire_order_is_scheduling_only():
    """The pipeline itself with the kernels of the retire order: a launch that hands nothing over takes them (here: hand-over switched
    off at a size that would use it; the headline size takes them by default).  Tick by tick against the un-pipelined sequence."""
    name, N, K, B = "usv_model_pf_ca", 20, 4, 16384 + 7
    wl = scenario.make_bench_batch(name, N, K, B, seed=5)
    ocp = usv_models.make_ocp(name, N * scenario.BENCH_DT, N, K)
    ocp.solver_options.sim_method_num_steps = scenario.BENCH_SIM_STEPS[name]

    def run(pipe):
        s = BatchOcpSolver(ocp, B)
        scenario.load_into(s, wl)
        s.set_option("static_obstacles", 1)
        s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
        s.set_option("handover_iter", 0)
        s.set_option("pipeline_linearize", pipe)
        out = []
        for t in range(10):
            s.solve_async()
            s.advance(1e-3, seed=50 + t)
            if t % 3 == 0 or t >= 8:
                s.sync()
                out += [s.get_all("x"), s.get_all("u"), s.get_int("status").copy(), s.get_int("qp_iter").copy(), s.get("x0", 0)]
        used = s.pipeline_stats()[0]
        s.close()
        return out, used

    (a, used), (b, _) = run(1), run(0)
    assert used >= 7  # (the lineariser runs ahead from the second solve on)
    for i, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p, q), i


def test_forced_modes_option_is_checked():
    name, N, K = "usv_model_pf_ca", 10, 2
    ocp = usv_models.make_ocp(name, N * scenario.BENCH_DT, N, K)
    s = BatchOcpSolver(ocp, 8)
    with pytest.raises(Exception):
        s.set_option("lin_force_modes", 3)
    s.close()
