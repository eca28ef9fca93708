"""The paired lineariser on the device (option "lin_pairs": two (instance, stage) pairs per 16-lane row) against the 16-lane kernels of the
same library.

As in tests/test_gpu_lin_modes.py the lineariser's planes are compared through what the QP launch makes of them - it reads every one -:
iterates, multipliers, statuses, iteration counts and x0 of every closed-loop tick must be equal to the bit.  The kernel bodies are compared
plane by plane on the lane emulator (tests/test_lin_pairs_emu.py)."""
import numpy as np
import pytest

from mpc_collisionavoidance_amd import BatchOcpSolver, scenario, usv_models

pytestmark = pytest.mark.gpu


def _closed_loop(name, N, K, B, steps, ticks, seed, **options):
    wl = scenario.make_bench_batch(name, N, K, B, seed=seed)
    ocp = usv_models.make_ocp(name, N * scenario.BENCH_DT, N, K if name != "usv_model" else None)
    ocp.solver_options.sim_method_num_steps = steps
    s = BatchOcpSolver(ocp, B)
    scenario.load_into(s, wl)
    if K:
        s.set_option("static_obstacles", 1)
    s.set_option("disturbance_mask", scenario.NOISE_MASK[name])
    for key, value in options.items():
        s.set_option(key, value)
    out = []
    for t in range(ticks):
        s.solve_async()
        s.advance(1e-3, seed=90 + t)
        s.sync()
        out.append([s.get_all("x"), s.get_all("u"), s.get_all("pi"), s.get_int("status").copy(), s.get_int("qp_status").copy(),
                    s.get_int("qp_iter").copy(), s.get("x0", 0)])
    used = s.pipeline_stats()[0]
    # which kernels ran: every lineariser launch of a handle with lin_pairs 1 is a paired one, none of a handle with 0
    pair_launches = s.lin_pair_launches()
    assert (pair_launches >= ticks) if options.get("lin_pairs", 1) else (pair_launches == 0), pair_launches
    s.close()
    return out, used


def _assert_equal(ref, got, what):
    for t, (a, b) in enumerate(zip(ref, got)):
        for i, (p, q) in enumerate(zip(a, b)):
            assert np.array_equal(p, q), (what, t, i)


# B = 37: the stage-major grid ends inside a workgroup, the retire order's last wave is padding; N = 5: six stages, N = 20: twenty-one - the last
# row of an instance in the retire order has a lone half; B = 1003: many workgroups, Bp - B = 1 padded group
SHAPES = [("usv_model_pf_ca", 5, 2, 37), ("usv_model_pf_ca", 20, 4, 1003)]


@pytest.mark.parametrize("name,N,K,B", SHAPES)
@pytest.mark.parametrize("steps", ["bench", 1])
def test_pairs_equal_the_16_lane_kernels(name, N, K, B, steps):
    """lin_pairs 1 against 0 for lin_force_modes 0 (the whole-batch kernel), 1 (retire order with every instance final + a fix-up that finds
    nothing) and 2 (nothing final: everything marked, the fix-up by groups does it all); from the second tick on the group -> instance map is
    a counting sort, not the identity."""
    steps = scenario.BENCH_SIM_STEPS[name] if steps == "bench" else steps
    for force in (0, 1, 2):
        ref, _ = _closed_loop(name, N, K, B, steps, 4, seed=11, lin_force_modes=force, lin_pairs=0)
        got, _ = _closed_loop(name, N, K, B, steps, 4, seed=11, lin_force_modes=force, lin_pairs=1)
        if force == 0:
            assert np.any(np.diff(ref[0][5]) > 0), "the next tick's map would be the identity"
            assert (ref[-1][3] == 0).mean() > 0.9
        _assert_equal(ref, got, force)


def test_pairs_in_the_pipeline():
    """The pipelined lineariser (speculative pass in the retire order beside the running QP launch + fix-up by groups) with the paired kernels
    against the 16-lane ones, tick by tick."""
    name, N, K, B = "usv_model_pf_ca", 6, 2, 16384 + 7
    steps = scenario.BENCH_SIM_STEPS[name]
    ref, used0 = _closed_loop(name, N, K, B, steps, 6, seed=5, handover_iter=0, lin_pairs=0)
    got, used1 = _closed_loop(name, N, K, B, steps, 6, seed=5, handover_iter=0, lin_pairs=1)
    assert used0 >= 4 and used1 >= 4  # (the lineariser runs ahead from the second solve on)
    _assert_equal(ref, got, "pipeline")


def test_pairs_three_dof_model():
    """usv_model (seven columns, no quadrature entry, one RK4 step) through the same table."""
    name, N, K, B = "usv_model", 5, 0, 37
    steps = scenario.BENCH_SIM_STEPS[name]
    for force in (0, 2):
        ref, _ = _closed_loop(name, N, K, B, steps, 4, seed=11, lin_force_modes=force, lin_pairs=0)
        got, _ = _closed_loop(name, N, K, B, steps, 4, seed=11, lin_force_modes=force, lin_pairs=1)
        _assert_equal(ref, got, force)


def test_pairs_is_the_default_and_checked():
    name, N, K = "usv_model_pf_ca", 10, 2
    ocp = usv_models.make_ocp(name, N * scenario.BENCH_DT, N, K)
    s = BatchOcpSolver(ocp, 8)
    scenario.load_into(s, scenario.make_bench_batch(name, N, K, 8, seed=3))
    s.solve()
    assert s.lin_pair_launches() == 1  # (the default: nothing was set)
    with pytest.raises(Exception):
        s.set_option("lin_pairs", 2)
    s.set_option("lin_pairs", 0)
    s.set_option("lin_pairs", 1)
    s.close()
    # a generated model declares no columns: one pair per row, and asking for two is an error
    gocp = usv_models.make_ocp("usv_model_guidance_ca1", 1.0, 20, 8, symbolic=True)
    g = BatchOcpSolver(gocp, 8)
    with pytest.raises(Exception, match="lin_pairs"):
        g.set_option("lin_pairs", 1)
    g.set_option("lin_pairs", 0)
    scenario.load_into(g, scenario.make_bench_batch("usv_model_guidance_ca1", 20, 8, 8, seed=3))
    g.solve()
    assert g.lin_pair_launches() == 0
    g.close()
