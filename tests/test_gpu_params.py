"""GPU suite (`-m gpu`), off the reference's default parameters: the plan-path kernels of libse3mpc.so on an MI355X at the parameter sets
of tests/param_sets.py (no two fields equal, so a kernel that reads one constant where another belongs shows), against the oracle; and
the solver's limits (max_corrections, max_linesearch, max_fun) at valid non-default values against SciPy."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mppi_checks as mc  # noqa: E402
import mppi_moving_checks as mv  # noqa: E402
import mppi_split_checks as sc  # noqa: E402
import param_sets as ps  # noqa: E402
import parity_checks as pc  # noqa: E402


@pytest.fixture(scope="module")
def gpu_ops():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend("cuda:0"))
    assert ops.lib.device_count() >= 1, "no gfx950 device visible to libse3mpc"
    assert os.path.basename(ops.lib.path) == "libse3mpc.so"
    return ops


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"),
                      lambda a: a.detach().cpu().numpy(), dt)


@pytest.fixture(scope="module")
def golden_params():
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return np.load(os.path.join(g, "param_cases.npz")), json.load(open(os.path.join(g, "param_cases.json")))

SETS_AB = ["A", "B"]
DTYPES = [np.float64, np.float32]
ALL_VARIANTS = (0, 1, 2, 3, 4, 5, 6)


# ------------------------------------------------------------------ lane kernels and rollout
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,N,B", [(s, N, B) for s in SETS_AB for N, B in ((6, 70), (7, 9), (30, 66), (33, 65))] + [("C", 6, 70), ("C", 7, 9)])
def test_lane_kernels(gpu_ops, dt, name, N, B):
    # (6, 70): the exact-N register kernels, every rollout variant; (7, 9): the generic path; (30, 66): f64 through memory; (33, 65): the bucket past 32
    pc.check_lane_kernels(harness(gpu_ops, dt), N, B, seed=N, variants=ALL_VARIANTS if (N, B) == (6, 70) else (0,), params=ps.overrides(name))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,N,B", [(s, N, B) for s in SETS_AB for N, B in ((6, 70), (30, 66), (7, 9))] + [("C", 6, 70)])
def test_rollout_iterate(gpu_ops, dt, name, N, B):
    pc.check_rollout_iterate(harness(gpu_ops, dt), N, B, seed=N, iters=4, step=ps.iterate_step(name, N), params=ps.overrides(name))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,N,B", [(s, N, B) for s in SETS_AB for N, B in ((6, 70), (30, 66), (7, 9))] + [("C", 6, 70)])
def test_rollout_iterate_obstacles(gpu_ops, dt, name, N, B):
    it = ps.ITERATE[name]
    pc.check_rollout_iterate_obstacles(harness(gpu_ops, dt), N, B, seed=N, iters=3, step=it["obstacle_step"], w_obs=it["obstacle_weight"],
                                       params=ps.overrides(name))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", SETS_AB)
def test_shooting_finish_and_iterate_keys(gpu_ops, dt, name):
    it = ps.ITERATE[name]
    pc.check_shooting_finish(harness(gpu_ops, dt), 6, 70, seed=6, params=ps.overrides(name))
    pc.check_iterate_keys(harness(gpu_ops, dt), 6, 70, seed=1, step=it["obstacle_step"], w_obs=it["obstacle_weight"], params=ps.overrides(name))


# ------------------------------------------------------------------ MPPI
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", SETS_AB)
@pytest.mark.parametrize("N,S,nprob,iters,K", [(6, 64, 3, 2, 0), (6, 128, 2, 2, 3), (30, 64, 1, 2, 4)])
def test_mppi_against_oracle(gpu_ops, dt, name, N, S, nprob, iters, K):
    mc.check_against_oracle(harness(gpu_ops, dt), N, S, nprob, iters, K=K, seed=ps.MPPI_SEED, params=ps.overrides(name))


@pytest.mark.parametrize("dt", DTYPES)
def test_mppi_limits(gpu_ops, dt):
    mc.check_limits(harness(gpu_ops, dt), 6, 64, 2, K=2, seed=ps.MPPI_SEED, params=ps.overrides("A"))


@pytest.mark.parametrize("dt", DTYPES)
def test_mppi_split_and_moving_against_their_oracles(gpu_ops, dt):
    sc.check_against_oracle(harness(gpu_ops, dt), 6, 256, 4, 2, (2, 0), K=3, seed=ps.MPPI_SEED, params=ps.overrides("A"))
    mv.check_against_oracle(harness(gpu_ops, dt), 6, 64, 3, 2, 3, params=ps.overrides("A"))


# ------------------------------------------------------------------ solver
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", SETS_AB)
@pytest.mark.parametrize("N,G", [(6, 8), (13, 16), (30, 32), (50, 64)])
def test_solver_vs_oracle(gpu_ops, dt, name, N, G):
    # the four group sizes, ragged last wavefronts as in test_solver_group_sizes
    B = 5 * (64 // G) + 3
    worst, mism = pc.check_solver_vs_oracle(harness(gpu_ops, dt), N, B, seed=N, group=G, **ps.overrides(name))
    print(f"set {name} N={N} group {G} {np.dtype(dt).name}: worst position error {worst:.3e} m, mismatch {mism:.3f}")
    assert mism <= pc.mismatch_budget(B, dt) and worst <= (1e-4 if dt == np.float32 else 1e-9)


@pytest.mark.parametrize("dt", DTYPES)
def test_solver_reproduces_reference_solves_at_the_sets(gpu_ops, golden_params, dt):
    data, meta = golden_params
    solves = dict(cases=[c for c in meta["cases"] if c["kind"] == "solve"])
    assert len(solves["cases"]) == 12
    knife = [c["key"] for c in solves["cases"] if pc.summation_order_outcomes(c, data, pc.params_case_params(c)) != {(c["nit"], c["nfev"], c["status"])}]
    assert knife == ["s08_"], knife               # one of the twelve hangs on the rounding of f (parity_checks.summation_order_outcomes)
    worst = pc.check_solver_golden(harness(gpu_ops, dt), data, solves, params_of=pc.params_case_params, either_summation_order=True)
    print(f"worst position error vs the reference at sets A and B ({np.dtype(dt).name}): {worst:.3e} m")
    assert worst <= (1e-4 if dt == np.float32 else 1e-9)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,G", [(6, None), (20, None), (30, None), (6, 64)])
@pytest.mark.parametrize("limits", pc.LIMIT_CASES, ids=lambda d: "-".join(f"{k[4:]}{v}" for k, v in d.items()))
def test_solver_limits(gpu_ops, dt, N, G, limits):
    worst, mism = pc.check_solver_limits(harness(gpu_ops, dt), N, limits, group=G)
    print(f"N={N} group {G} {limits} {np.dtype(dt).name}: worst position error {worst:.3e} m, mismatch fraction {mism:.3f}")


def test_solver_limits_closed_form_cauchy_point_against_the_published_search(gpu_ops):
    """max_corrections = 1 on parity_checks.random_batch's distribution at horizon 30: the memory is refreshed again and again, and every
    refresh takes the default solver through its closed-form generalized Cauchy point, whose last bits are not those of SciPy's
    accumulated breakpoint search.  A line search that fails at the end of a solve collapses its last trial points onto each other, and
    whether two of them are the same floating-point vector -- which SciPy does not count as an evaluation -- hangs on those bits: on the
    host-emulated build problem 14 ends at SciPy's point to 4e-13 m with (nit, nfev, status) = (15, 57, 2) against SciPy's (15, 58, 2).
    With the published search (se3mpc_set_solver_variant(1)) float64 must follow SciPy exactly; the default is held to
    check_solver_vs_oracle's unconditional rule and to SciPy's positions, and its mismatch count is printed."""
    h = harness(gpu_ops, np.float64)
    gpu_ops.lib.set_solver_variant(1)
    try:
        worst, mism = pc.check_solver_limits(h, 30, dict(max_corrections=1), kind="cfg2")
    finally:
        gpu_ops.lib.set_solver_variant(0)
    assert mism == 0.0 and worst <= 1e-8
    worst, mism = pc.check_solver_limits(h, 30, dict(max_corrections=1), kind="cfg2", exact=False)
    print(f"closed-form Cauchy point, max_corrections = 1, N = 30: {mism * 16:.0f} of 16 problems count differently from SciPy, worst {worst:.3e} m")
    assert worst <= 1e-8
