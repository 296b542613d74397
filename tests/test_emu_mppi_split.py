"""CPU suite: the split-sample MPPI kernels of dart_planner_amd/csrc/mppi_split.hip (one problem's samples over several workgroups, one
launch per iteration), compiled for the host by tests/emu and driven through the C ABI, Ops and the planner, against the NumPy oracle
of tests/mppi_oracle.py and against se3mpc_mppi_*.  The smaller shapes of tests/test_gpu_mppi_split.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402
from numpy_backend import NumpyBackend  # noqa: E402

from dart_planner_amd import capi  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402
import mppi_split_checks as sc  # noqa: E402
import parity_checks as pc  # noqa: E402

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(NumpyBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    return pc.Harness(ops, lambda a: a, lambda a: a, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,splits,nprob,K", [(6, 64, 1, 2, 0), (6, 256, 4, 2, 3), (6, 320, 5, 2, 0), (30, 256, 4, 1, 3), (6, 640, 2, 1, 0)])
def test_against_oracle(emu_ops, dt, N, S, splits, nprob, K):
    sc.check_against_oracle(harness(emu_ops, dt), N, S, splits, nprob, (3, 1, 0), K=K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,K", [(6, 64, 2), (6, 320, 0), (30, 64, 0)])
def test_one_split_is_the_unsplit_kernel(emu_ops, dt, N, S, K):
    sc.check_one_split_is_the_unsplit_kernel(harness(emu_ops, dt), N, S, 2, iters=2, K=K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,splits,K", [(6, 256, 4, 0), (6, 320, 5, 2), (6, 640, 2, 0), (30, 128, 2, 0)])
def test_one_iteration_any_split_against_the_unsplit_kernel(emu_ops, dt, N, S, splits, K):
    sc.check_one_iteration_any_split(harness(emu_ops, dt), N, S, splits, 2, K=K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("S,splits,K", [(128, 2, 0), (192, 3, 2)])
def test_iteration_chunks_problem_slices_and_run_to_run(emu_ops, dt, S, splits, K):
    sc.check_chunking_and_slices(harness(emu_ops, dt), 6, S, splits, 3, iters=2, K=K)


@pytest.mark.parametrize("dt", DTYPES)
def test_temperature_limits(emu_ops, dt):
    winners = []
    for N, S, splits in [(6, 256, 4), (6, 384, 2)]:
        winners += sc.check_limits(harness(emu_ops, dt), N, S, splits, 2, iters=2)
    sc.assert_winners_spread(winners)


@pytest.mark.parametrize("dt", DTYPES)
def test_nan_costs_weigh_nothing(emu_ops, dt):
    sc.check_nan_costs_weigh_nothing(harness(emu_ops, dt), 6, 128, 2)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(emu_ops, dt):
    sc.check_invalid_arguments(harness(emu_ops, dt))


def _planner(N=6, dt=0.1):
    from numpy_backend import TorchCpuBackend
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=N))
    pl.se3_config = SE3MPCConfig(**{**pl.se3_config.__dict__, "dt": dt})
    pl._ops = Ops(TorchCpuBackend(), capi.Library(build_emu.build()))
    return pl


def test_auto_splits_rule():
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCPlanner as P
    assert P._mppi_splits(None, 1024) is None and P._mppi_splits(4, 1024) == 4
    assert [P._mppi_splits("auto", S) for S in (64, 256, 320, 1024, 4096, 16384)] == [None, None, None, 4, 16, 64]
    assert P._mppi_splits("auto", 832) is None and P._mppi_splits("auto", 768) == 3            # 832 = 13 x 64: no split count above 1 divides it
    assert [P._mppi_splits("auto", 1024, B) for B in (1, 16, 256, 512, 4096)] == [4, 4, 4, 2, None]                  # one split left: the one-launch path
    with pytest.raises(ValueError):
        P._mppi_splits("many", 1024)


def test_plan_mppi_split_warm_start_and_one_split():
    """The planner's eager path on the emulated library: splits = 1 is plan_mppi() bit for bit, a split plan warm-starts from exactly
    the shifted nominal and advances the iteration counter as the unsplit one does."""
    from dart_planner_amd.common.types import DroneState
    st = DroneState(timestamp=0.0, position=np.array([0.0, 0.0, 2.0]), velocity=np.zeros(3))
    goal = np.array([3.0, 1.0, 2.0])
    kw = dict(n_samples=256, iters=2, sigma=2.0, temperature=50.0, seed=1, precision="f64")
    a, b = _planner(), _planner()
    for _ in range(2):                                                                  # cold, then warm-started
        ta, tb = a.plan_mppi(st, goal, **kw), b.plan_mppi(st, goal, splits=1, **kw)
        assert np.array_equal(ta.positions, tb.positions) and np.array_equal(a.last_result["U"], b.last_result["U"])
        assert a.last_result["cost"] == b.last_result["cost"] and np.array_equal(a.last_result["trace"], b.last_result["trace"])
        assert (a.last_result["splits"], b.last_result["splits"]) == (None, 1)
    pl = _planner()
    pl.plan_mppi(st, goal, splits=4, **kw)
    r1 = dict(pl.last_result)
    assert r1["shift"] == 0 and r1["iter_base"] == 0 and r1["splits"] == 4 and len(r1["trace"]) == 2
    want = np.concatenate([r1["U"][1:], [[0.0, 0.0, pl.hover_thrust]]])
    assert pl._mppi_nominal(6, True)[0].tolist() == want.tolist()
    pl.plan_mppi(st, goal, splits=4, **kw)
    r2 = dict(pl.last_result)
    assert r2["shift"] == 1 and r2["iter_base"] == 2
    ops, prm = pl._ops, pl._params()
    col = lambda x: ops.be.from_host(np.asarray(x, float).reshape(-1, 1).copy())
    o = ops.mppi_split(prm, col(st.position), col(st.velocity), col(pl.goal_position), col(want), 256, 2, 2.0, 50.0, 4, seed=1, iter_base=2)
    assert np.array_equal(ops.be.to_host(o["U"])[:, 0].reshape(6, 3), r2["U"])
    assert np.max(np.abs(r2["U"] - a.last_result["U"])) <= sc.F64_REL * 25, "the split plan is the unsplit plan up to summation order"
    pl.plan_mppi(st, np.array([-3.0, 1.0, 2.0]), splits="auto", **kw)
    assert pl.last_result["shift"] == 0 and pl.last_result["splits"] is None, "a new goal resets the nominal; auto at 256 samples is the one-launch path"


def test_plan_batch_mppi_split_rows_are_single_problems():
    pl = _planner()
    rng = np.random.default_rng(2)
    B = 3
    pos, vel, goals = rng.uniform(-1, 1, (B, 3)) + [0, 0, 2], rng.uniform(-1, 1, (B, 3)), rng.uniform(-3, 3, (B, 3)) + [0, 0, 2]
    res = pl.plan_batch_mppi(pos, vel, goals, n_samples=128, iters=2, sigma=2.0, temperature=50.0, seed=4, precision="f64", splits=2)
    assert res["positions"].shape == (B, 6, 3) and res["trace"].shape == (B, 2)
    ops, prm = pl._ops, pl._params(has_goal=1)
    col = lambda a: ops.be.from_host(np.asarray(a, float).reshape(-1, 1).copy())
    for b in range(B):
        o = ops.mppi_split(prm, col(pos[b]), col(vel[b]), col(goals[b]), col(np.tile([0.0, 0.0, pl.hover_thrust], (6, 1))), 128, 2, 2.0, 50.0, 2,
                           seed=4, index_base=b)
        assert np.array_equal(ops.be.to_host(o["U"])[:, 0].reshape(6, 3), res["thrust_vectors"][b])
        assert ops.be.to_host(o["cost"])[0] == res["cost"][b]
        assert np.array_equal(ops.be.to_host(o["trace"])[:, 0], res["trace"][b])
