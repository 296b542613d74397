"""CPU suite: the MPPI kernels of dart_planner_amd/csrc/mppi.hip, compiled for the host by tests/emu and driven through the C ABI
and Ops, against the NumPy oracle of tests/mppi_oracle.py (Philox4x32-10, Box-Muller, the float64 update)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402
from numpy_backend import NumpyBackend  # noqa: E402

from dart_planner_amd import capi  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402
import mppi_checks as mc  # noqa: E402
import mppi_oracle as mo  # noqa: E402
import parity_checks as pc  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(NumpyBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    return pc.Harness(ops, lambda a: a, lambda a: a, dt)


def test_philox_known_answers():
    for ctr, key, want in mo.KNOWN_ANSWERS:
        assert [int(x) for x in mo.philox4x32_10(*ctr, *key)] == list(want)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N,S,nprob", [(6, 64, 3), (30, 128, 2)])
def test_noise_and_samples(emu_ops, dt, N, S, nprob):
    mc.check_noise(harness(emu_ops, dt), N, S, nprob)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N,S,nprob,iters,K", [(6, 64, 3, 3, 0), (6, 128, 2, 2, 3), (30, 64, 2, 2, 0), (30, 64, 1, 2, 4), (6, 320, 1, 2, 0)])
def test_against_oracle(emu_ops, dt, N, S, nprob, iters, K):
    mc.check_against_oracle(harness(emu_ops, dt), N, S, nprob, iters, K=K)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N,S,K", [(6, 64, 0), (6, 128, 2), (30, 64, 0), (6, 320, 0)])
def test_temperature_limits(emu_ops, dt, N, S, K):
    mc.check_limits(harness(emu_ops, dt), N, S, 2, iters=3, K=K)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_composed_iteration(emu_ops, dt):
    mc.check_composition(harness(emu_ops, dt), 6, 128)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("K", [0, 2])
def test_iteration_chunks_and_problem_slices(emu_ops, dt, K):
    mc.check_chunking_and_slices(harness(emu_ops, dt), 6, 64, 5, iters=3, K=K)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_invalid_arguments(emu_ops, dt):
    mc.check_invalid_arguments(harness(emu_ops, dt))


def _planner(N=6, dt=0.1):
    from numpy_backend import TorchCpuBackend
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=N))
    pl.se3_config = SE3MPCConfig(**{**pl.se3_config.__dict__, "dt": dt})
    pl._ops = Ops(TorchCpuBackend(), capi.Library(build_emu.build()))
    return pl


def test_plan_mppi_warm_start_and_goal_reset():
    """The planner's eager path on the emulated library: the second call starts from exactly the shifted nominal, a goal change resets it."""
    from dart_planner_amd.common.types import DroneState
    pl = _planner()
    st = DroneState(timestamp=0.0, position=np.array([0.0, 0.0, 2.0]), velocity=np.zeros(3))
    kw = dict(n_samples=64, iters=2, sigma=2.0, temperature=50.0, seed=1, precision="f64")
    tr = pl.plan_mppi(st, np.array([3.0, 1.0, 2.0]), **kw)
    r1 = dict(pl.last_result)
    assert r1["shift"] == 0 and r1["iter_base"] == 0 and np.all(np.isfinite(tr.positions)) and len(r1["trace"]) == 2
    assert np.array_equal(tr.positions[0], st.position)
    want = np.concatenate([r1["U"][1:], [[0.0, 0.0, pl.hover_thrust]]])
    assert pl._mppi_nominal(6, True)[0].tolist() == want.tolist()
    pl.plan_mppi(st, np.array([3.0, 1.0, 2.0]), **kw)
    r2 = dict(pl.last_result)
    assert r2["shift"] == 1 and r2["iter_base"] == 2
    # the same call made by hand from the shifted nominal
    ops, prm = pl._ops, pl._params()
    col = lambda a: ops.be.from_host(np.asarray(a, float).reshape(-1, 1).copy())
    o = ops.mppi(prm, col(st.position), col(st.velocity), col(pl.goal_position), col(want), 64, 2, 2.0, 50.0, seed=1, iter_base=2)
    assert np.array_equal(ops.be.to_host(o["U"])[:, 0].reshape(6, 3), r2["U"])
    pl.plan_mppi(st, np.array([-3.0, 1.0, 2.0]), **kw)
    assert pl.last_result["shift"] == 0, "a new goal resets the nominal to hover"
    pl.plan_mppi(st, np.array([-3.0, 1.0, 2.0]), warm_start=False, **kw)
    assert pl.last_result["shift"] == 0


def test_plan_batch_mppi_rows_are_single_problems():
    pl = _planner()
    rng = np.random.default_rng(2)
    B = 3
    pos, vel, goals = rng.uniform(-1, 1, (B, 3)) + [0, 0, 2], rng.uniform(-1, 1, (B, 3)), rng.uniform(-3, 3, (B, 3)) + [0, 0, 2]
    res = pl.plan_batch_mppi(pos, vel, goals, n_samples=64, iters=2, sigma=2.0, temperature=50.0, seed=4, precision="f64")
    assert res["positions"].shape == (B, 6, 3) and res["trace"].shape == (B, 2) and res["thrusts"].shape == (B, 6)
    ops, prm = pl._ops, pl._params(has_goal=1)
    col = lambda a: ops.be.from_host(np.asarray(a, float).reshape(-1, 1).copy())
    for b in range(B):
        o = ops.mppi(prm, col(pos[b]), col(vel[b]), col(goals[b]), col(np.tile([0.0, 0.0, pl.hover_thrust], (6, 1))), 64, 2, 2.0, 50.0, seed=4,
                     index_base=b)
        assert np.array_equal(ops.be.to_host(o["U"])[:, 0].reshape(6, 3), res["thrust_vectors"][b])
        assert ops.be.to_host(o["cost"])[0] == res["cost"][b]
    assert np.allclose(res["positions"][:, 0], pos)
