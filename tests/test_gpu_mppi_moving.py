"""GPU suite (`-m gpu`): MPPI around moving spheres (dart_planner_amd/csrc/mppi_moving.hip, mppi_closed_loop_moving.hip) on a real MI355X
through the C ABI, Ops, SE3MPCPlanner and ClosedLoopMonteCarlo: the checks of tests/mppi_moving_checks.py at N in {1, 6, 13}, K in
{0, 1, 3} (odd K: the alignment of the [K][3] table), S in {64, 320} (one full chunk and a partial one), both types."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mppi_moving_checks as mv  # noqa: E402
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
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"), lambda a: a.detach().cpu().numpy(), dt)


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,nprob,K", [(1, 64, 3, 1), (6, 320, 3, 3), (13, 64, 4, 0), (13, 320, 3, 3)])
def test_zero_velocity_is_the_static_planner(gpu_ops, dt, N, S, nprob, K):
    mv.check_zero_velocity_planner(harness(gpu_ops, dt), N, S, nprob, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,S", [(1, 3, 1, 64), (6, 3, 3, 320), (13, 4, 0, 64), (13, 3, 3, 320)])
def test_zero_velocity_is_the_static_closed_loop(gpu_ops, dt, N, B, K, S):
    mv.check_zero_velocity_closed_loop(harness(gpu_ops, dt), N, B, K, S=S)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,nprob,iters,K", [(1, 64, 3, 2, 1), (6, 64, 3, 3, 3), (6, 320, 3, 2, 1), (13, 320, 4, 2, 3), (13, 64, 3, 2, 0)])
def test_against_the_oracle(gpu_ops, dt, N, S, nprob, iters, K):
    mv.check_against_oracle(harness(gpu_ops, dt), N, S, nprob, iters, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,K", [(6, 64, 3), (13, 320, 1), (1, 64, 0)])
def test_iteration_chunks_and_problem_slices(gpu_ops, dt, N, S, K):
    mv.check_chunking_and_slices(harness(gpu_ops, dt), N, S, 4, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,S,shift,wind", [(6, 4, 1, 64, 1, "per_drone"), (13, 3, 3, 320, 0, "shared"), (1, 3, 3, 64, 1, None), (6, 3, 0, 320, 6, "shared")])
def test_cycles_in_one_call_equal_chained_calls(gpu_ops, dt, N, B, K, S, shift, wind):
    mv.check_cycle_equivalence(harness(gpu_ops, dt), N, B, K, S=S, shift=shift, wind=wind)


@pytest.mark.parametrize("dt", DTYPES)
def test_long_act_phase_runs_in_chunks(gpu_ops, dt):
    mv.check_cycle_equivalence(harness(gpu_ops, dt), 6, 3, 3, cycles=2, substeps=70, sim_dt=0.002)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,S", [(6, 3, 1, 64), (13, 3, 3, 320), (1, 3, 0, 64)])
def test_planner_inside_is_the_planner_outside(gpu_ops, dt, N, B, K, S):
    mv.check_planner_inside(harness(gpu_ops, dt), N, B, K, S=S)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,S", [(6, 3, 1, 64), (13, 4, 3, 320)])
def test_clearance_against_the_oracle(gpu_ops, dt, N, B, K, S):
    mv.check_clearance(harness(gpu_ops, dt), N, B, K, S=S)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_penalty_dodges_the_sphere_that_crosses_the_goal(gpu_ops, dt):
    mv.check_behaviour(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_determinism_dirty_buffers_and_nan_drone(gpu_ops, dt):
    mv.check_determinism_and_dirty_buffers(harness(gpu_ops, dt), N=13, B=4, K=3)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(gpu_ops, dt):
    mv.check_invalid_arguments(harness(gpu_ops, dt))


def _planner(N, dt=0.1):
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=N), device="cuda:0")
    pl.se3_config = SE3MPCConfig(**{**pl.se3_config.__dict__, "dt": dt})
    return pl


@pytest.mark.parametrize("dt", DTYPES)
def test_front_end(gpu_ops, dt):
    mv.check_front_end(harness(gpu_ops, dt), _planner)


@pytest.mark.parametrize("dt", DTYPES)
def test_a_different_constant_in_every_block(gpu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    b = ps.loop_blocks(L["N"], dt=0.1)
    kw = dict(prm=b["prm"], cp=b["cp"], sp=b["sp"], ccfg=b["ccfg"], sim=b["sim"])
    mv.check_cycle_equivalence(harness(gpu_ops, dt), L["N"], L["B"], L["K"], cycles=L["cycles"], substeps=L["substeps"], **kw)
    mv.check_planner_inside(harness(gpu_ops, dt), L["N"], L["B"], L["K"], run_substeps=L["substeps"], **kw)
