"""GPU suite (`-m gpu`): the mission layer's goal source -- se3mpc_mission_goal_*, se3mpc_monte_carlo_mission_*, ClosedLoopMonteCarlo.run_mission /
run_mission_fused and the mirror GlobalMissionPlanner -- on a real MI355X: the checks of tests/mission_checks.py (at most 130 drones, 6 cycles of 5
steps; the golden sequences are 1582 one-drone calls)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_checks as pc  # noqa: E402
import mission_checks as mc  # noqa: E402


@pytest.fixture(scope="module")
def gpu_ops():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend("cuda:0"))
    assert ops.lib.device_count() >= 1, "no gfx950 device visible to libse3mpc"
    assert os.path.basename(ops.lib.path) == "libse3mpc.so"
    return ops


def harness(ops, dt=np.float64):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"), lambda a: a.detach().cpu().numpy(), dt)


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_sequences_through_the_c_abi(gpu_ops, dt):
    mc.check_golden_sequences(harness(gpu_ops, dt))


def test_golden_sequences_through_the_mirror_class(gpu_ops):
    mc.check_mirror_class(harness(gpu_ops))


def test_stamp_table_gives_the_golden_grids(gpu_ops):
    mc.check_stamp_table(harness(gpu_ops))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B", [1, 63, 65, 130])
@pytest.mark.parametrize("W,per_drone", [(0, False), (4, False), (4, True), (0, True)])
def test_random_batches_against_the_oracle(gpu_ops, dt, B, W, per_drone):
    mc.check_random_batch(harness(gpu_ops, dt), B, W, per_drone)


@pytest.mark.parametrize("dt", DTYPES)
def test_run_mission_equals_its_hand_chained_form(gpu_ops, dt):
    mc.check_run_mission_equals_hand_chain(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", [(6, 65), (6, 130), (30, 9)])
def test_one_launch_equals_the_chain_bit_for_bit(gpu_ops, dt, N, B):
    mc.check_fused_equals_chain(harness(gpu_ops, dt), N, B)


@pytest.mark.parametrize("dt", DTYPES)
def test_a_second_launch_continues_the_first(gpu_ops, dt):
    mc.check_fused_continues(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_mppi_missions_equal_their_hand_chained_form(gpu_ops, dt):
    mc.check_mppi_missions(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_behaviour_on_the_chain(gpu_ops, dt):
    mc.check_behaviour(harness(gpu_ops, dt), report=True)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(gpu_ops, dt):
    mc.check_invalid_arguments(harness(gpu_ops, dt))
