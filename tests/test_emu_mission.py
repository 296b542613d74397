"""CPU suite: the mission layer's goal source -- se3mpc_mission_goal_*, se3mpc_monte_carlo_mission_*, ClosedLoopMonteCarlo.run_mission /
run_mission_fused and the mirror GlobalMissionPlanner -- on the product kernels compiled for the host (tests/emu): the checks of
tests/mission_checks.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402
from numpy_backend import TorchCpuBackend  # noqa: E402

from dart_planner_amd import capi  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402
import parity_checks as pc  # noqa: E402
import mission_checks as mc  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops, dt=np.float64):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), dt)


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_sequences_through_the_c_abi(emu_ops, dt):
    mc.check_golden_sequences(harness(emu_ops, dt))


def test_golden_sequences_through_the_mirror_class(emu_ops):
    mc.check_mirror_class(harness(emu_ops))


def test_stamp_table_gives_the_golden_grids(emu_ops):
    mc.check_stamp_table(harness(emu_ops))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B", [1, 63, 65, 130])
@pytest.mark.parametrize("W,per_drone", [(0, False), (4, False), (4, True), (0, True)])
def test_random_batches_against_the_oracle(emu_ops, dt, B, W, per_drone):
    mc.check_random_batch(harness(emu_ops, dt), B, W, per_drone)


@pytest.mark.parametrize("dt", DTYPES)
def test_run_mission_equals_its_hand_chained_form(emu_ops, dt):
    mc.check_run_mission_equals_hand_chain(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", [(6, 65), (6, 130), (30, 9)])
def test_one_launch_equals_the_chain_bit_for_bit(emu_ops, dt, N, B):
    mc.check_fused_equals_chain(harness(emu_ops, dt), N, B)


@pytest.mark.parametrize("dt", DTYPES)
def test_a_second_launch_continues_the_first(emu_ops, dt):
    mc.check_fused_continues(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_mppi_missions_equal_their_hand_chained_form(emu_ops, dt):
    mc.check_mppi_missions(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_behaviour_on_the_chain(emu_ops, dt):
    mc.check_behaviour(harness(emu_ops, dt), report=True)


def test_forms_that_are_not_built_raise(emu_ops):
    mc.check_unbuilt_forms(harness(emu_ops))


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(emu_ops, dt):
    mc.check_invalid_arguments(harness(emu_ops, dt))
