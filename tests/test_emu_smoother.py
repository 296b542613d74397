"""CPU suite: the TrajectorySmoother kernels of dart_planner_amd/csrc/smoother.hip compiled for the host by tests/emu and driven through the C ABI, Ops,
ClosedLoopMonteCarlo and the mirror class: the checks of tests/smoother_checks.py."""
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
import smoother_checks as sc  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), dt)


DTYPES = [np.float64, np.float32]
BATCHES = [(1, 1, False, True, True), (63, 2, False, True, False), (64, 6, True, True, True), (65, 30, False, False, False), (130, 6, False, False, True),
           (65, 2, True, False, True)]


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_sequences_through_the_c_abi(emu_ops, dt):
    sc.check_golden_sequences(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_closed_loops(emu_ops, dt):
    sc.check_golden_loops(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_switching_scene_keeps_the_reference_s_commanded_jump(emu_ops, dt):
    sc.check_switch_scene(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,N,shared,with_v,with_a", BATCHES)
def test_random_batches_against_the_oracle(emu_ops, dt, B, N, shared, with_v, with_a):
    sc.check_random_batch(harness(emu_ops, dt), B, N, shared, with_v, with_a)


@pytest.mark.parametrize("dt", DTYPES)
def test_empty_plan_samples_zeros(emu_ops, dt):
    sc.check_empty_plan(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,N,n", [(65, 6, 20), (130, 30, 7)])
def test_one_launch_equals_chained_launches_bit_for_bit(emu_ops, dt, B, N, n):
    sc.check_bit_for_bit(harness(emu_ops, dt), B, N, n)


@pytest.mark.parametrize("dt", DTYPES)
def test_monte_carlo_option(emu_ops, dt):
    sc.check_monte_carlo_option(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_mirror_class(emu_ops, dt, monkeypatch):
    sc.check_mirror(harness(emu_ops, dt), monkeypatch)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(emu_ops, dt):
    sc.check_invalid_arguments(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_dirty_buffers_and_nan_drone(emu_ops, dt):
    sc.check_dirty_buffers_and_nan_drone(harness(emu_ops, dt))
