"""GPU suite (`-m gpu`): the TrajectorySmoother kernels of dart_planner_amd/csrc/smoother.hip on a real MI355X through the C ABI, Ops,
ClosedLoopMonteCarlo and the mirror class: the checks of tests/smoother_checks.py (at most 130 drones x 300 steps)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_checks as pc  # noqa: E402
import smoother_checks as sc  # noqa: E402


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
BATCHES = [(1, 1, False, True, True), (63, 2, False, True, False), (64, 6, True, True, True), (65, 30, False, False, False), (130, 6, False, False, True),
           (65, 2, True, False, True)]


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_sequences_through_the_c_abi(gpu_ops, dt):
    sc.check_golden_sequences(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_closed_loops(gpu_ops, dt):
    sc.check_golden_loops(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_switching_scene_keeps_the_reference_s_commanded_jump(gpu_ops, dt):
    sc.check_switch_scene(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,N,shared,with_v,with_a", BATCHES)
def test_random_batches_against_the_oracle(gpu_ops, dt, B, N, shared, with_v, with_a):
    sc.check_random_batch(harness(gpu_ops, dt), B, N, shared, with_v, with_a)


@pytest.mark.parametrize("dt", DTYPES)
def test_empty_plan_samples_zeros(gpu_ops, dt):
    sc.check_empty_plan(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,N,n", [(65, 6, 20), (130, 30, 7)])
def test_one_launch_equals_chained_launches_bit_for_bit(gpu_ops, dt, B, N, n):
    sc.check_bit_for_bit(harness(gpu_ops, dt), B, N, n)


@pytest.mark.parametrize("dt", DTYPES)
def test_monte_carlo_option(gpu_ops, dt):
    sc.check_monte_carlo_option(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_mirror_class(gpu_ops, dt, monkeypatch):
    sc.check_mirror(harness(gpu_ops, dt), monkeypatch)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(gpu_ops, dt):
    sc.check_invalid_arguments(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_dirty_buffers_and_nan_drone(gpu_ops, dt):
    sc.check_dirty_buffers_and_nan_drone(harness(gpu_ops, dt))
