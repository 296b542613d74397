"""GPU suite (`-m gpu`): the MotorMixer / motor model kernels of dart_planner_amd/csrc/mixer.hip on a real MI355X through the C ABI, Ops,
ClosedLoopMonteCarlo and the mirror classes: the checks of tests/mixer_checks.py (at most 130 drones x 300 steps)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_checks as pc  # noqa: E402
import mixer_checks as xc  # noqa: E402


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
BATCHES = [(1, "default", None, "all"), (63, "linear", "shared", "all"), (64, "dead_and_linear", "per_drone", "all"), (65, "disc_negative", None, "pwm_only"),
           (130, "high_motor_limit", "per_drone", "no_state"), (65, "mixed", "shared", "all")]


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_sequences_through_the_c_abi(gpu_ops, dt):
    xc.check_golden_sequences(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_closed_loops(gpu_ops, dt):
    xc.check_golden_loops(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_body_rate_commands_and_watchdog(gpu_ops, dt):
    xc.check_golden_body_rate(harness(gpu_ops, dt))


def test_default_params_match_the_reference_s_x_factory(gpu_ops):
    xc.check_golden_matrices_and_defaults(harness(gpu_ops, np.float64))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,model,health,outputs", BATCHES)
def test_random_batches_against_the_oracle(gpu_ops, dt, B, model, health, outputs):
    xc.check_random_batch(harness(gpu_ops, dt), B, model, health, outputs)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("smoothed", [False, True])
@pytest.mark.parametrize("B,N,n", [(65, 6, 20), (130, 30, 7)])
def test_one_launch_equals_chained_launches_bit_for_bit(gpu_ops, dt, B, N, n, smoothed):
    xc.check_bit_for_bit(harness(gpu_ops, dt), B, N, n, smoothed)


@pytest.mark.parametrize("dt", DTYPES)
def test_transparent_mixer_equals_the_plain_closed_loop(gpu_ops, dt):
    xc.check_transparent_mixer_equals_plain_loop(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_behaviour_under_actuator_limits(gpu_ops, dt):
    xc.check_behaviour(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_monte_carlo_option(gpu_ops, dt):
    xc.check_monte_carlo_option(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_mirror_classes(gpu_ops, dt, monkeypatch):
    xc.check_mirror(harness(gpu_ops, dt), monkeypatch)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(gpu_ops, dt):
    xc.check_invalid_arguments(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_dirty_buffers_and_nan_drone(gpu_ops, dt):
    xc.check_dirty_buffers_and_nan_drone(harness(gpu_ops, dt))
