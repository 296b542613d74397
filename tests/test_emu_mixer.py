"""CPU suite: the MotorMixer / motor model kernels of dart_planner_amd/csrc/mixer.hip compiled for the host by tests/emu and driven through the C ABI,
Ops, ClosedLoopMonteCarlo and the mirror classes: the checks of tests/mixer_checks.py."""
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
import mixer_checks as xc  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), dt)


DTYPES = [np.float64, np.float32]
BATCHES = [(1, "default", None, "all"), (63, "linear", "shared", "all"), (64, "dead_and_linear", "per_drone", "all"), (65, "disc_negative", None, "pwm_only"),
           (130, "high_motor_limit", "per_drone", "no_state"), (65, "mixed", "shared", "all")]


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_sequences_through_the_c_abi(emu_ops, dt):
    xc.check_golden_sequences(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_closed_loops(emu_ops, dt):
    xc.check_golden_loops(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_body_rate_commands_and_watchdog(emu_ops, dt):
    xc.check_golden_body_rate(harness(emu_ops, dt))


def test_default_params_match_the_reference_s_x_factory(emu_ops):
    xc.check_golden_matrices_and_defaults(harness(emu_ops, np.float64))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,model,health,outputs", BATCHES)
def test_random_batches_against_the_oracle(emu_ops, dt, B, model, health, outputs):
    xc.check_random_batch(harness(emu_ops, dt), B, model, health, outputs)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("smoothed", [False, True])
@pytest.mark.parametrize("B,N,n", [(65, 6, 20), (130, 30, 7)])
def test_one_launch_equals_chained_launches_bit_for_bit(emu_ops, dt, B, N, n, smoothed):
    xc.check_bit_for_bit(harness(emu_ops, dt), B, N, n, smoothed)


@pytest.mark.parametrize("dt", DTYPES)
def test_transparent_mixer_equals_the_plain_closed_loop(emu_ops, dt):
    xc.check_transparent_mixer_equals_plain_loop(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_behaviour_under_actuator_limits(emu_ops, dt):
    xc.check_behaviour(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_monte_carlo_option(emu_ops, dt):
    xc.check_monte_carlo_option(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_mirror_classes(emu_ops, dt, monkeypatch):
    xc.check_mirror(harness(emu_ops, dt), monkeypatch)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(emu_ops, dt):
    xc.check_invalid_arguments(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_dirty_buffers_and_nan_drone(emu_ops, dt):
    xc.check_dirty_buffers_and_nan_drone(harness(emu_ops, dt))
