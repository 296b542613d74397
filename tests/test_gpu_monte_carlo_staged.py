"""GPU suite (`-m gpu`): se3mpc_monte_carlo_staged_* / ClosedLoopMonteCarlo.run_fused_staged on a real MI355X: the one-launch Monte-Carlo with
the TrajectorySmoother and the MotorMixer inside gives the bits of the chain of launches it fuses -- the checks of
tests/monte_carlo_staged_checks.py (at most 130 drones x 6 cycles x 10 steps)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_checks as pc  # noqa: E402
import monte_carlo_staged_checks as sc  # noqa: E402


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
@pytest.mark.parametrize("N,B", sc.SHAPES)
def test_chain_conditions_are_not_vacuous(gpu_ops, dt, N, B):
    sc.check_not_vacuous(harness(gpu_ops, dt), N, B)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", sc.GPU_SHAPES)
@pytest.mark.parametrize("stage", list(sc.STAGES))
def test_one_launch_equals_the_chain_bit_for_bit(gpu_ops, dt, N, B, stage):
    sc.check_equals_chain(harness(gpu_ops, dt), N, B, stage, last_plan=stage == "both_health")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", sc.GPU_SHAPES)
@pytest.mark.parametrize("wind", [None, "shared"])
def test_one_launch_equals_the_chain_without_and_with_shared_wind(gpu_ops, dt, N, B, wind):
    sc.check_equals_chain(harness(gpu_ops, dt), N, B, "both_health", wind=wind)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", sc.GPU_SHAPES)
@pytest.mark.parametrize("smoother", ["no_transition", "short_timeout"])
def test_smoother_branches_bit_for_bit(gpu_ops, dt, N, B, smoother):
    sc.check_equals_chain(harness(gpu_ops, dt), N, B, "both_health", smoother=smoother)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", sc.GPU_SHAPES)
def test_absent_stages_equal_run_fused(gpu_ops, dt, N, B):
    sc.check_absent_stages_equal_run_fused(harness(gpu_ops, dt), N, B)


@pytest.mark.parametrize("dt", DTYPES)
def test_argument_rules(gpu_ops, dt):
    sc.check_argument_rules(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_equals_chain_with_a_different_constant_in_every_block(gpu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    sc.check_equals_chain(harness(gpu_ops, dt), L["N"], L["B"], "both_health", last_plan=True, cycles=L["cycles"], substeps=L["substeps"],
                          blocks=ps.loop_blocks(L["N"]))
