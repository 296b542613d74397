"""GPU suite (`-m gpu`): se3mpc_mppi_closed_loop_staged_* / ClosedLoopMonteCarlo.run_mppi_fused_staged on a real MI355X: the one-launch
closed-loop MPPI Monte-Carlo with the TrajectorySmoother and the MotorMixer inside gives the bits of the chain of launches it fuses, and a
clearance that agrees with the positions that chain logs -- the checks of tests/mppi_closed_loop_staged_checks.py (at most 5 drones x 4
cycles x 5 steps, 512 samples)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_checks as pc  # noqa: E402
import mppi_closed_loop_staged_checks as sc  # noqa: E402


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
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_chain_conditions_are_not_vacuous(gpu_ops, dt, shape):
    sc.check_not_vacuous(harness(gpu_ops, dt), shape)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("stage", list(sc.STAGES))
def test_one_launch_equals_the_chain_bit_for_bit(gpu_ops, dt, shape, stage):
    sc.check_equals_chain(harness(gpu_ops, dt), shape, stage)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("wind", [None, "shared"])
def test_one_launch_equals_the_chain_without_and_with_shared_wind(gpu_ops, dt, shape, wind):
    sc.check_equals_chain(harness(gpu_ops, dt), shape, "both_health", wind=wind)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("smoother", ["no_transition", "short_timeout"])
def test_smoother_branches_bit_for_bit(gpu_ops, dt, shape, smoother):
    sc.check_equals_chain(harness(gpu_ops, dt), shape, "both_health", smoother=smoother)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("shift", [0, 1, "N"])
def test_every_shift_bit_for_bit(gpu_ops, dt, shape, shift):
    sc.check_equals_chain(harness(gpu_ops, dt), shape, "both_health", shift=shape[0] if shift == "N" else shift)


@pytest.mark.parametrize("dt", DTYPES)
def test_an_act_phase_of_two_chunks_bit_for_bit(gpu_ops, dt):
    sc.check_equals_chain(harness(gpu_ops, dt), sc.SHAPES[0], "both_health", substeps=sc.LONG_SUBSTEPS)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [s for s in sc.SHAPES if s[2]])
def test_clearance_agrees_with_the_logged_chain(gpu_ops, dt, shape):
    sc.check_clearance(harness(gpu_ops, dt), shape)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_absent_stages_equal_run_mppi_fused(gpu_ops, dt, shape):
    sc.check_without_stages(harness(gpu_ops, dt), shape)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_a_second_launch_continues_the_run_and_slices_are_rows(gpu_ops, dt, shape):
    sc.check_continuation(harness(gpu_ops, dt), shape)


@pytest.mark.parametrize("dt", DTYPES)
def test_argument_rules(gpu_ops, dt):
    sc.check_argument_rules(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_equals_chain_with_a_different_constant_in_every_block(gpu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    sc.check_equals_chain(harness(gpu_ops, dt), (L["N"], L["B"], L["K"], 64), "both_health", cycles=L["cycles"], substeps=L["substeps"],
                          blocks=ps.loop_blocks(L["N"], dt=sc.PLAN_DT))
