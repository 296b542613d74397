"""GPU suite (`-m gpu`): se3mpc_mppi_closed_loop_edge_* / Ops.mppi_closed_loop_edge / ClosedLoopMonteCarlo.run_mppi_edge_fused on a real MI355X:
the one-launch closed-loop MPPI Monte-Carlo on the reference's edge loop gives the bytes of the chain of launches it fuses, and its clearance
agrees with the positions that chain logs -- the checks of tests/mppi_closed_loop_edge_checks.py at every shape (at most 70 drones x 4 cycles x
10 steps, or 3 drones x 2 x 70)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_checks as pc  # noqa: E402
import mppi_closed_loop_edge_checks as ec  # noqa: E402


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
@pytest.mark.parametrize("shape", ec.SHAPES)
@pytest.mark.parametrize("substeps", ec.SUBSTEPS)
def test_chain_conditions_are_not_vacuous(gpu_ops, dt, shape, substeps):
    ec.check_not_vacuous(harness(gpu_ops, dt), shape, substeps)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.GPU_SHAPES)
@pytest.mark.parametrize("substeps", ec.SUBSTEPS)
@pytest.mark.parametrize("depth", ec.DEPTHS)
@pytest.mark.parametrize("wind", ec.WINDS)
def test_one_launch_equals_the_chain_byte_for_byte(gpu_ops, dt, shape, substeps, depth, wind):
    ec.check_equals_chain(harness(gpu_ops, dt), shape, depth, substeps, wind=wind, last_plan=depth == 2 and wind == "rows")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.GPU_SHAPES)
@pytest.mark.parametrize("depth", [1, 5])
def test_one_call_of_four_cycles_equals_four_calls_and_one_plus_three(gpu_ops, dt, shape, depth):
    ec.check_cycles_equal_calls(harness(gpu_ops, dt), shape, depth, 4)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.GPU_SHAPES)
@pytest.mark.parametrize("depth", [0, 5])
def test_a_slice_of_the_drones_gives_their_rows_and_ring_columns(gpu_ops, dt, shape, depth):
    ec.check_slices(harness(gpu_ops, dt), shape, depth, 10)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [ec.SHAPES[0], ec.SHAPES[2]])
@pytest.mark.parametrize("depth", ec.LONG_DEPTHS)
def test_an_act_phase_of_two_chunks_byte_for_byte(gpu_ops, dt, shape, depth):
    ec.check_long_act(harness(gpu_ops, dt), shape, depth)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [s for s in ec.GPU_SHAPES if s[2]])
@pytest.mark.parametrize("substeps", ec.SUBSTEPS)
def test_clearance_agrees_with_the_logged_chain(gpu_ops, dt, shape, substeps):
    ec.check_clearance(harness(gpu_ops, dt), shape, 5, substeps)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.GPU_SHAPES)
def test_without_steps_it_is_the_planner_and_touches_no_record(gpu_ops, dt, shape):
    ec.check_planner_inside(harness(gpu_ops, dt), shape)


@pytest.mark.parametrize("dt", DTYPES)
def test_argument_rules(gpu_ops, dt):
    ec.check_argument_rules(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_equals_chain_with_a_different_constant_in_every_block(gpu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    ec.check_equals_chain(harness(gpu_ops, dt), (L["N"], L["B"], L["K"], 64), 2, L["substeps"], last_plan=True, cycles=L["cycles"],
                          blocks=ps.loop_blocks(L["N"], dt=ec.PLAN_DT))
