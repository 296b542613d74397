"""CPU suite: the closed-loop MPPI Monte-Carlo of dart_planner_amd/csrc/mppi_closed_loop.hip (se3mpc_mppi_closed_loop_*: plan, control and
simulate, every cycle of every drone in one launch) compiled for the host by tests/emu and driven through the C ABI, Ops and
ClosedLoopMonteCarlo: the checks of tests/mppi_closed_loop_checks.py at small shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402
from numpy_backend import TorchCpuBackend  # noqa: E402

from dart_planner_amd import capi  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402
import mppi_closed_loop_checks as lc  # noqa: E402
import parity_checks as pc  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), dt)


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,shift,wind", [(6, 4, 0, 1, "per_drone"), (6, 3, 2, 0, "shared"), (13, 3, 3, 13, None), (13, 4, 0, 1, "shared")])
def test_cycles_in_one_call_equal_chained_calls(emu_ops, dt, N, B, K, shift, wind):
    lc.check_cycle_equivalence(harness(emu_ops, dt), N, B, K, shift=shift, wind=wind)


@pytest.mark.parametrize("dt", DTYPES)
def test_long_act_phase_runs_in_chunks(emu_ops, dt):
    """More simulator steps per cycle than one clearance reduction parks (64): the act phase continues across the chunks."""
    lc.check_cycle_equivalence(harness(emu_ops, dt), 6, 3, 2, cycles=2, substeps=70, sim_dt=0.002)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K", [(6, 3, 0), (13, 3, 2)])
def test_planner_inside_is_the_planner_outside(emu_ops, dt, N, B, K):
    lc.check_planner_inside(harness(emu_ops, dt), N, B, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K", [(6, 4, 0), (13, 3, 3)])
def test_against_the_float64_chain_cycle_by_cycle(emu_ops, dt, N, B, K):
    lc.check_against_oracle(harness(emu_ops, dt), N, B, K)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_penalty_keeps_every_drone_clear_of_the_sphere(emu_ops, dt):
    lc.check_behaviour(harness(emu_ops, dt), B=2, N=8, cycles=15)


@pytest.mark.parametrize("dt", DTYPES)
def test_determinism_dirty_buffers_and_nan_drone(emu_ops, dt):
    lc.check_determinism_and_dirty_buffers(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(emu_ops, dt):
    lc.check_invalid_arguments(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_front_end(emu_ops, dt):
    lc.check_front_end(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_a_different_constant_in_every_block(emu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    b = ps.loop_blocks(L["N"], dt=0.1)
    kw = dict(prm=b["prm"], cp=b["cp"], sp=b["sp"], ccfg=b["ccfg"], sim=b["sim"])
    lc.check_cycle_equivalence(harness(emu_ops, dt), L["N"], L["B"], L["K"], cycles=L["cycles"], substeps=L["substeps"], **kw)
    lc.check_planner_inside(harness(emu_ops, dt), L["N"], L["B"], L["K"], substeps=L["substeps"], **kw)
    lc.check_against_oracle(harness(emu_ops, dt), L["N"], L["B"], L["K"], cycles=L["cycles"], substeps=L["substeps"], **kw)
