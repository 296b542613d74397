"""CPU suite: the swarm MPPI closed loop (dart_planner_amd/csrc/mppi_swarm.hip: se3mpc_mppi_closed_loop_swarm_*, se3mpc_swarm_separation_*)
compiled for the host by tests/emu and driven through the C ABI, Ops and ClosedLoopMonteCarlo: the checks of tests/mppi_swarm_checks.py at
N in {1, 6, 13}, S in {64, 320}, swarms in {1, 3}, M in {1, 2, 5, 70} (70 mates: more than a 64-lane workgroup has lanes), Kn in {0, 1, 3, 8}
(8 > the mates of a swarm of 5), Ks in {0, 2} (the mates sit behind the shared rows; odd totals)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402
from numpy_backend import TorchCpuBackend  # noqa: E402

from dart_planner_amd import capi  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402
import mppi_swarm_checks as sw  # noqa: E402
import parity_checks as pc  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), dt)


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,swarms,M,Kn,Ks", [(6, 64, 3, 1, 3, 2), (13, 64, 1, 5, 0, 2), (1, 64, 1, 1, 8, 0), (6, 320, 1, 2, 0, 0)])
def test_without_mates_it_is_the_moving_loop(emu_ops, dt, N, S, swarms, M, Kn, Ks):
    sw.check_reduces_to_moving(harness(emu_ops, dt), N, S, swarms, M, Kn, Ks, cycles=1 if S > 64 else 2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,swarms,M,Kn,Ks,cycles,substeps", [(6, 64, 3, 5, 3, 2, 2, 2), (6, 64, 1, 70, 3, 0, 2, 1), (1, 64, 3, 2, 1, 0, 3, 3),
                                                              (13, 64, 1, 5, 8, 2, 2, 3)])
def test_equals_the_per_drone_chain_of_the_moving_entry(emu_ops, dt, N, S, swarms, M, Kn, Ks, cycles, substeps):
    sw.check_chain(harness(emu_ops, dt), N, S, swarms, M, Kn, Ks, cycles=cycles, substeps=substeps, mates_matter=M == 5)


@pytest.mark.parametrize("dt", DTYPES)
def test_selection_ties_short_swarms_and_a_nan_drone(emu_ops, dt):
    sw.check_selection(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [2, 70])
def test_separation_entry_against_numpy(emu_ops, dt, M):
    sw.check_separation_entry(harness(emu_ops, dt), M)


@pytest.mark.parametrize("dt", DTYPES)
def test_separation_of_a_run_is_the_minimum_over_cycle_starts_and_the_end(emu_ops, dt):
    sw.check_separation_of_a_run(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_clearance_sees_the_shared_rows_only(emu_ops, dt):
    sw.check_clearance(harness(emu_ops, dt), 6, swarms=1, cycles=4)


@pytest.mark.parametrize("dt", DTYPES)
def test_continuation_determinism_and_dirty_buffers(emu_ops, dt):
    sw.check_continuation_and_determinism(harness(emu_ops, dt), swarms=1)


@pytest.mark.parametrize("dt", DTYPES)
def test_two_drones_swapping_places_keep_apart(emu_ops, dt):
    sw.check_behaviour(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(emu_ops, dt):
    sw.check_invalid_arguments(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_front_end(emu_ops, dt):
    sw.check_front_end(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_equals_the_per_drone_chain_with_a_different_constant_in_every_block(emu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    b = ps.loop_blocks(L["N"], dt=0.1)
    sw.check_chain(harness(emu_ops, dt), L["N"], 64, 1, L["B"], 2, L["K"], cycles=L["cycles"], substeps=L["substeps"], mates_matter=False,
                   prm=b["prm"], cp=b["cp"], sp=b["sp"], ccfg=b["ccfg"], sim=b["sim"])
