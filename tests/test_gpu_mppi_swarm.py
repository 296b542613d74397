"""GPU suite (`-m gpu`): the swarm MPPI closed loop (dart_planner_amd/csrc/mppi_swarm.hip) on a real MI355X through the C ABI, Ops and
ClosedLoopMonteCarlo: the checks of tests/mppi_swarm_checks.py at N in {1, 6, 13}, S in {64, 320} (one full chunk and a partial one),
swarms in {1, 3}, M in {1, 2, 5, 70} (70 mates: the prologue loops over a 64-lane workgroup), Kn in {0, 1, 3, 8} (8 > the mates of a swarm of
5), Ks in {0, 2} (the mates sit behind the shared rows; odd totals), both types."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mppi_swarm_checks as sw  # noqa: E402
import parity_checks as pc  # noqa: E402


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
@pytest.mark.parametrize("N,S,swarms,M,Kn,Ks", [(6, 64, 3, 1, 3, 2), (13, 320, 3, 5, 0, 2), (1, 64, 1, 1, 8, 0), (6, 320, 1, 5, 0, 0)])
def test_without_mates_it_is_the_moving_loop(gpu_ops, dt, N, S, swarms, M, Kn, Ks):
    sw.check_reduces_to_moving(harness(gpu_ops, dt), N, S, swarms, M, Kn, Ks, cycles=3)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,swarms,M,Kn,Ks,cycles,substeps", [(13, 320, 3, 5, 3, 2, 3, 2), (6, 64, 1, 70, 3, 0, 2, 1), (1, 64, 3, 2, 1, 0, 3, 3),
                                                              (13, 64, 1, 5, 8, 2, 2, 3)])
def test_equals_the_per_drone_chain_of_the_moving_entry(gpu_ops, dt, N, S, swarms, M, Kn, Ks, cycles, substeps):
    sw.check_chain(harness(gpu_ops, dt), N, S, swarms, M, Kn, Ks, cycles=cycles, substeps=substeps, mates_matter=M == 5)


@pytest.mark.parametrize("dt", DTYPES)
def test_selection_ties_short_swarms_and_a_nan_drone(gpu_ops, dt):
    sw.check_selection(harness(gpu_ops, dt), N=13, S=320)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [2, 70])
def test_separation_entry_against_numpy(gpu_ops, dt, M):
    sw.check_separation_entry(harness(gpu_ops, dt), M)


@pytest.mark.parametrize("dt", DTYPES)
def test_separation_of_a_run_is_the_minimum_over_cycle_starts_and_the_end(gpu_ops, dt):
    sw.check_separation_of_a_run(harness(gpu_ops, dt), N=13, S=320)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S", [(6, 64), (13, 320)])
def test_clearance_sees_the_shared_rows_only(gpu_ops, dt, N, S):
    sw.check_clearance(harness(gpu_ops, dt), N, S=S)


@pytest.mark.parametrize("dt", DTYPES)
def test_continuation_determinism_and_dirty_buffers(gpu_ops, dt):
    sw.check_continuation_and_determinism(harness(gpu_ops, dt), N=13, S=320)


@pytest.mark.parametrize("dt", DTYPES)
def test_two_drones_swapping_places_keep_apart(gpu_ops, dt):
    sw.check_behaviour(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(gpu_ops, dt):
    sw.check_invalid_arguments(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_front_end(gpu_ops, dt):
    sw.check_front_end(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_equals_the_per_drone_chain_with_a_different_constant_in_every_block(gpu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    b = ps.loop_blocks(L["N"], dt=0.1)
    sw.check_chain(harness(gpu_ops, dt), L["N"], 64, 1, L["B"], 2, L["K"], cycles=L["cycles"], substeps=L["substeps"], mates_matter=False,
                   prm=b["prm"], cp=b["cp"], sp=b["sp"], ccfg=b["ccfg"], sim=b["sim"])
