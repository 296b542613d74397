"""CPU suite: MPPI around moving spheres (dart_planner_amd/csrc/mppi_moving.hip, mppi_closed_loop_moving.hip: se3mpc_mppi_moving_*,
se3mpc_mppi_closed_loop_moving_*) compiled for the host by tests/emu and driven through the C ABI, Ops, SE3MPCPlanner and
ClosedLoopMonteCarlo: the checks of tests/mppi_moving_checks.py at small shapes (N in {1, 6, 13}, K in {0, 1, 3}, S = 64, and S = 320 -- one full chunk and a partial one -- where the emulation affords it; the MI355X
suite runs every check at S = 320)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402
from numpy_backend import TorchCpuBackend  # noqa: E402

from dart_planner_amd import capi  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402
import mppi_moving_checks as mv  # noqa: E402
import parity_checks as pc  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), dt)


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,nprob,K", [(1, 64, 3, 1), (6, 320, 3, 3), (13, 64, 4, 0), (13, 64, 3, 3)])
def test_zero_velocity_is_the_static_planner(emu_ops, dt, N, S, nprob, K):
    mv.check_zero_velocity_planner(harness(emu_ops, dt), N, S, nprob, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,S", [(1, 3, 1, 64), (6, 3, 3, 320), (13, 4, 0, 64), (13, 3, 3, 64)])
def test_zero_velocity_is_the_static_closed_loop(emu_ops, dt, N, B, K, S):
    mv.check_zero_velocity_closed_loop(harness(emu_ops, dt), N, B, K, S=S, cycles=1 if S > 64 else 2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,nprob,iters,K", [(1, 64, 3, 2, 1), (6, 64, 3, 3, 3), (6, 320, 3, 2, 1), (13, 64, 4, 2, 3), (13, 64, 3, 2, 0)])
def test_against_the_oracle(emu_ops, dt, N, S, nprob, iters, K):
    mv.check_against_oracle(harness(emu_ops, dt), N, S, nprob, iters, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,K", [(6, 64, 3), (13, 64, 1), (1, 64, 0)])
def test_iteration_chunks_and_problem_slices(emu_ops, dt, N, S, K):
    mv.check_chunking_and_slices(harness(emu_ops, dt), N, S, 4, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,S,shift,wind", [(6, 4, 1, 64, 1, "per_drone"), (13, 3, 3, 64, 0, "shared"), (1, 3, 3, 64, 1, None), (6, 3, 0, 64, 6, "shared")])
def test_cycles_in_one_call_equal_chained_calls(emu_ops, dt, N, B, K, S, shift, wind):
    mv.check_cycle_equivalence(harness(emu_ops, dt), N, B, K, S=S, shift=shift, wind=wind)


@pytest.mark.parametrize("dt", DTYPES)
def test_long_act_phase_runs_in_chunks(emu_ops, dt):
    """More simulator steps per cycle than one clearance reduction parks (64): the parked times continue across the chunks."""
    mv.check_cycle_equivalence(harness(emu_ops, dt), 6, 3, 3, cycles=2, substeps=70, sim_dt=0.002)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,S", [(6, 3, 1, 64), (13, 3, 3, 64), (1, 3, 0, 64)])
def test_planner_inside_is_the_planner_outside(emu_ops, dt, N, B, K, S):
    mv.check_planner_inside(harness(emu_ops, dt), N, B, K, S=S)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K", [(6, 3, 1), (13, 4, 3)])
def test_clearance_against_the_oracle(emu_ops, dt, N, B, K):
    mv.check_clearance(harness(emu_ops, dt), N, B, K)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_penalty_dodges_the_sphere_that_crosses_the_goal(emu_ops, dt):
    mv.check_behaviour(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_determinism_dirty_buffers_and_nan_drone(emu_ops, dt):
    mv.check_determinism_and_dirty_buffers(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(emu_ops, dt):
    mv.check_invalid_arguments(harness(emu_ops, dt))


def _planner(ops):
    def make(N, dt=0.1):
        from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
        pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=N))
        pl.se3_config = SE3MPCConfig(**{**pl.se3_config.__dict__, "dt": dt})
        pl._ops = ops
        return pl
    return make


@pytest.mark.parametrize("dt", DTYPES)
def test_front_end(emu_ops, dt):
    mv.check_front_end(harness(emu_ops, dt), _planner(emu_ops))


@pytest.mark.parametrize("dt", DTYPES)
def test_a_different_constant_in_every_block(emu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    b = ps.loop_blocks(L["N"], dt=0.1)
    kw = dict(prm=b["prm"], cp=b["cp"], sp=b["sp"], ccfg=b["ccfg"], sim=b["sim"])
    mv.check_cycle_equivalence(harness(emu_ops, dt), L["N"], L["B"], L["K"], cycles=L["cycles"], substeps=L["substeps"], **kw)
    mv.check_planner_inside(harness(emu_ops, dt), L["N"], L["B"], L["K"], run_substeps=L["substeps"], **kw)
