"""GPU suite (`-m gpu`): MPPI around tracked spheres and the swarm's shared plans (dart_planner_amd/csrc/mppi_tracks.hip,
mppi_closed_loop_tracks.hip, mppi_swarm.hip) on a real MI355X through the C ABI, Ops, SE3MPCPlanner and ClosedLoopMonteCarlo: the checks of
tests/mppi_tracks_checks.py at the shapes of tests/test_emu_mppi_tracks.py.  Unless a case says otherwise N = 6, S = 64, 2 swarms of M = 5,
Kn = 3, Ks = 2, 2-3 cycles x 3 substeps; the chain also at N = 30 with Kn = 4 (the slab copy loops over the lanes), M = 70 (the rank loop
exceeds the workgroup), S = 512 (four wavefronts), Kn = 8 (more than a swarm of 5 has mates), a NaN drone and Ks = 0."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mppi_tracks_checks as tk  # noqa: E402
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
# N, S, swarms, M, Kn, Ks, cycles, substeps, nan_drone
CHAIN = [(6, 64, 2, 5, 3, 2, 2, 3, None), (30, 64, 1, 5, 4, 2, 2, 3, None), (6, 64, 1, 70, 3, 0, 2, 1, None), (6, 512, 1, 5, 3, 2, 2, 3, None),
         (6, 64, 2, 5, 8, 2, 2, 3, None), (6, 64, 2, 5, 3, 2, 2, 3, 6), (6, 64, 2, 5, 3, 0, 3, 3, None)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,nprob,K", [(6, 64, 3, 2), (13, 320, 3, 0)])
def test_no_tracks_is_the_moving_planner(gpu_ops, dt, N, S, nprob, K):
    tk.check_no_tracks_is_the_moving_planner(harness(gpu_ops, dt), N, S, nprob, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K", [(6, 3, 2), (13, 3, 0)])
def test_no_tracks_is_the_moving_loop(gpu_ops, dt, N, B, K):
    tk.check_no_tracks_is_the_moving_loop(harness(gpu_ops, dt), N, B, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,nprob,K,Kt", [(6, 64, 3, 2, 3), (13, 320, 3, 0, 1), (1, 64, 3, 1, 16)])
def test_held_tracks_are_still_spheres_planner(gpu_ops, dt, N, S, nprob, K, Kt):
    tk.check_held_tracks_are_still_spheres_planner(harness(gpu_ops, dt), N, S, nprob, K, Kt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,Kt", [(6, 3, 2, 3), (13, 3, 0, 1)])
def test_held_tracks_are_still_spheres_loop(gpu_ops, dt, N, B, K, Kt):
    tk.check_held_tracks_are_still_spheres_loop(harness(gpu_ops, dt), N, B, K, Kt)


@pytest.mark.parametrize("dt", DTYPES)
def test_unshared_plans_are_the_swarm_call(gpu_ops, dt):
    tk.check_unshared_plans_are_the_swarm_call(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,nprob,iters,K,Kt", [(6, 64, 3, 2, 2, 3), (13, 64, 3, 2, 0, 1), (6, 320, 2, 2, 1, 16)])
def test_planner_against_the_oracle(gpu_ops, dt, N, S, nprob, iters, K, Kt):
    tk.check_against_oracle(harness(gpu_ops, dt), N, S, nprob, iters, K, Kt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", [(6, 10), (30, 70), (1, 3)])
def test_intent_is_the_rollout_of_the_nominal(gpu_ops, dt, N, B):
    tk.check_intent(harness(gpu_ops, dt), N, B)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,swarms,M,Kn,Ks,cycles,substeps,nan_drone", CHAIN)
def test_equals_the_chain_of_intent_and_tracks_entries(gpu_ops, dt, N, S, swarms, M, Kn, Ks, cycles, substeps, nan_drone):
    tk.check_chain(harness(gpu_ops, dt), N, S, swarms, M, Kn, Ks, cycles=cycles, substeps=substeps, nan_drone=nan_drone, mates_matter=M == 5)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_intent_reaches_the_planner(gpu_ops, dt):
    tk.check_intent_reaches_the_planner(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_continuation_determinism_and_dirty_buffers(gpu_ops, dt):
    tk.check_continuation_and_determinism(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_tracks_entries_determinism_and_dirty_buffers(gpu_ops, dt):
    tk.check_tracks_determinism_and_dirty_buffers(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(gpu_ops, dt):
    tk.check_invalid_arguments(harness(gpu_ops, dt))


def _planner(N, dt=0.1):
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=N), device="cuda:0")
    pl.se3_config = SE3MPCConfig(**{**pl.se3_config.__dict__, "dt": dt})
    return pl


@pytest.mark.parametrize("dt", DTYPES)
def test_front_end(gpu_ops, dt):
    tk.check_front_end(harness(gpu_ops, dt), _planner)


@pytest.mark.parametrize("dt", DTYPES)
def test_shared_plans_part_the_drones_no_less_often(gpu_ops, dt):
    tk.check_behaviour(harness(gpu_ops, dt))
