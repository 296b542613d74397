"""GPU suite (`-m gpu`): the closed-loop MPPI Monte-Carlo of dart_planner_amd/csrc/mppi_closed_loop.hip on a real MI355X through the C ABI,
Ops and ClosedLoopMonteCarlo: the checks of tests/mppi_closed_loop_checks.py at device sizes -- several chunks of samples (S = 256, 1024),
N = 30, K = 16, both types."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mppi_closed_loop_checks as lc  # noqa: E402
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
@pytest.mark.parametrize("N,B,K,S,shift,wind", [(6, 5, 0, 64, 1, "per_drone"), (13, 4, 3, 256, 0, "shared"), (30, 4, 16, 1024, 30, None),
                                                (30, 67, 16, 256, 1, "per_drone"), (30, 5, 0, 320, 2, "shared")])
def test_cycles_in_one_call_equal_chained_calls(gpu_ops, dt, N, B, K, S, shift, wind):
    lc.check_cycle_equivalence(harness(gpu_ops, dt), N, B, K, S=S, shift=shift, wind=wind)


@pytest.mark.parametrize("dt", DTYPES)
def test_long_act_phase_runs_in_chunks(gpu_ops, dt):
    lc.check_cycle_equivalence(harness(gpu_ops, dt), 6, 3, 2, cycles=2, substeps=70, sim_dt=0.002)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,S", [(6, 3, 0, 64), (30, 4, 16, 256), (30, 3, 0, 1024)])
def test_planner_inside_is_the_planner_outside(gpu_ops, dt, N, B, K, S):
    lc.check_planner_inside(harness(gpu_ops, dt), N, B, K, S=S)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B,K,S", [(6, 4, 0, 64), (13, 3, 3, 256), (30, 3, 16, 256), (30, 2, 0, 1024)])
def test_against_the_float64_chain_cycle_by_cycle(gpu_ops, dt, N, B, K, S):
    lc.check_against_oracle(harness(gpu_ops, dt), N, B, K, S=S)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_penalty_keeps_every_drone_clear_of_the_sphere(gpu_ops, dt):
    lc.check_behaviour(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_determinism_dirty_buffers_and_nan_drone(gpu_ops, dt):
    lc.check_determinism_and_dirty_buffers(harness(gpu_ops, dt), N=30, B=5, K=16)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(gpu_ops, dt):
    lc.check_invalid_arguments(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_front_end(gpu_ops, dt):
    lc.check_front_end(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_a_different_constant_in_every_block(gpu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    b = ps.loop_blocks(L["N"], dt=0.1)
    kw = dict(prm=b["prm"], cp=b["cp"], sp=b["sp"], ccfg=b["ccfg"], sim=b["sim"])
    lc.check_cycle_equivalence(harness(gpu_ops, dt), L["N"], L["B"], L["K"], cycles=L["cycles"], substeps=L["substeps"], **kw)
    lc.check_planner_inside(harness(gpu_ops, dt), L["N"], L["B"], L["K"], substeps=L["substeps"], **kw)
    lc.check_against_oracle(harness(gpu_ops, dt), L["N"], L["B"], L["K"], cycles=L["cycles"], substeps=L["substeps"], **kw)
