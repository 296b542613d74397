"""GPU suite (`-m gpu`): the edge-loop kernels of dart_planner_amd/csrc/edge_loop.hip (latency buffer, OnboardController, the loop) on a real MI355X
through the C ABI, Ops, ClosedLoopMonteCarlo.run_edge and the mirror classes: the checks of tests/edge_checks.py (at most 130 drones x 300 steps)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_checks as pc  # noqa: E402
import edge_checks as ec  # noqa: E402


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
def test_golden_sequences_through_the_c_abi(gpu_ops, dt):
    ec.check_golden_sequences(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_closed_loops(gpu_ops, dt):
    ec.check_golden_loops(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ec.BATCHES, ids=lambda c: "B%d-depth%d-N%d-%s%s%s-n%d" % (c[0], c[1], c[2], "s" if c[3] else "p", "V" if c[4] else "", "A" if c[5] else "", c[6]))
def test_random_batches_against_the_oracle(gpu_ops, dt, case):
    ec.check_random_batch(harness(gpu_ops, dt), case)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,depth,nsteps", [(65, 5, 23), (130, 2, 7), (64, 1, 5)])
def test_one_launch_equals_chained_launches_bit_for_bit(gpu_ops, dt, B, depth, nsteps):
    ec.check_bit_for_bit(harness(gpu_ops, dt), B, depth, nsteps)


@pytest.mark.parametrize("dt", DTYPES)
def test_split_launches_equal_the_whole_run(gpu_ops, dt):
    ec.check_split_launches(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_differing_ring_positions_inside_a_wavefront(gpu_ops, dt):
    ec.check_differing_ring_positions(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_run_edge_equals_its_hand_chained_form(gpu_ops, dt):
    ec.check_run_edge(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_mirror_classes(gpu_ops, dt, monkeypatch):
    ec.check_mirror(harness(gpu_ops, dt), monkeypatch)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(gpu_ops, dt):
    ec.check_invalid_arguments(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_dirty_buffers_and_nan_drone(gpu_ops, dt):
    ec.check_dirty_buffers_and_nan_drone(harness(gpu_ops, dt))
