"""CPU suite: the edge-loop kernels of dart_planner_amd/csrc/edge_loop.hip (latency buffer, OnboardController, the loop) compiled for the host by
tests/emu and driven through the C ABI, Ops, ClosedLoopMonteCarlo.run_edge and the mirror classes: the checks of tests/edge_checks.py; and, on the
oracle alone, the discarded share of the random batches and the float32 loop bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402
from numpy_backend import TorchCpuBackend  # noqa: E402

from dart_planner_amd import capi  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402
import parity_checks as pc  # noqa: E402
import edge_checks as ec  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), dt)


DTYPES = [np.float64, np.float32]


def test_oracle_alone_discards_little_and_sets_the_float32_loop_bound():
    """The generator's inputs keep the oracle's own decisions away from their thresholds (at most 5 % of the (drone, step) cases within 1e-6), and
    the float32 bounds of edge_checks.py (loops, and the calls of each golden sequence) are 4 x what the oracle measures here between float64 and float32 -- no more."""
    worst, discarded = ec.measure_f32_loop_difference()
    print("float64 / float32 oracle difference over the loops:", worst, "largest discarded share:", discarded)
    assert discarded <= ec.MAX_DISCARDED
    for k, v in worst.items():           # (within a quarter either way: NumPy's float32 sin / cos differ in the last bit from one CPU to the next)
        assert v <= 1.25 * ec.F32_LOOP_MEASURED[k] and ec.F32_LOOP_MEASURED[k] <= 1.25 * v, (k, v, ec.F32_LOOP_MEASURED[k])
        assert ec.F32_LOOP_TOL[k] == 4.0 * ec.F32_LOOP_MEASURED[k]
    calls = ec.measure_f32_call_difference()
    print("float64 / float32 oracle difference over the calls of each golden sequence:", calls)
    assert set(calls) == set(ec.F32_CALL_MEASURED)
    for k, v in calls.items():
        assert v <= 1.25 * ec.F32_CALL_MEASURED[k] and ec.F32_CALL_MEASURED[k] <= 1.25 * v, (k, v, ec.F32_CALL_MEASURED[k])
        assert ec.F32_CALL_TOL[k] == 4.0 * ec.F32_CALL_MEASURED[k]


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_sequences_through_the_c_abi(emu_ops, dt):
    ec.check_golden_sequences(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_golden_closed_loops(emu_ops, dt):
    ec.check_golden_loops(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ec.BATCHES, ids=lambda c: "B%d-depth%d-N%d-%s%s%s-n%d" % (c[0], c[1], c[2], "s" if c[3] else "p", "V" if c[4] else "", "A" if c[5] else "", c[6]))
def test_random_batches_against_the_oracle(emu_ops, dt, case):
    ec.check_random_batch(harness(emu_ops, dt), case)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,depth,nsteps", [(65, 5, 23), (130, 2, 7), (64, 1, 5)])
def test_one_launch_equals_chained_launches_bit_for_bit(emu_ops, dt, B, depth, nsteps):
    ec.check_bit_for_bit(harness(emu_ops, dt), B, depth, nsteps)


@pytest.mark.parametrize("dt", DTYPES)
def test_split_launches_equal_the_whole_run(emu_ops, dt):
    ec.check_split_launches(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_differing_ring_positions_inside_a_wavefront(emu_ops, dt):
    ec.check_differing_ring_positions(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_run_edge_equals_its_hand_chained_form(emu_ops, dt):
    ec.check_run_edge(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_mirror_classes(emu_ops, dt, monkeypatch):
    ec.check_mirror(harness(emu_ops, dt), monkeypatch)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(emu_ops, dt):
    ec.check_invalid_arguments(harness(emu_ops, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_dirty_buffers_and_nan_drone(emu_ops, dt):
    ec.check_dirty_buffers_and_nan_drone(harness(emu_ops, dt))
