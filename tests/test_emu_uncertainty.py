"""CPU suite: the uncertainty-field kernels of dart_planner_amd/csrc/uncertainty_field.hip compiled for the host by tests/emu and driven through the
C ABI, Ops and the mirror class: the checks of tests/uncertainty_checks.py."""
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
import uncertainty_checks as uc  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), np.float64)


def test_golden_sequences_through_the_c_abi(emu_ops):
    uc.check_golden_sequences(harness(emu_ops))


@pytest.mark.parametrize("grid", ["g24", "g19"])
@pytest.mark.parametrize("mask", uc.MASKS)
def test_labelling_against_the_oracle(emu_ops, grid, mask):
    uc.check_labelling(harness(emu_ops), grid, mask)


def test_regions_and_statistics_are_deterministic(emu_ops):
    uc.check_determinism(harness(emu_ops))


def test_130_stamps_in_one_launch_equal_130_launches(emu_ops):
    uc.check_batched_stamps_equal_single_launches(harness(emu_ops))


@pytest.mark.parametrize("n,weighted", [(65, False), (130, True)])
def test_point_updates_in_input_order(emu_ops, n, weighted):
    uc.check_point_updates(harness(emu_ops), n, weighted)


def test_dirty_workspace(emu_ops):
    uc.check_dirty_workspace(harness(emu_ops))


def test_nan_uncertainties_stay_in_their_voxels(emu_ops):
    uc.check_nan_voxels(harness(emu_ops))


def test_invalid_arguments(emu_ops):
    uc.check_invalid_arguments(harness(emu_ops))


def test_behaviour_of_the_mirror_class(emu_ops):
    uc.check_behaviour(harness(emu_ops))
