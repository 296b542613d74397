"""GPU suite (`-m gpu`): the uncertainty-field kernels of dart_planner_amd/csrc/uncertainty_field.hip on a real MI355X through the C ABI, Ops and the
mirror class: the checks of tests/uncertainty_checks.py (grids of at most 5760 voxels)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_checks as pc  # noqa: E402
import uncertainty_checks as uc  # noqa: E402


@pytest.fixture(scope="module")
def gpu_ops():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend("cuda:0"))
    assert ops.lib.device_count() >= 1, "no gfx950 device visible to libse3mpc"
    assert os.path.basename(ops.lib.path) == "libse3mpc.so"
    return ops


def harness(ops):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"), lambda a: a.detach().cpu().numpy(), np.float64)


def test_golden_sequences_through_the_c_abi(gpu_ops):
    uc.check_golden_sequences(harness(gpu_ops))


@pytest.mark.parametrize("grid", ["g24", "g19"])
@pytest.mark.parametrize("mask", uc.MASKS)
def test_labelling_against_the_oracle(gpu_ops, grid, mask):
    uc.check_labelling(harness(gpu_ops), grid, mask)


def test_regions_and_statistics_are_deterministic(gpu_ops):
    uc.check_determinism(harness(gpu_ops))


def test_130_stamps_in_one_launch_equal_130_launches(gpu_ops):
    uc.check_batched_stamps_equal_single_launches(harness(gpu_ops))


@pytest.mark.parametrize("n,weighted", [(65, False), (130, True)])
def test_point_updates_in_input_order(gpu_ops, n, weighted):
    uc.check_point_updates(harness(gpu_ops), n, weighted)


def test_dirty_workspace(gpu_ops):
    uc.check_dirty_workspace(harness(gpu_ops))


def test_nan_uncertainties_stay_in_their_voxels(gpu_ops):
    uc.check_nan_voxels(harness(gpu_ops))


def test_invalid_arguments(gpu_ops):
    uc.check_invalid_arguments(harness(gpu_ops))


def test_behaviour_of_the_mirror_class(gpu_ops):
    uc.check_behaviour(harness(gpu_ops))
