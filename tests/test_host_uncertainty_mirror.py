"""CPU: the host logic of the mirror class dart_planner_amd.neural_scene.UncertaintyField over the host-emulated kernels, with an injected
clock: the 5-second refresh rule of get_exploration_targets, min_volume, num_targets, last_updated, and the import shim."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402
from numpy_backend import TorchCpuBackend  # noqa: E402

from dart_planner_amd import capi  # noqa: E402
from dart_planner_amd.neural_scene import UncertaintyField, UncertaintyRegion  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402

BOUNDS = np.array([[-6.0, -5.0, 0.0], [6.0, 5.0, 6.0]])


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


class Clock:
    def __init__(self):
        self.t = 100.0

    def __call__(self):
        return self.t


def cubes(field):
    """a 27-voxel, a 12-voxel and a 1-voxel region in a field that is certain elsewhere"""
    field.reduce_uncertainty_around_position(np.array([0.0, 0.0, 3.0]), radius=30.0, reduction_factor=0.9)
    u = field.uncertainty_grid
    assert np.all(u < 0.7)
    u[2:5, 2:5, 2:5] = 0.95
    u[10:12, 9:12, 5:7] = 0.9
    u[20, 15, 10] = 0.8
    field._u.copy_(field.be.from_host(u))


def test_refresh_rule_min_volume_and_num_targets(emu_ops):
    clock = Clock()
    f = UncertaintyField(BOUNDS, 0.5, ops=emu_ops, max_regions=16, clock=clock)
    assert list(f.grid_size) == [24, 20, 12] and f.uncertainty_threshold == 0.7 and f.high_uncertainty_regions == [] and f.last_region_update == 0.0
    cubes(f)
    regions = f.identify_high_uncertainty_regions()                                 # min_volume 1.0: 8 voxels
    assert [r.volume for r in regions] == [27 * 0.125, 12 * 0.125] and all(isinstance(r, UncertaintyRegion) for r in regions)
    assert all(r.last_updated == 100.0 for r in regions) and f.last_region_update == 100.0 and f.regions_found == 2
    assert len(f.identify_high_uncertainty_regions(min_volume=0.1)) == 3 and len(f.identify_high_uncertainty_regions(threshold=0.92, min_volume=0.1)) == 1
    f.identify_high_uncertainty_regions()
    assert [len(f.get_exploration_targets(n)) for n in (0, 1, 2, 5)] == [0, 1, 2, 2]
    first = f.get_exploration_targets(5)
    assert regions[0].center[2] == 1.75 and np.array_equal(first[0], [regions[0].center[0], regions[0].center[1], 2.0])      # the 2 m floor
    assert np.array_equal(first[1], regions[1].center) and regions[1].center[2] == 3.0
    # within 5 s the cached regions answer, whatever happened to the grid since
    f.reduce_uncertainty_around_position(np.array([-4.25, -3.25, 1.75]), radius=1.5, reduction_factor=0.9)
    clock.t = 105.0
    assert len(f.get_exploration_targets(5)) == 2 and f.last_region_update == 100.0
    clock.t = 105.5                                                                  # later than 5 s: re-identified at the defaults
    again = f.get_exploration_targets(5)
    assert len(again) == 1 and f.last_region_update == 105.5 and f.high_uncertainty_regions[0].last_updated == 105.5
    assert f.get_statistics()["uncertainty_regions"] == 1
    # an empty cache is refreshed at every call
    empty = UncertaintyField(BOUNDS, 0.5, ops=emu_ops, max_regions=16, clock=clock)
    empty.reduce_uncertainty_around_position(np.array([0.0, 0.0, 3.0]), radius=30.0, reduction_factor=0.9)
    assert empty.get_exploration_targets(5) == [] and empty.last_region_update == 105.5
    clock.t = 106.0
    assert empty.get_exploration_targets(5) == [] and empty.last_region_update == 106.0


def test_more_regions_than_rows_is_visible(emu_ops):
    f = UncertaintyField(BOUNDS, 0.5, ops=emu_ops, max_regions=2, clock=Clock())
    cubes(f)
    regions = f.identify_high_uncertainty_regions(min_volume=0.1)
    assert len(regions) == 2 and f.regions_found == 3
    assert [r.volume for r in regions] == [27 * 0.125, 12 * 0.125]                   # the first two in discovery order, then by priority


def test_more_targets_than_one_call_ranks_is_an_error(emu_ops):
    f = UncertaintyField(np.array([[0.0, 0.0, 0.0], [17.0, 16.0, 4.0]]), 0.5, ops=emu_ops, max_regions=2048, clock=Clock())
    u = np.full(tuple(f.grid_size), 0.1)
    u[::2, ::2, ::2] = 0.9                                                          # 17 x 16 x 4 = 1088 single voxels
    f._u.copy_(f.be.from_host(u))
    assert len(f.identify_high_uncertainty_regions(min_volume=0.1)) == 1088 and f.regions_found == 1088
    assert len(f.get_exploration_targets(1024, np.zeros(3))) == 1024
    with pytest.raises(ValueError, match="at most 1024"):
        f.get_exploration_targets(2000)


def test_missing_library_raises(tmp_path):
    with pytest.raises(capi.Se3mpcLibraryError):
        UncertaintyField(BOUNDS, 0.5, ops=Ops(TorchCpuBackend(), capi.Library(str(tmp_path / "libse3mpc.so"))))


def test_import_shim():
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dart_planner_amd", "compat")
    sys.path.insert(0, compat)
    try:
        for m in [m for m in sys.modules if m == "dart_planner" or m.startswith("dart_planner.")]:
            del sys.modules[m]
        from dart_planner.neural_scene.uncertainty_field import UncertaintyField as Shimmed, UncertaintyRegion as ShimmedRegion
        assert Shimmed is UncertaintyField and ShimmedRegion is UncertaintyRegion
    finally:
        sys.path.remove(compat)
        for m in [m for m in sys.modules if m == "dart_planner" or m.startswith("dart_planner.")]:
            del sys.modules[m]
