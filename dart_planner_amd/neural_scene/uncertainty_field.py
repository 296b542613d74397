"""The reference's UncertaintyField (src/dart_planner/neural_scene/uncertainty_field.py, "field.py") with its grids in HBM and every number
computed by the kernels of dart_planner_amd/csrc/uncertainty_field.hip: same constructor, method names and signatures, the
same float64 results.  Beyond the reference: ``reduce_uncertainty_around_positions`` stamps B drones in one launch and
``get_uncertainty_at_positions`` answers B queries in one.

What stays on the host is what is not arithmetic: the 5-second refresh rule of ``get_exploration_targets`` and the ``last_updated`` stamps
(behind an injectable ``clock``), and the slicing of ``get_uncertainty_field_region``.  There is no CPU path: without the HIP library the
constructor raises ``capi.Se3mpcLibraryError``."""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional

import numpy as np

from ..ops import Ops

MAX_TARGETS = 1024      # num_targets of se3mpc_ufield_targets (include/se3mpc.h)

@dataclass
class UncertaintyRegion:
    """One row of se3mpc_ufield_regions as the record the reference's callers read (field.py:21-30): lengths in metres, `bounds` a (2, 3)
    array of the extreme voxel centres, `priority` = uncertainty_value * log(1 + volume), `last_updated` from the field's clock."""

    center: np.ndarray
    bounds: np.ndarray
    uncertainty_value: float
    volume: float
    priority: float
    last_updated: float


class UncertaintyField:
    def __init__(self, scene_bounds: np.ndarray, resolution: float, ops: Optional[Ops] = None, max_regions: int = 1024,
                 clock: Callable[[], float] = time.time):
        """scene_bounds: a (2, 3) array, the lower corner first; resolution: the voxel edge in metres (field.py:41-55).  max_regions: the rows
        the device keeps per region extraction (the first max_regions regions in discovery order; ``regions_found`` tells how many
        qualified)."""
        self.ops = ops if ops is not None else Ops()
        self.be = self.ops.be
        self.scene_bounds = scene_bounds
        self.resolution = resolution
        bounds = np.asarray(scene_bounds, dtype=np.float64)
        self.grid_size = np.ceil((bounds[1] - bounds[0]) / resolution).astype(int)                     # field.py:53-55
        n = tuple(int(v) for v in self.grid_size)
        self.max_regions = int(max_regions)
        self._clock = clock
        self._u = self.be.empty(n, "f64")
        self._c = self.be.empty(n, "f64")
        self._origin = bounds[0].copy()
        self._desc = self.ops.ufield_desc(self._u, self._c, self._origin, float(resolution))
        self._ws = self.ops.ufield_workspace(n, self.max_regions)
        self._labels = self.be.empty(n, "i32")
        self.ops.ufield_fill(self._desc)
        self.high_uncertainty_regions: List[UncertaintyRegion] = []
        self.uncertainty_threshold = 0.7
        self.last_region_update = 0.0
        self.regions_found = 0
        self._rows = None              # device rows and counts of the last extraction
        self._counts = None

    # ------------------------------------------------------------------ the grids
    @property
    def uncertainty_grid(self) -> np.ndarray:
        """A host copy of the uncertainty grid (synchronises)."""
        return np.array(self.be.to_host(self._u))

    @property
    def observation_count(self) -> np.ndarray:
        return np.array(self.be.to_host(self._c))

    @property
    def device_uncertainty(self):
        """The grid itself, on the device."""
        return self._u

    def _dev(self, a, shape):
        return self.be.from_host(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape)))

    # ------------------------------------------------------------------ updates
    def update_uncertainty_at_position(self, position: np.ndarray, uncertainty: float, observation_weight: float = 1.0):
        self.update_uncertainty_field(np.asarray(position, float).reshape(1, 3), np.array([uncertainty], float), np.array([observation_weight], float))

    def update_uncertainty_field(self, positions: np.ndarray, uncertainties: np.ndarray, weights: Optional[np.ndarray] = None):
        n = len(positions)
        if n == 0:
            return
        self.ops.ufield_update_points(self._desc, self._dev(positions, (n, 3)), self._dev(uncertainties, (n,)),
                                      None if weights is None else self._dev(weights, (n,)), alpha=0.1, workspace=self._ws)

    def reduce_uncertainty_around_position(self, position: np.ndarray, radius: float = 2.0, reduction_factor: float = 0.5):
        self.reduce_uncertainty_around_positions(np.asarray(position, float).reshape(1, 3), radius, reduction_factor)

    def reduce_uncertainty_around_positions(self, positions: np.ndarray, radius=2.0, reduction_factor=0.5):
        """B stamps in one launch, applied in row order: positions (B, 3); radius and reduction_factor scalars or (B,)."""
        positions = np.asarray(positions, float).reshape(-1, 3)
        B = len(positions)
        if B == 0:
            return
        radius = np.array(np.broadcast_to(np.asarray(radius, float), (B,)))
        factor = np.array(np.broadcast_to(np.asarray(reduction_factor, float), (B,)))
        voxels = np.array([int(r / self.resolution) for r in radius.tolist()], dtype=np.int32)       # field.py:234, Python float64
        self.ops.ufield_stamp(self._desc, self._dev(positions, (B, 3)), self._dev(radius, (B,)), self.be.from_host(voxels), self._dev(factor, (B,)))

    # ------------------------------------------------------------------ queries
    def get_uncertainty_at_position(self, position: np.ndarray) -> float:
        return float(self.get_uncertainty_at_positions(np.asarray(position, float).reshape(1, 3))[0])

    def get_uncertainty_at_positions(self, positions: np.ndarray) -> np.ndarray:
        positions = np.asarray(positions, float).reshape(-1, 3)
        if len(positions) == 0:
            return np.zeros(0)
        return np.array(self.be.to_host(self.ops.ufield_query(self._desc, self._dev(positions, (len(positions), 3)))))

    def get_uncertainty_field_region(self, bounds: np.ndarray) -> np.ndarray:
        bounds = np.asarray(bounds, float)
        min_idx = np.maximum(self._position_to_grid_index(bounds[0]), 0)                             # field.py:138-143
        max_idx = np.minimum(self._position_to_grid_index(bounds[1]), self.grid_size - 1)
        region = self._u[int(min_idx[0]):int(max_idx[0]) + 1, int(min_idx[1]):int(max_idx[1]) + 1, int(min_idx[2]):int(max_idx[2]) + 1]
        return np.array(self.be.to_host(region))

    def _position_to_grid_index(self, position: np.ndarray) -> np.ndarray:
        return np.floor((np.asarray(position, float) - self._origin) / self.resolution).astype(int)

    # ------------------------------------------------------------------ regions and targets
    def identify_high_uncertainty_regions(self, threshold: Optional[float] = None, min_volume: float = 1.0) -> List[UncertaintyRegion]:
        if threshold is None:
            threshold = self.uncertainty_threshold
        out = self.ops.ufield_regions(self._desc, threshold, min_volume, self.max_regions, workspace=self._ws, labels=self._labels)
        written, found = (int(v) for v in self.be.to_host(out["counts"]))
        rows = np.array(self.be.to_host(out["regions"]))[:written]
        now = self._clock()
        regions = [UncertaintyRegion(center=r[0:3].copy(), bounds=np.array([r[3:6], r[6:9]]), uncertainty_value=float(r[9]), volume=float(r[10]),
                                     priority=float(r[11]), last_updated=now) for r in rows]
        self._rows, self._counts = out["regions"], out["counts"]
        self.regions_found = found
        self.high_uncertainty_regions = regions
        self.last_region_update = self._clock()
        return regions

    def get_exploration_targets(self, num_targets: int = 5, current_position: Optional[np.ndarray] = None) -> List[np.ndarray]:
        if not self.high_uncertainty_regions or self._clock() - self.last_region_update > 5.0:       # field.py:198-202
            self.identify_high_uncertainty_regions()
        if not self.high_uncertainty_regions or num_targets <= 0:
            return []
        wanted = min(int(num_targets), len(self.high_uncertainty_regions))
        if wanted > MAX_TARGETS:
            raise ValueError(f"get_exploration_targets: {wanted} targets asked for, se3mpc_ufield_targets ranks at most {MAX_TARGETS} in one call")
        targets, n = self.ops.ufield_targets(self._rows, self._counts, wanted, current_position)
        count = int(self.be.to_host(n)[0])
        return [t.copy() for t in np.array(self.be.to_host(targets))[:count]]

    # ------------------------------------------------------------------ statistics
    def get_statistics(self) -> Dict[str, Any]:
        out = self.ops.ufield_statistics(self._desc, self.uncertainty_threshold, workspace=self._ws)
        observed, high = (int(v) for v in self.be.to_host(out["counts"]))
        total, lo, hi = (float(v) for v in self.be.to_host(out["values"]))
        total_voxels = int(np.prod(self.grid_size))
        return {
            "total_voxels": total_voxels,
            "observed_voxels": observed,
            "observation_coverage": float(observed / total_voxels),
            "high_uncertainty_voxels": high,
            "high_uncertainty_percentage": float(high / total_voxels * 100),
            "average_uncertainty": float(total / total_voxels),
            "min_uncertainty": lo,
            "max_uncertainty": hi,
            "uncertainty_regions": len(self.high_uncertainty_regions),
            "resolution": self.resolution,
            "grid_size": self.grid_size.tolist(),
        }
