"""The reference's GlobalMissionPlanner (src/dart_planner/planning/global_mission_planner.py, "mission.py") with its phase machine on the
device: same class, method and attribute names, and every goal computed by ``se3mpc_mission_goal_*`` -- one B = 1 call per
``get_current_goal``, with ``now`` from the wall clock as in the reference (an injectable ``clock``).  The planner's mutable members (phase,
waypoint index, time of the last global plan, plans made) are one mission record on the device; ``current_phase`` and
``current_waypoint_index`` read and write it.  With ``use_neural_scene`` the stamp of every global plan goes to the mirror's own
UncertaintyField through ``se3mpc_ufield_stamp``.

Not reproduced (mission.py:433-442, :462-465, and neural_scene/base_neural_scene.py): the np.random-simulated high-uncertainty regions, the
region-uncertainty placeholder and PlaceholderNeuralScene -- ``high_uncertainty_regions`` stays empty, EXPLORATION always takes its systematic
branch, and ``neural_scene_updates`` of the status is the number of global plans, which is what the placeholder counts.  For B drones per
launch drive ``Ops.mission_goal`` or ``ClosedLoopMonteCarlo.run_mission``.  There is no CPU path."""
from __future__ import annotations

import time
from dataclasses import dataclass
from enum import Enum
from typing import Any, Callable, Dict, List, Optional

import numpy as np

from ..capi import MISSION_LABELS, MISSION_PHASES, MissionParams
from ..common.units import Q_, ensure_units, to_float
from ..neural_scene.uncertainty_field import UncertaintyField
from ..ops import Ops


class MissionPhase(Enum):
    """mission.py:17-25; the record's phase code is the position in this order."""

    TAKEOFF = "takeoff"
    EXPLORATION = "exploration"
    MAPPING = "mapping"
    NAVIGATION = "navigation"
    LANDING = "landing"
    EMERGENCY = "emergency"


assert tuple(p.value for p in MissionPhase) == MISSION_PHASES


@dataclass
class SemanticWaypoint:
    """mission.py:28-38."""

    position: np.ndarray
    semantic_label: str
    uncertainty: float
    priority: int

    def __post_init__(self):
        self.position = ensure_units(self.position, "m", "SemanticWaypoint.position")


@dataclass
class GlobalMissionConfig:
    """mission.py:41-68, lengths as SI magnitudes."""

    exploration_radius: Any = 50.0
    mapping_resolution: Any = 0.5
    safety_margin: Any = 2.0
    use_neural_scene: bool = True
    nerf_update_frequency: float = 0.1
    uncertainty_threshold: float = 0.7
    enable_multi_agent: bool = False
    communication_range: Any = 100.0
    global_replan_frequency: float = 1.0
    waypoint_update_frequency: float = 2.0

    def __post_init__(self):
        for name in ("exploration_radius", "mapping_resolution", "safety_margin", "communication_range"):
            object.__setattr__(self, name, ensure_units(getattr(self, name), "m", f"GlobalMissionConfig.{name}"))


class GlobalMissionPlanner:
    def __init__(self, config: Optional[GlobalMissionConfig] = None, ops: Optional[Ops] = None, clock: Callable[[], float] = time.time,
                 uncertainty_field: Optional[UncertaintyField] = None):
        """config: mission.py:91-92.  uncertainty_field: the field the global plans stamp (None with use_neural_scene: the reference's own,
        exploration_radius around the origin up to 20 m at mapping_resolution, mission.py:121-138)."""
        self.config = config if config else GlobalMissionConfig()
        self.ops = ops if ops is not None else Ops()
        self.be = self.ops.be
        self._clock = clock
        self.params = MissionParams.reference_defaults(safety_margin=float(to_float(self.config.safety_margin)),
                                                       exploration_radius=float(to_float(self.config.exploration_radius)),
                                                       global_replan_period=1.0 / self.config.global_replan_frequency,
                                                       use_neural_scene=bool(self.config.use_neural_scene))
        self.mission_waypoints: List[SemanticWaypoint] = []
        self.neural_scene_model = None
        self.uncertainty_field = None
        if self.config.use_neural_scene:
            r = float(to_float(self.config.exploration_radius))
            self.uncertainty_field = uncertainty_field if uncertainty_field is not None else UncertaintyField(
                np.array([[-r, -r, 0.0], [r, r, 20.0]]), float(to_float(self.config.mapping_resolution)), ops=self.ops)
        self.explored_regions: List[np.ndarray] = []
        self.high_uncertainty_regions: List[np.ndarray] = []
        self.planning_history: List[Dict[str, Any]] = []
        self._state = self.ops.mission_state(1)
        self._out = None
        self._table = self._pack([])

    # ------------------------------------------------------------------ the record
    def _record(self) -> np.ndarray:
        return np.array(self.be.to_host(self._state))[0]

    def _write(self, word: int, value: float) -> None:
        rec = self._record()
        rec[word] = value
        self._state = self.be.from_host(rec.reshape(1, -1))

    @property
    def current_phase(self) -> MissionPhase:
        return list(MissionPhase)[int(self._record()[0])]

    @current_phase.setter
    def current_phase(self, phase: MissionPhase) -> None:
        self._write(0, float(list(MissionPhase).index(MissionPhase(phase))))

    @property
    def current_waypoint_index(self) -> int:
        return int(self._record()[1])

    @current_waypoint_index.setter
    def current_waypoint_index(self, index: int) -> None:
        self._write(1, float(int(index)))

    @property
    def last_global_plan_time(self) -> float:
        return float(self._record()[2])

    @property
    def global_plans(self) -> int:
        return int(self._record()[3])

    # ------------------------------------------------------------------ mission.py:171-224
    def _pack(self, waypoints):
        pos = np.array([np.asarray(to_float(w.position), float) for w in waypoints], dtype=np.float64).reshape(-1, 3)
        lab = np.array([MISSION_LABELS.get(w.semantic_label, 0) for w in waypoints], dtype=np.int32)
        return self.be.from_host(pos), self.be.from_host(lab)

    def set_mission_waypoints(self, waypoints: List[SemanticWaypoint]):
        self.mission_waypoints = waypoints
        self._table = self._pack(waypoints)
        self.current_waypoint_index = 0

    def get_current_goal(self, current_state) -> np.ndarray:
        pos = np.asarray(to_float(current_state.position), dtype=np.float64).reshape(1, 3)
        now = self.be.from_host(np.array([float(self._clock())]))
        field = self.uncertainty_field
        self._out = self.ops.mission_goal(self.params, self._state, now, self.be.from_host(pos), *self._table,
                                          resolution=float(field.resolution) if field is not None else 1.0,
                                          goal=None if self._out is None else self._out["goal"], stamps=None if self._out is None else self._out["stamps"])
        if field is not None:
            s = self._out["stamps"]
            self.ops.ufield_stamp(field._desc, s["centres"], s["radius"], s["radius_voxels"], s["factor"])
        return Q_(np.array(self.be.to_host(self._out["goal"]))[0], "m")

    def get_mission_status(self) -> Dict[str, Any]:
        """mission.py:467-482; planning_history_length and neural_scene_updates count the global plans made."""
        plans = self.global_plans
        return {
            "current_phase": self.current_phase.value,
            "waypoint_progress": f"{self.current_waypoint_index}/{len(self.mission_waypoints)}",
            "neural_scene_updates": plans if self.config.use_neural_scene else 0,
            "uncertainty_regions": len(self.high_uncertainty_regions),
            "explored_regions": len(self.explored_regions),
            "planning_history_length": plans,
        }
