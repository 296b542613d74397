"""Mirror of the reference's ``dart_planner.control.trajectory_smoother.TrajectorySmoother`` (src/dart_planner/control/
trajectory_smoother.py), one drone: same constructor, public members and method names; the state lives in a one-drone device record
(SE3MPC_SMOOTHER_STATE_WORDS doubles, include/se3mpc.h) and every number comes from the kernels of ``csrc/smoother.hip``
(``se3mpc_smoother_update_*`` / ``se3mpc_smoother_desired_*``).  ``time.time()`` is read where the reference reads it.

The members of the reference that hold numbers (``last_filtered_pos``, ``in_transition``, ``last_cloud_update``, ...) are properties that
read the record; assigning one writes it.  The private methods are the same two kernels on a scratch copy of the record prepared so that
only the wanted part of ``get_desired_state`` runs (the docstrings say how); two of them have a narrower domain than the reference's
and raise outside it instead of answering from the host.

For B drones at once, and for the control-rate loop in one launch, use ``Ops.smoother_update`` / ``smoother_desired`` /
``closed_loop_smoothed`` directly (``dart_planner_amd/control/closed_loop.py``)."""
import math
import time
from typing import Optional, Tuple

import numpy as np

from ..capi import SMOOTHER_STATE_WORDS, SmootherParams
from ..common.types import DroneState, Trajectory
from ..common.units import to_float

_VEC = dict(last_filtered_pos=0, last_filtered_vel=3, last_filtered_acc=6, transition_start_pos=9, transition_start_vel=12,
            transition_target_pos=15, transition_target_vel=18)
_SCALAR = dict(transition_start_time=21, last_cloud_update=22, trajectory_start_time=23)


class TrajectorySmoother:
    """smoother.py:11-354 on the device, one drone."""

    def __init__(self, transition_time: float = 0.5, smoothing_factor: float = 0.8, *, precision: str = "f64", device=None):
        self.transition_time = transition_time
        self.smoothing_factor = smoothing_factor          # kept as the reference keeps it: no statement of the class reads it
        self.velocity_limit = 5.0                         # smoother.py:24-26
        self.acceleration_limit = 3.0
        self.jerk_limit = 10.0
        self._trajectory: Optional[Trajectory] = None     # current_trajectory (a property: the record's bit 1 and _plan follow it)
        self.precision = precision
        self._device = device
        self._ops = None
        self._state = None
        self._plan = None                                 # device tensors of current_trajectory: (timestamps, P, V, A)

    # ------------------------------------------------------------------ device plumbing
    def _get_ops(self):
        if self._ops is None:
            from ..ops import Ops, TorchBackend
            self._ops = Ops(TorchBackend(self._device))      # raises without a HIP device / built library
        return self._ops

    def _dev(self, a, kind=None):
        dt = {"f32": np.float32, "f64": np.float64}[kind or self.precision]
        return self._get_ops().be.from_host(np.ascontiguousarray(np.asarray(to_float(a), dtype=float).astype(dt)))

    def _params(self, **overrides) -> SmootherParams:
        return SmootherParams.reference_defaults(**{**dict(transition_time=self.transition_time, velocity_limit=self.velocity_limit,
                                                           acceleration_limit=self.acceleration_limit, jerk_limit=self.jerk_limit), **overrides})

    def _members(self):
        if self._state is None:
            self._state = self._get_ops().smoother_state(1)
        return self._state

    def _record(self) -> np.ndarray:
        return np.array(self._get_ops().be.to_host(self._members()), dtype=float).reshape(SMOOTHER_STATE_WORDS)

    def _write_record(self, rec: np.ndarray) -> None:
        self._state = self._get_ops().be.from_host(np.ascontiguousarray(np.asarray(rec, float).reshape(1, SMOOTHER_STATE_WORDS)))

    def _scratch(self, **words):
        rec = self._record()
        for k, v in words.items():
            if k in _VEC:
                rec[_VEC[k]:_VEC[k] + 3] = v
            elif k in _SCALAR:
                rec[_SCALAR[k]] = v
            else:
                rec[24] = v
        return self._get_ops().be.from_host(rec.reshape(1, SMOOTHER_STATE_WORDS))

    def _plan_of(self, trajectory: Optional[Trajectory]):
        if trajectory is None:
            return None
        opt = lambda a: None if a is None else self._dev(np.asarray(to_float(a), float).reshape(-1, 3))
        return (self._dev(np.asarray(to_float(trajectory.timestamps), float).reshape(-1), "f64"),
                self._dev(np.asarray(to_float(trajectory.positions), float).reshape(-1, 3)), opt(trajectory.velocities), opt(trajectory.accelerations))

    def _desired(self, params, record, current_time, position, velocity, plan):
        ops = self._get_ops()
        if plan is None:                                  # no plan: an empty one, which no branch that is reachable then reads
            plan = (self._dev(np.zeros(0), "f64"), self._dev(np.zeros((0, 3))), None, None)
        out = ops.smoother_desired(params, record, self._dev([float(current_time)], "f64"), self._dev(np.asarray(to_float(position), float).reshape(1, 3)),
                                   self._dev(np.asarray(to_float(velocity), float).reshape(1, 3)), *plan)
        x = np.array(ops.be.to_host(out["target"]), dtype=float).reshape(9)
        return (x[0:3].copy(), x[3:6].copy(), x[6:9].copy()), int(ops.be.to_host(out["branch"])[0])

    # ------------------------------------------------------------------ the reference's interface
    def update_trajectory(self, new_trajectory: Trajectory, current_state: DroneState):
        """update_trajectory (smoother.py:115-165)."""
        current_time = time.time()                        # :122
        new_plan = self._plan_of(new_trajectory)
        self._get_ops().smoother_update(self._params(), self._members(), self._dev([current_time], "f64"), *new_plan, old=self._plan)
        self._trajectory, self._plan = new_trajectory, new_plan      # (the kernel has set the record's bit 1)

    def get_desired_state(self, current_time: float, current_state: DroneState) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """get_desired_state (smoother.py:167-213)."""
        return self._desired(self._params(), self._members(), current_time, current_state.position, current_state.velocity, self._plan)[0]

    def is_trajectory_valid(self) -> bool:                # :340-345
        return self.current_trajectory is not None and time.time() - self.last_cloud_update < 2.0

    def get_status(self) -> dict:                         # :347-354
        return {"has_trajectory": self.current_trajectory is not None, "in_transition": self.in_transition,
                "last_update_age": time.time() - self.last_cloud_update, "trajectory_valid": self.is_trajectory_valid()}

    # ------------------------------------------------------------------ the private methods
    _INF = float("inf")

    def _interpolate_trajectory(self, current_time: float, trajectory: Trajectory, start_time: float):
        """_interpolate_trajectory (:215-278): normal following on a scratch record with that start time, no transition, the filter
        bypassed (filtered position at the origin) and every limit infinite."""
        rec = self._scratch(trajectory_start_time=float(start_time), last_cloud_update=float(current_time), bits=1.0,
                            last_filtered_pos=0.0, last_filtered_vel=0.0, last_filtered_acc=0.0)
        prm = self._params(velocity_limit=self._INF, acceleration_limit=self._INF, jerk_limit=self._INF)
        return self._desired(prm, rec, current_time, np.zeros(3), np.zeros(3), self._plan_of(trajectory))[0]

    def _generate_transition_state(self, progress: float):
        """_generate_transition_state (:280-319): the transition branch on a scratch record whose transition started `progress` transition
        times ago, with the filter bypassed and the per-call limits lifted by making one update step a day long (velocity_limit * dt and
        acceleration_limit * dt, :71 / :79, then exceed any change and jerk = change / dt falls under its limit); the two norm clamps of
        the transition keep self's limits.  The kernel forms (now - start) / transition_time, so the progress it sees can differ from the
        argument in the last bit; a progress at or past 1 is evaluated at the largest double below 1 (:285 clips there)."""
        p = float(progress)
        if not p < 1.0:
            p = math.nextafter(1.0, 0.0)
        now = p * self.transition_time
        rec = self._scratch(transition_start_time=0.0, last_cloud_update=now, bits=3.0, last_filtered_pos=0.0, last_filtered_vel=0.0,
                            last_filtered_acc=0.0)
        return self._desired(self._params(update_dt=86400.0, smoothing_window=86400.0), rec, now, np.zeros(3), np.zeros(3), None)[0]

    def _get_failsafe_trajectory(self, current_time: float, current_state: DroneState):
        """_get_failsafe_trajectory (:321-338), defined here where get_desired_state calls it: more than 2 s after the last update."""
        rec = self._scratch()
        out, branch = self._desired(self._params(), rec, current_time, current_state.position, current_state.velocity, self._plan)
        if branch != 0:
            raise ValueError("_get_failsafe_trajectory: current_time is not past the 2 s timeout (the device computes the failsafe only there)")
        return out

    def _smooth_trajectory_point(self, pos, vel, acc, dt: float):
        """_smooth_trajectory_point (:94-113): normal following of a one-row plan (pos, vel, acc) with update_dt = dt on self's record (the
        filter state moves, as in the reference); dt > 0."""
        t = self.last_cloud_update
        plan = (self._dev([0.0], "f64"), self._dev(np.asarray(to_float(pos), float).reshape(1, 3)), self._dev(np.asarray(to_float(vel), float).reshape(1, 3)),
                self._dev(np.asarray(to_float(acc), float).reshape(1, 3)))
        rec = self._scratch(bits=1.0)
        out, _ = self._desired(self._params(update_dt=float(dt), timeout=self._INF), rec, t, np.zeros(3), np.zeros(3), plan)
        keep = self._record()
        keep[0:9] = np.array(self._get_ops().be.to_host(rec), dtype=float).reshape(-1)[0:9]
        self._write_record(keep)
        return out

    def _apply_trajectory_limits(self, pos, vel, acc, dt: float):
        """_apply_trajectory_limits (:64-92): as _smooth_trajectory_point on a scratch record with the filter bypassed (filtered position at
        the origin); self's record is not touched; dt > 0."""
        plan = (self._dev([0.0], "f64"), self._dev(np.asarray(to_float(pos), float).reshape(1, 3)), self._dev(np.asarray(to_float(vel), float).reshape(1, 3)),
                self._dev(np.asarray(to_float(acc), float).reshape(1, 3)))
        rec = self._scratch(bits=1.0, last_filtered_pos=0.0)
        return self._desired(self._params(update_dt=float(dt), timeout=self._INF), rec, self.last_cloud_update, np.zeros(3), np.zeros(3), plan)[0]

    def _create_butterworth_filter(self, cutoff_freq: float = 2.0, order: int = 2):
        """:56-62.  Host-side coefficients of filters the class builds and never applies (needs scipy)."""
        from scipy import signal
        b, a = signal.butter(order, cutoff_freq / 50.0, btype="low", analog=False)
        return {"b": b, "a": a, "zi": signal.lfilter_zi(b, a)}

    @property
    def position_filter(self):
        return self._create_butterworth_filter()

    @property
    def velocity_filter(self):
        return self._create_butterworth_filter()

    @property
    def current_trajectory(self) -> Optional[Trajectory]:
        return self._trajectory

    @current_trajectory.setter
    def current_trajectory(self, value: Optional[Trajectory]) -> None:
        """Assigned directly, as code written against the reference may: the device plan and the record's "has a trajectory" bit follow;
        the clocks stay as they are, as in the reference."""
        self._trajectory, self._plan = value, self._plan_of(value)
        if value is not None or self._state is not None:
            rec = self._record()
            rec[24] = (int(rec[24]) & ~1) | (1 if value is not None else 0)
            self._write_record(rec)

    @property
    def in_transition(self) -> bool:
        return bool(int(self._record()[24]) & 2)

    @in_transition.setter
    def in_transition(self, value) -> None:
        rec = self._record()
        rec[24] = (int(rec[24]) & ~2) | (2 if value else 0)
        self._write_record(rec)


def _vec_member(off):
    def get(self):
        return self._record()[off:off + 3].copy()

    def set_(self, value):
        rec = self._record()
        rec[off:off + 3] = np.asarray(to_float(value), float)
        self._write_record(rec)
    return property(get, set_)


def _scalar_member(off):
    def get(self):
        return float(self._record()[off])

    def set_(self, value):
        rec = self._record()
        rec[off] = float(value)
        self._write_record(rec)
    return property(get, set_)


for _name, _off in _VEC.items():
    setattr(TrajectorySmoother, _name, _vec_member(_off))
for _name, _off in _SCALAR.items():
    setattr(TrajectorySmoother, _name, _scalar_member(_off))
