"""ctypes binding of libse3mpc.so (include/se3mpc.h) -- raw pointers in, status codes out.

This is the only place the package touches the C ABI.  There is NO fallback: if the HIP library
has not been built (``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C dart_planner_amd/csrc``) loading raises :class:`Se3mpcLibraryError`.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIBRARY = os.path.join(_HERE, "libse3mpc.so")

SE3MPC_MAX_HORIZON = 64
SE3MPC_MAX_CORRECTIONS = 10
SE3MPC_MAX_SPHERES = 256
SE3MPC_MAX_TRACKS = 16

STATUS_NAMES = {0: "SE3MPC_OK", -1: "SE3MPC_ERR_NULL", -2: "SE3MPC_ERR_HORIZON", -3: "SE3MPC_ERR_SHAPE",
                -4: "SE3MPC_ERR_PARAM", -5: "SE3MPC_ERR_WORKSPACE", -6: "SE3MPC_ERR_LAUNCH",
                -7: "SE3MPC_ERR_NO_DEVICE"}
TASK_MESSAGES = {1: "CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL",
                 2: "CONVERGENCE: RELATIVE REDUCTION OF F <= FACTR*EPSMCH",
                 3: "STOP: TOTAL NO. OF ITERATIONS REACHED LIMIT",
                 4: "STOP: TOTAL NO. OF F,G EVALUATIONS EXCEEDS LIMIT",
                 5: "ABNORMAL: "}


class Se3mpcLibraryError(RuntimeError):
    """libse3mpc.so is missing or does not export the ABI of include/se3mpc.h."""


class Se3mpcError(RuntimeError):
    """A C-ABI call returned a negative status."""

    def __init__(self, fn: str, status: int, detail: str = ""):
        self.status = status
        super().__init__(f"{fn} -> {STATUS_NAMES.get(status, status)}" + (f": {detail}" if detail else ""))


class Params(C.Structure):
    """struct se3mpc_params (include/se3mpc.h) == SE3MPCConfig + ctor constants of the reference
    (src/dart_planner/planning/se3_mpc_planner.py:36-79, :149-151), unit-stripped."""
    _fields_ = [("horizon", C.c_int32), ("has_goal", C.c_int32), ("dt", C.c_double), ("mass", C.c_double),
                ("gravity", C.c_double), ("position_weight", C.c_double), ("velocity_weight", C.c_double),
                ("acceleration_weight", C.c_double), ("thrust_weight", C.c_double), ("terminal_factor", C.c_double),
                ("position_bound", C.c_double), ("max_velocity", C.c_double), ("max_acceleration", C.c_double),
                ("max_thrust", C.c_double), ("min_thrust", C.c_double), ("max_tilt_angle", C.c_double),
                ("safety_margin", C.c_double), ("max_iterations", C.c_int32), ("max_corrections", C.c_int32),
                ("max_linesearch", C.c_int32), ("max_fun", C.c_int32), ("pgtol", C.c_double), ("ftol", C.c_double)]

    @classmethod
    def reference_defaults(cls, **overrides) -> "Params":
        """The reference defaults, computed here the same way se3mpc_default_params() does (the
        test-suite checks the two agree)."""
        p = cls(horizon=6, has_goal=1, dt=1.0 / 400.0, mass=1.5, gravity=9.81, position_weight=100.0,
                velocity_weight=10.0, acceleration_weight=1.0, thrust_weight=0.1, terminal_factor=10.0,
                position_bound=100.0, max_velocity=10.0, max_acceleration=15.0, max_thrust=25.0, min_thrust=2.0,
                max_tilt_angle=math.pi / 4, safety_margin=1.5, max_iterations=15, max_corrections=10,
                max_linesearch=20, max_fun=15000, pgtol=0.05, ftol=0.5)
        names = cls._field_names()
        for k, v in overrides.items():
            if k not in names:
                raise AttributeError(f"se3mpc_params has no field {k!r}")
            setattr(p, k, v)
        return p

    @classmethod
    def _field_names(cls) -> frozenset:
        names = cls.__dict__.get("_names")
        if names is None:
            names = cls._names = frozenset(n for n, _ in cls._fields_)
        return names

    def copy(self, **overrides) -> "Params":
        q = Params()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(Params))
        for k, v in overrides.items():
            setattr(q, k, v)
        return q

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class SolveInfo(C.Structure):
    """struct se3mpc_solve_info."""
    _fields_ = [("fun", C.c_double), ("nit", C.c_int32), ("nfev", C.c_int32), ("status", C.c_int32),
                ("task", C.c_int32)]


class VoxelMapDesc(C.Structure):
    """struct se3mpc_voxel_map: the caller-owned hash table of the device voxel map (device addresses)."""
    _fields_ = [("keys", C.c_void_p), ("prob", C.c_void_p), ("count", C.c_void_p), ("capacity", C.c_int32),
                ("reserved", C.c_int32), ("resolution", C.c_double), ("prior", C.c_double)]


class UFieldDesc(C.Structure):
    """struct se3mpc_ufield: the caller-owned dense grids of the device uncertainty field (device addresses)."""
    _fields_ = [("uncertainty", C.c_void_p), ("observation_count", C.c_void_p), ("n", C.c_int32 * 3), ("reserved", C.c_int32),
                ("origin", C.c_double * 3), ("resolution", C.c_double)]


assert C.sizeof(UFieldDesc) == 64      # static_assert in csrc/uncertainty_field.hip


class ControllerParams(C.Structure):
    """struct se3mpc_controller_params == GeometricControllerConfig after its tuning profile
    (src/dart_planner/control/geometric_controller.py:26-77, :140-158), unit-stripped."""
    _fields_ = [("kp_pos", C.c_double * 3), ("ki_pos", C.c_double * 3), ("kd_pos", C.c_double * 3), ("kp_att", C.c_double * 3),
                ("kd_att", C.c_double * 3), ("inertia", C.c_double * 3), ("max_torque_xyz", C.c_double * 3),
                ("max_integral_per_axis", C.c_double * 3), ("max_integral_pos", C.c_double), ("max_tilt_angle", C.c_double),
                ("mass", C.c_double), ("gravity", C.c_double), ("max_thrust", C.c_double), ("min_thrust", C.c_double),
                ("tracking_error_threshold", C.c_double), ("velocity_error_threshold", C.c_double),
                ("back_calculation_gain", C.c_double), ("integral_decay_factor", C.c_double), ("saturation_threshold", C.c_double),
                ("yaw_singularity_threshold", C.c_double), ("default_heading_yaw", C.c_double),
                ("anti_windup_method", C.c_int32), ("yaw_fallback_method", C.c_int32)]
    ANTI_WINDUP = {"clamping": 0, "back_calculation": 1}
    YAW_FALLBACK = {"skip_yaw": 0, "default_heading": 1, "maintain_current": 2}

    @classmethod
    def from_config(cls, cfg) -> "ControllerParams":
        """From any object with GeometricControllerConfig's attribute names (the mirror's dataclass, the oracle's)."""
        p = cls()
        for name, ctype in cls._fields_:
            if name == "anti_windup_method":
                p.anti_windup_method = cls.ANTI_WINDUP.get(cfg.anti_windup_method, 2)
            elif name == "yaw_fallback_method":
                p.yaw_fallback_method = cls.YAW_FALLBACK.get(cfg.yaw_singularity_fallback_method, 3)
            elif ctype is C.c_double:
                setattr(p, name, float(getattr(cfg, name)))
            else:
                setattr(p, name, (C.c_double * 3)(*[float(v) for v in getattr(cfg, name)]))
        return p


class SimulatorParams(C.Structure):
    """struct se3mpc_simulator_params == DroneSimulator.__init__ (src/dart_planner/utils/drone_simulator.py:41-50)."""
    _fields_ = [("mass", C.c_double), ("gravity", C.c_double), ("inertia", C.c_double * 3), ("max_thrust", C.c_double),
                ("max_torque", C.c_double)]

    @classmethod
    def reference_defaults(cls, **overrides) -> "SimulatorParams":
        p = cls(mass=1.5, gravity=9.81, inertia=(C.c_double * 3)(0.1, 0.1, 0.2), max_thrust=20.0, max_torque=10.0)
        for k, v in overrides.items():
            setattr(p, k, v)
        return p


class SmootherParams(C.Structure):
    """struct se3mpc_smoother_params == the constants of TrajectorySmoother (src/dart_planner/control/trajectory_smoother.py:19-26,
    :101, :151, :176-179, :329-331)."""
    _fields_ = [("transition_time", C.c_double), ("velocity_limit", C.c_double), ("acceleration_limit", C.c_double),
                ("jerk_limit", C.c_double), ("update_dt", C.c_double), ("smoothing_window", C.c_double),
                ("pos_diff_threshold", C.c_double), ("vel_diff_threshold", C.c_double), ("timeout", C.c_double),
                ("decay_rate", C.c_double), ("decay_cap", C.c_double)]

    @classmethod
    def reference_defaults(cls, **overrides) -> "SmootherParams":
        p = cls(transition_time=0.5, velocity_limit=5.0, acceleration_limit=3.0, jerk_limit=10.0, update_dt=0.01, smoothing_window=0.1,
                pos_diff_threshold=0.5, vel_diff_threshold=1.0, timeout=2.0, decay_rate=2.0, decay_cap=5.0)
        for k, v in overrides.items():
            if k not in dict(cls._fields_):
                raise AttributeError(f"se3mpc_smoother_params has no field {k!r}")
            setattr(p, k, float(v))
        return p

    def copy(self, **overrides) -> "SmootherParams":
        return type(self).reference_defaults(**{**{k: getattr(self, k) for k, _ in self._fields_}, **overrides})


class MixerParams(C.Structure):
    """struct se3mpc_mixer_params == MotorMixer.inverse_matrix / mixing_matrix (src/dart_planner/hardware/motor_mixer.py:379-398, :152-166),
    the MotorParameters of motors 0..3 (src/dart_planner/hardware/motor_model.py:33-48), MotorMixingConfig's PWM limits (motor_mixer.py:64-66)
    and the constants of the Pixhawk loop (hardware/pixhawk_interface.py:413, :473, :482).  All doubles."""
    MOTOR_FIELDS = ("thrust_a", "thrust_b", "thrust_c", "pwm_min", "pwm_max", "pwm_idle", "torque_coefficient", "rpm_coefficient", "rpm_offset")
    SCALAR_FIELDS = ("config_pwm_min", "config_pwm_max", "config_pwm_idle", "max_thrust", "body_rate_scale", "watchdog_threshold")
    _fields_ = ([("inverse", C.c_double * 16), ("mixing", C.c_double * 16)] + [(n, C.c_double * 4) for n in MOTOR_FIELDS]
                + [(n, C.c_double) for n in SCALAR_FIELDS])

    @classmethod
    def from_matrices(cls, B, inverse, motors, config_pwm_min=0.0, config_pwm_max=1.0, config_pwm_idle=0.1, max_thrust=10.0,
                      body_rate_scale=2.0, watchdog_threshold=5.0) -> "MixerParams":
        """B, inverse: 4 x 4 (mixing_matrix, inverse_matrix); motors: four objects with MotorParameters' attribute names (or dicts)."""
        p = cls()
        for name, m in (("mixing", B), ("inverse", inverse)):
            flat = [float(v) for row in m for v in row]
            if len(flat) != 16:
                raise ValueError(f"{name}: a 4 x 4 matrix")
            setattr(p, name, (C.c_double * 16)(*flat))
        motors = list(motors)
        if len(motors) != 4:
            raise ValueError("motors: the parameters of motors 0..3")
        for name in cls.MOTOR_FIELDS:
            setattr(p, name, (C.c_double * 4)(*[float(m[name] if isinstance(m, dict) else getattr(m, name)) for m in motors]))
        p.config_pwm_min, p.config_pwm_max, p.config_pwm_idle = float(config_pwm_min), float(config_pwm_max), float(config_pwm_idle)
        p.max_thrust, p.body_rate_scale, p.watchdog_threshold = float(max_thrust), float(body_rate_scale), float(watchdog_threshold)
        return p

    @classmethod
    def reference_defaults(cls, **overrides) -> "MixerParams":
        """create_x_configuration_mixer(0.15) with create_default_motor_model() and the Pixhawk constants, computed here the way
        se3mpc_mixer_default_params() does (the test-suite checks the two agree); B's inverse by Gauss-Jordan with partial pivoting."""
        x = 0.15 * 0.707
        px, py, dirs = (x, x, -x, -x), (-x, x, x, -x), (1.0, -1.0, 1.0, -1.0)
        motor = dict(thrust_a=2.5, thrust_b=1.2, thrust_c=0.1, pwm_min=0.0, pwm_max=1.0, pwm_idle=0.1, torque_coefficient=1e-7,
                     rpm_coefficient=8000.0, rpm_offset=500.0)
        rpm = max(0.0, motor["rpm_coefficient"] * 1.0 + motor["rpm_offset"])
        k_drag = max(0.0, motor["torque_coefficient"] * (rpm * rpm)) / max(0.0, (motor["thrust_a"] * 1.0 + motor["thrust_b"] * 1.0) + motor["thrust_c"])
        Bm = [[1.0] * 4, list(py), list(px), [d * k_drag for d in dirs]]
        a = [row[:] + [1.0 if i == j else 0.0 for j in range(4)] for i, row in enumerate(Bm)]
        for k in range(4):
            piv = max(range(k, 4), key=lambda i: abs(a[i][k]))
            a[k], a[piv] = a[piv], a[k]
            a[k] = [v / a[k][k] for v in a[k]]
            for i in range(4):
                if i != k:
                    a[i] = [v - a[i][k] * w for v, w in zip(a[i], a[k])]
        p = cls.from_matrices(Bm, [row[4:] for row in a], [motor] * 4)
        return p.copy(**overrides) if overrides else p

    def copy(self, **overrides) -> "MixerParams":
        q = type(self)()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(type(self)))
        for k, v in overrides.items():
            if k not in dict(self._fields_):
                raise AttributeError(f"se3mpc_mixer_params has no field {k!r}")
            if k in self.SCALAR_FIELDS:
                setattr(q, k, float(v))
            else:
                flat = [float(x) for x in (v if k in self.MOTOR_FIELDS else [x for row in v for x in row])]
                setattr(q, k, (C.c_double * len(flat))(*flat))
        return q


assert C.sizeof(MixerParams) == 592       # static_assert of csrc/mixer_device.hpp


class OnboardParams(C.Structure):
    """struct se3mpc_onboard_params == OnboardController.__init__ (src/dart_planner/control/onboard_controller.py:25-35) and the first dt
    of sense (:139).  pid: rows pos_x, pos_y, pos_z, roll, pitch, yaw_rate; columns Kp, Ki, Kd, integral_limit (0 = no clamp)."""
    PID_ROWS = ("pos_x", "pos_y", "pos_z", "roll", "pitch", "yaw_rate")
    _fields_ = [("mass", C.c_double), ("g", C.c_double), ("pid", (C.c_double * 4) * 6), ("first_dt", C.c_double)]

    @classmethod
    def reference_defaults(cls, **overrides) -> "OnboardParams":
        """The reference defaults, computed here the way se3mpc_onboard_default_params() does (the test-suite checks the two agree).
        Overrides: mass, g, first_dt, or a PID row's name = (Kp, Ki, Kd, integral_limit)."""
        p = cls(mass=1.0, g=9.81, first_dt=0.01)
        rows = dict(pos_x=(10.0, 1.0, 5.0, 2.0), pos_y=(10.0, 1.0, 5.0, 2.0), pos_z=(12.0, 1.5, 6.0, 2.0), roll=(8.0, 0.0, 2.0, 1.0),
                    pitch=(8.0, 0.0, 2.0, 1.0), yaw_rate=(4.0, 0.0, 1.0, 0.5))
        for k, v in overrides.items():
            if k in rows:
                rows[k] = tuple(0.0 if x is None else float(x) for x in v)
            elif k in ("mass", "g", "first_dt"):
                setattr(p, k, float(v))
            else:
                raise AttributeError(f"se3mpc_onboard_params has no field {k!r}")
        for i, name in enumerate(cls.PID_ROWS):
            p.pid[i] = (C.c_double * 4)(*rows[name])
        return p

    def copy(self, **overrides) -> "OnboardParams":
        rows = {name: tuple(self.pid[i]) for i, name in enumerate(self.PID_ROWS)}
        return type(self).reference_defaults(**{**dict(mass=self.mass, g=self.g, first_dt=self.first_dt), **rows, **overrides})


assert C.sizeof(OnboardParams) == 216     # static_assert of csrc/edge_device.hpp


class MissionParams(C.Structure):
    """struct se3mpc_mission_params == the literals of GlobalMissionPlanner.get_current_goal and what it reads of GlobalMissionConfig
    (src/dart_planner/planning/global_mission_planner.py:46-60, :254-261, :322, :347, :358, :380, :411-413, :454)."""
    _fields_ = [(n, C.c_double) for n in ("safe_altitude", "takeoff_band", "waypoint_reach", "safety_margin", "landing_pad_lift", "landing_step",
                                         "landing_floor", "emergency_step", "emergency_floor", "emergency_altitude", "global_replan_period",
                                         "exploration_base", "exploration_radius", "stamp_radius", "stamp_factor")] + [
        ("use_neural_scene", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def reference_defaults(cls, **overrides) -> "MissionParams":
        """The reference's literals, computed here the way se3mpc_mission_default_params() does (the test-suite checks the two agree)."""
        p = cls(safe_altitude=5.0, takeoff_band=0.5, waypoint_reach=2.0, safety_margin=2.0, landing_pad_lift=3.0, landing_step=1.0, landing_floor=0.5,
                emergency_step=2.0, emergency_floor=0.0, emergency_altitude=0.5, global_replan_period=1.0 / 1.0, exploration_base=10.0,
                exploration_radius=50.0, stamp_radius=3.0, stamp_factor=0.2, use_neural_scene=1, reserved=0)
        return p.copy(**overrides) if overrides else p

    def copy(self, **overrides) -> "MissionParams":
        q = type(self)()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(type(self)))
        for k, v in overrides.items():
            if k not in dict(self._fields_):
                raise AttributeError(f"se3mpc_mission_params has no field {k!r}")
            setattr(q, k, int(bool(v)) if k == "use_neural_scene" else float(v))
        return q


assert C.sizeof(MissionParams) == 128     # static_assert of csrc/mission_device.hpp

CONTROLLER_STATE_WORDS = 12
SMOOTHER_STATE_WORDS = 25
MIXER_STATE_WORDS = 5
ONBOARD_STATE_WORDS = 14
LATENCY_STATE_WORDS = 4
LATENCY_MAX_DEPTH = 1000
MISSION_STATE_WORDS = 4
# MissionPhase in the reference's order, and the semantic labels the goal rule tells apart (include/se3mpc.h)
MISSION_PHASES = ("takeoff", "exploration", "mapping", "navigation", "landing", "emergency")
MISSION_LABELS = {"obstacle": 1, "landing_pad": 2, "doorway": 3}
# flag bits of se3mpc_mixer_mix_* (include/se3mpc.h)
MIXER_NEGATIVE_THRUST, MIXER_NON_FINITE, MIXER_OVERRUN, MIXER_SATURATION_EVENT, MIXER_ALL_IDLE, MIXER_WATCHDOG = 1, 2, 4, 8, 16, 32

_P = C.c_void_p
_I = C.c_int
_D = C.c_double
_PP = C.POINTER(Params)
_VP = C.POINTER(VoxelMapDesc)

# name -> argtypes after the leading (const se3mpc_params*) when `params` is True
_TYPED_API = {
    "init": (True, [_I, _I, _P, _P, _P, _I, _P, _P]),
    "cost_grad": (True, [_I, _I, _P, _P, _P, _P, _P]),
    "dynamics_residual": (True, [_I, _I, _P, _P, _P, _P, _P]),
    "obstacle_residual": (True, [_I, _I, _P, _P, _I, _P, _P, _P, _P]),
    "physical_constraints": (True, [_I, _I, _P, _P, _P]),
    "extract": (True, [_I, _I, _P, _P, _P, _P, _P, _P]),
    "rollout_cost_grad": (True, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint32, _P]),
    "rollout_cost_grad_batched": (True, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, C.c_uint32, _P]),
    "rollout_obstacles": (True, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, C.c_uint32, _P]),
    "rollout_obstacles_batched": (True, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, C.c_uint32, _P]),
    "rollout_iterate": (True, [_I, _I, _I, _I, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint32, _P]),
    "rollout_iterate_obstacles": (True, [_I, _I, _I, _I, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _D, _P, _P, C.c_uint32, _P]),
    "shooting_finish": (True, [_I, _I, _P, _P, _I, C.c_uint32, _P, _P, _I, _D, _P, _P, _P]),
    "projected_step": (True, [_I, _I, _D, _P, _P, _P, _P]),
    "is_plan_valid": (True, [_I, _I, _P, _P, _P, _P]),
    "argmin": (False, [_I, _P, C.c_uint32, _P, _P]),
    "spheres_from_grid": (False, [_P, _P, _I, C.c_double, _I, C.c_double, _P, _I, _P, _P]),
    "transpose": (False, [_I, _I, _P, _I, _P, _I, _P]),
    "population_sums": (False, [_I, _I, _I, _P, _P, _D, _P, _D, _P, _P, _P]),
    "mppi": (True, [_I, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, _I, _D, _P, _P, _P, _P]),
    "mppi_moving": (True, [_I, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _D, _I, _D, _P, _P, _P, _P]),
    "mppi_tracks": (True, [_I, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _D, _I, _P, _I, C.c_longlong, _D,
                           _P, _P, _P, _P]),
    "mppi_split": (True, [_I, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, _I, _D, _P, _P, _P, _I, _P, C.c_size_t,
                          _P]),
    "mppi_samples": (True, [_I, _I, _I, _D, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _I, _P, _P, _P]),
    "solve": (True, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "plan_host": (True, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_double, _P]),
}
# voxel map: se3mpc_voxel_<base>_<suffix>(const se3mpc_voxel_map*, ...)
_VOXEL_TYPED_API = {
    "query": [_P, _I, _P, _P],
    "trajectory_safe": [_P, _I, _I, C.c_longlong, _D, _D, _P, _P, _P],
    "local_spheres": [C.POINTER(C.c_double * 3), _D, _D, _I, _D, _P, _I, _P, _P, _P],
}
_VOXEL_PLAIN_API = {
    "se3mpc_voxel_clear": (C.c_int, [_VP, _P]),
    "se3mpc_voxel_insert": (C.c_int, [_VP, _P, _P, _D, _P, _I, _P, _P]),
    "se3mpc_voxel_update_rays": (C.c_int, [_VP, _P, _P, _P, _P, _I, _D, _D, _P, _P, _I, _P, _P, _P, _P]),
    "se3mpc_voxel_update_row_words": (C.c_longlong, [_I, _I]),
    "se3mpc_voxel_trace_rays": (C.c_int, [_VP, _P, _P, _P, _I, _P, _P, _I, _P, _P]),
    "se3mpc_voxel_export": (C.c_int, [_VP, _P, _P, _P, _P, _P]),
    "se3mpc_voxel_local_workspace": (C.c_int, [_I]),
}
# uncertainty field: se3mpc_ufield_<name>(const se3mpc_ufield*, ...); workspace and targets take no descriptor
_UP = C.POINTER(UFieldDesc)
_UFIELD_API = {
    "se3mpc_ufield_workspace": (C.c_longlong, [_I, _I, _I, _I]),
    "se3mpc_ufield_fill": (C.c_int, [_UP, _P]),
    "se3mpc_ufield_stamp": (C.c_int, [_UP, _P, _P, _P, _P, _I, _P]),
    "se3mpc_ufield_update_points": (C.c_int, [_UP, _P, _P, _P, _I, _D, _P, _P, C.c_longlong, _P]),
    "se3mpc_ufield_query": (C.c_int, [_UP, _P, _I, _P, _P]),
    "se3mpc_ufield_statistics": (C.c_int, [_UP, _D, _P, _P, _P, C.c_longlong, _P]),
    "se3mpc_ufield_regions": (C.c_int, [_UP, _D, _D, _I, _P, _P, _P, _P, _P, C.c_longlong, _P]),
    "se3mpc_ufield_targets": (C.c_int, [_P, _P, _I, C.POINTER(C.c_double * 3), _P, _P, _P]),
}
_CP = C.POINTER(ControllerParams)
_SP = C.POINTER(SimulatorParams)
_MP = C.POINTER(SmootherParams)
_XP = C.POINTER(MixerParams)
_OP = C.POINTER(OnboardParams)
_GP = C.POINTER(MissionParams)
_LL = C.c_longlong
_PLAN = [_I, _P, _LL, _P, _LL, _P, _LL, _P, _LL]            # N, timestamps, ts_stride, P, strideP, V, strideV, A, strideA
# consumer side of the contract: se3mpc_<base>_<suffix>(...)
_LOOP_TYPED_API = {
    "control": [_CP, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "control_fast": [_CP, _D, _D, _I, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "controller_integral_update": [_CP, _I, _P, _D, _P, _P, _P],
    "controller_attitude_torque": [_CP, _I, _P, _P, _P, _P, _P, C.POINTER(C.c_double * 9), _P, _P, _P, _P],
    "controller_desired_frame": [_CP, _I, _I, _P, _P, _P, _P, _P, _P, _P],
    "control_plan": [_CP, _I, _P, _P, _P, _P, _P, _P, _I, _P, _LL, _P, _LL, _P, _LL, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P],
    "simulator_step": [_SP, _I, _D, _P, _P, _P, _LL, _P, _P, _P, _P, _P, _P],
    "closed_loop": [_CP, _SP, _I, _I, _D, _I, _P, _LL, _P, _LL, _P, _LL, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _LL, _I,
                    C.POINTER(C.c_double * 3), _I, _P, _P, _P, _P, _P],
    "smoother_update": [_MP, _I, _P] + _PLAN + _PLAN + [_P, _P],
    "smoother_desired": [_MP, _I, _P, _P, _P] + _PLAN + [_P, _P, _P, _P],
    "closed_loop_smoothed": [_MP, _CP, _SP, _I, _I, _D] + _PLAN + [_P, _P, _P, _P, _P, _P, _P, _P, _LL, _I, C.POINTER(C.c_double * 3),
                             _P, _P, _P, _P, _P],
    "mixer_mix": [_XP, _I, _P, _P, _P, _P, _P, _P, _P],
    "mixer_readback": [_XP, _I, _P, _P, _LL, _P, _P, _P, _P, _P, _P],
    "closed_loop_actuated": [_MP, _CP, _SP, _XP, _I, _I, _D] + _PLAN + [_P, _P, _P, _P, _P, _P, _P, _P, _P, _LL, _P, _LL, _I,
                             C.POINTER(C.c_double * 3), _P, _P, _P, _P, _P, _P, _P],
    "latency_push": [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "onboard_control": [_OP, _I, _P, _P, _P, _P] + _PLAN + [_P, _P, _P, _P, _P],
    "edge_loop": [_OP, _SP, _I, _I, _D] + _PLAN + [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _LL, _I, C.POINTER(C.c_double * 3),
                  _P, _P, _P, _P, _P, _P, _P],
    "monte_carlo": [_PP, _CP, _SP, _I, _I, _I, _D, _P, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "monte_carlo_staged": [_PP, _CP, _SP, _MP, _XP, _I, _I, _I, _D, _P, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P, _P, _LL, _P, _P, _P, _P, _P],
    "monte_carlo_edge": [_PP, _OP, _SP, _I, _I, _I, _D, _I, _P, _P, _LL, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "mission_goal": [_GP, _I, _P, _P, _P, _P, _LL, _P, _LL, _I, _D, _P, _P, _P, _P, _P, _P],
    "monte_carlo_mission": [_PP, _CP, _SP, _GP, _I, _I, _I, _D, _I, _D, _P, _LL, _P, _LL, _I, _D, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                            _P, _P, _P, _P, _P],
    "mppi_closed_loop": [_PP, _CP, _SP, _I, _I, _I, _D, C.c_uint32, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _I, _D, _P, _LL,
                         _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "mppi_closed_loop_moving": [_PP, _CP, _SP, _I, _I, _I, _D, C.c_uint32, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _P, _D, _I,
                                _D, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "mppi_closed_loop_tracks": [_PP, _CP, _SP, _I, _I, _I, _D, C.c_uint32, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _P, _D, _I,
                                _P, _I, _D, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "mppi_closed_loop_swarm_intent": [_PP, _CP, _SP, _I, _I, _I, _D, _I, _I, _D, C.c_uint32, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, C.c_uint32, _P,
                                      _P, _P, _D, _I, _D, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P],
    "swarm_intent": [_PP, _I, _P, _P, _P, _P, _P],
    "mppi_closed_loop_swarm": [_PP, _CP, _SP, _I, _I, _I, _D, _I, _I, _D, C.c_uint32, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _P,
                               _D, _I, _D, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P],
    "swarm_separation": [_I, _I, _P, _P, _P, _P],
    "mppi_closed_loop_staged": [_PP, _CP, _SP, _MP, _XP, _I, _I, _I, _D, C.c_uint32, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _I,
                                _D, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P, _P, _LL, _P, _P, _P, _P, _P, _P, _P],
    "mppi_closed_loop_edge": [_PP, _OP, _SP, _I, _I, _I, _D, C.c_uint32, _I, _I, _I, _D, _D, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P, _I, _D, _P,
                              _LL, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
}
_PLAIN_API = {
    "se3mpc_controller_default_params": (C.c_int, [_CP]),
    "se3mpc_simulator_default_params": (C.c_int, [_SP]),
    "se3mpc_controller_reset": (C.c_int, [_CP, _I, _P, _P]),
    "se3mpc_smoother_default_params": (C.c_int, [_MP]),
    "se3mpc_smoother_reset": (C.c_int, [_I, _P, _P]),
    "se3mpc_mixer_default_params": (C.c_int, [_XP]),
    "se3mpc_mixer_reset": (C.c_int, [_I, _P, _P]),
    "se3mpc_onboard_default_params": (C.c_int, [_OP]),
    "se3mpc_onboard_reset": (C.c_int, [_I, _P, _P]),
    "se3mpc_latency_reset": (C.c_int, [_I, _I, _P, _P]),
    "se3mpc_mission_default_params": (C.c_int, [_GP]),
    "se3mpc_check_mission_params": (C.c_int, [_GP]),
    "se3mpc_mission_reset": (C.c_int, [_I, _P, _P]),
    "se3mpc_abi_version": (C.c_int, []),
    "se3mpc_last_error": (C.c_char_p, []),
    "se3mpc_device_count": (C.c_int, []),
    "se3mpc_default_params": (C.c_int, [_PP]),
    "se3mpc_check_params": (C.c_int, [_PP]),
    "se3mpc_set_rollout_variant": (C.c_int, [_I]),
    "se3mpc_set_solver_variant": (C.c_int, [_I]),
    "se3mpc_set_edge_loop_variant": (C.c_int, [_I]),
    "se3mpc_reduce_keys": (C.c_int, [_P, _I, _I, _P, _P]),
    "se3mpc_key_index": (C.c_uint32, [C.c_uint64]),
    "se3mpc_key_cost": (C.c_float, [C.c_uint64]),
    "se3mpc_population_workspace": (C.c_int, [_I, _I]),
    "se3mpc_mppi_split_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "se3mpc_mppi_swarm_workspace_bytes": (C.c_size_t, [_I, _I]),
    "se3mpc_mppi_swarm_intent_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
}


def exported_symbols() -> list:
    """Every symbol include/se3mpc.h declares (the CPU test-suite checks the .so exports them)."""
    names = list(_PLAIN_API)
    for base in _TYPED_API:
        names += [f"se3mpc_{base}_f32", f"se3mpc_{base}_f64"]
    for base in _LOOP_TYPED_API:
        names += [f"se3mpc_{base}_f32", f"se3mpc_{base}_f64"]
    names += list(_VOXEL_PLAIN_API)
    for base in _VOXEL_TYPED_API:
        names += [f"se3mpc_voxel_{base}_f32", f"se3mpc_voxel_{base}_f64"]
    names += list(_UFIELD_API)
    return names


class Library:
    """A loaded libse3mpc.so.  Methods take raw device addresses (ints) and return nothing;
    a negative status raises :class:`Se3mpcError`."""

    def __init__(self, path: Optional[str] = None):
        self.path = path or os.environ.get("SE3MPC_LIBRARY", DEFAULT_LIBRARY)
        if not os.path.exists(self.path):
            raise Se3mpcLibraryError(
                f"{self.path} not found: the HIP extension has not been built.  Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C dart_planner_amd/csrc`). "
                "There is no CPU fallback.")
        try:
            self._dll = C.CDLL(self.path)
        except OSError as e:  # pragma: no cover
            raise Se3mpcLibraryError(f"cannot load {self.path}: {e}") from e
        missing = [s for s in exported_symbols() if not hasattr(self._dll, s)]
        if missing:
            raise Se3mpcLibraryError(f"{self.path} does not export {missing}")
        for name, (res, args) in _PLAIN_API.items():
            fn = getattr(self._dll, name)
            fn.restype, fn.argtypes = res, args
        for base, (has_params, args) in _TYPED_API.items():
            for suf in ("f32", "f64"):
                fn = getattr(self._dll, f"se3mpc_{base}_{suf}")
                fn.restype = C.c_int
                fn.argtypes = ([_PP] if has_params else []) + args
        for base, args in _LOOP_TYPED_API.items():
            for suf in ("f32", "f64"):
                fn = getattr(self._dll, f"se3mpc_{base}_{suf}")
                fn.restype, fn.argtypes = C.c_int, args
        for name, (res, args) in _VOXEL_PLAIN_API.items():
            fn = getattr(self._dll, name)
            fn.restype, fn.argtypes = res, args
        for base, args in _VOXEL_TYPED_API.items():
            for suf in ("f32", "f64"):
                fn = getattr(self._dll, f"se3mpc_voxel_{base}_{suf}")
                fn.restype = C.c_int
                fn.argtypes = [_VP] + args
        for name, (res, args) in _UFIELD_API.items():
            fn = getattr(self._dll, name)
            fn.restype, fn.argtypes = res, args
        if self._dll.se3mpc_abi_version() != 1:
            raise Se3mpcLibraryError(f"{self.path}: ABI version {self._dll.se3mpc_abi_version()} != 1")

    # -- plain entry points -----------------------------------------------------------------
    def abi_version(self) -> int:
        return self._dll.se3mpc_abi_version()

    def last_error(self) -> str:
        return (self._dll.se3mpc_last_error() or b"").decode()

    def device_count(self) -> int:
        return self._dll.se3mpc_device_count()

    def default_params(self) -> Params:
        p = Params()
        self._check("se3mpc_default_params", self._dll.se3mpc_default_params(C.byref(p)))
        return p

    def check_params(self, p: Params) -> int:
        return self._dll.se3mpc_check_params(C.byref(p))

    def set_rollout_variant(self, variant: int) -> None:
        self._check("se3mpc_set_rollout_variant", self._dll.se3mpc_set_rollout_variant(variant))

    def set_solver_variant(self, variant: int) -> None:
        self._check("se3mpc_set_solver_variant", self._dll.se3mpc_set_solver_variant(variant))

    def set_edge_loop_variant(self, variant: int) -> None:
        self._check("se3mpc_set_edge_loop_variant", self._dll.se3mpc_set_edge_loop_variant(variant))

    def reduce_keys(self, wave_keys: int, per_batch: int, nbatch: int, keys_out: int, stream: int) -> None:
        self._check("se3mpc_reduce_keys", self._dll.se3mpc_reduce_keys(wave_keys, per_batch, nbatch, keys_out, stream))

    def population_workspace(self, rows: int, B: int) -> int:
        return self._dll.se3mpc_population_workspace(rows, B)

    def mppi_split_workspace_bytes(self, horizon: int, nprob: int, splits: int) -> int:
        return self._dll.se3mpc_mppi_split_workspace_bytes(horizon, nprob, splits)

    def mppi_swarm_workspace_bytes(self, B: int, elem_size: int) -> int:
        return self._dll.se3mpc_mppi_swarm_workspace_bytes(B, elem_size)

    def mppi_swarm_intent_workspace_bytes(self, B: int, horizon: int, elem_size: int) -> int:
        return self._dll.se3mpc_mppi_swarm_intent_workspace_bytes(B, horizon, elem_size)

    def key_index(self, key: int) -> int:
        return self._dll.se3mpc_key_index(C.c_uint64(key))

    def key_cost(self, key: int) -> float:
        return self._dll.se3mpc_key_cost(C.c_uint64(key))

    # -- typed entry points -----------------------------------------------------------------
    def call(self, base: str, suffix: str, *args, params: Optional[Params] = None) -> None:
        """Call se3mpc_<base>_<suffix>(params?, *args); raise on a negative status."""
        fn = getattr(self._dll, f"se3mpc_{base}_{suffix}")
        has_params = _TYPED_API[base][0]
        if has_params:
            if params is None:
                raise TypeError(f"se3mpc_{base} needs params")
            rc = fn(C.byref(params), *args)
        else:
            rc = fn(*args)
        self._check(f"se3mpc_{base}_{suffix}", rc)

    def call_status(self, base: str, suffix: str, *args, params: Optional[Params] = None) -> int:
        """Same as :meth:`call` but returns the raw status (used by the error-behaviour tests)."""
        fn = getattr(self._dll, f"se3mpc_{base}_{suffix}")
        if _TYPED_API[base][0]:
            return fn(C.byref(params) if params is not None else None, *args)
        return fn(*args)

    # -- consumer side of the contract --------------------------------------------------------
    def controller_default_params(self) -> ControllerParams:
        p = ControllerParams()
        self._check("se3mpc_controller_default_params", self._dll.se3mpc_controller_default_params(C.byref(p)))
        return p

    def simulator_default_params(self) -> SimulatorParams:
        p = SimulatorParams()
        self._check("se3mpc_simulator_default_params", self._dll.se3mpc_simulator_default_params(C.byref(p)))
        return p

    def controller_reset(self, cp: ControllerParams, B: int, state: int, stream: int) -> None:
        self._check("se3mpc_controller_reset", self._dll.se3mpc_controller_reset(C.byref(cp), B, state, stream))

    def smoother_default_params(self) -> SmootherParams:
        p = SmootherParams()
        self._check("se3mpc_smoother_default_params", self._dll.se3mpc_smoother_default_params(C.byref(p)))
        return p

    def smoother_reset(self, B: int, state: int, stream: int) -> None:
        self._check("se3mpc_smoother_reset", self._dll.se3mpc_smoother_reset(B, state, stream))

    def mixer_default_params(self) -> MixerParams:
        p = MixerParams()
        self._check("se3mpc_mixer_default_params", self._dll.se3mpc_mixer_default_params(C.byref(p)))
        return p

    def mixer_reset(self, B: int, state: int, stream: int) -> None:
        self._check("se3mpc_mixer_reset", self._dll.se3mpc_mixer_reset(B, state, stream))

    def onboard_default_params(self) -> OnboardParams:
        p = OnboardParams()
        self._check("se3mpc_onboard_default_params", self._dll.se3mpc_onboard_default_params(C.byref(p)))
        return p

    def onboard_reset(self, B: int, state: int, stream: int) -> None:
        self._check("se3mpc_onboard_reset", self._dll.se3mpc_onboard_reset(B, state, stream))

    def latency_reset(self, B: int, depth: int, state: int, stream: int) -> None:
        self._check("se3mpc_latency_reset", self._dll.se3mpc_latency_reset(B, depth, state, stream))

    def mission_default_params(self) -> MissionParams:
        p = MissionParams()
        self._check("se3mpc_mission_default_params", self._dll.se3mpc_mission_default_params(C.byref(p)))
        return p

    def check_mission_params(self, mp: Optional[MissionParams]) -> int:
        return self._dll.se3mpc_check_mission_params(C.byref(mp) if mp is not None else None)

    def mission_reset(self, B: int, state: int, stream: int) -> None:
        self._check("se3mpc_mission_reset", self._dll.se3mpc_mission_reset(B, state, stream))

    def loop_call(self, base: str, suffix: str, *args) -> None:
        """se3mpc_control_<suffix> / se3mpc_closed_loop_<suffix>; struct arguments are passed by reference here."""
        a = [C.byref(x) if isinstance(x, _STRUCTS) else x for x in args]
        self._check(f"se3mpc_{base}_{suffix}", getattr(self._dll, f"se3mpc_{base}_{suffix}")(*a))

    def loop_status(self, base: str, suffix: str, *args) -> int:
        a = [C.byref(x) if isinstance(x, _STRUCTS) else x for x in args]
        return getattr(self._dll, f"se3mpc_{base}_{suffix}")(*a)

    # -- voxel map ----------------------------------------------------------------------------
    def voxel(self, name: str, desc: VoxelMapDesc, *args) -> None:
        """Call se3mpc_voxel_<name>(&desc, *args) (name = 'clear', 'insert', 'export', 'query_f32', ...)."""
        self._check(f"se3mpc_voxel_{name}", getattr(self._dll, f"se3mpc_voxel_{name}")(C.byref(desc), *args))

    def voxel_status(self, name: str, desc: Optional[VoxelMapDesc], *args) -> int:
        return getattr(self._dll, f"se3mpc_voxel_{name}")(C.byref(desc) if desc is not None else None, *args)

    def voxel_local_workspace(self, cells_per_axis: int) -> int:
        return self._dll.se3mpc_voxel_local_workspace(cells_per_axis)

    def voxel_update_row_words(self, M: int, max_len: int) -> int:
        return self._dll.se3mpc_voxel_update_row_words(M, max_len)

    # -- uncertainty field --------------------------------------------------------------------
    def ufield(self, name: str, desc: UFieldDesc, *args) -> None:
        """Call se3mpc_ufield_<name>(&desc, *args) (name = 'fill', 'stamp', 'update_points', 'query', 'statistics', 'regions')."""
        self._check(f"se3mpc_ufield_{name}", getattr(self._dll, f"se3mpc_ufield_{name}")(C.byref(desc), *args))

    def ufield_status(self, name: str, desc: Optional[UFieldDesc], *args) -> int:
        return getattr(self._dll, f"se3mpc_ufield_{name}")(C.byref(desc) if desc is not None else None, *args)

    def ufield_workspace(self, nx: int, ny: int, nz: int, max_regions: int) -> int:
        return self._dll.se3mpc_ufield_workspace(nx, ny, nz, max_regions)

    @staticmethod
    def _position(position):
        return None if position is None else (C.c_double * 3)(*[float(v) for v in position])

    def ufield_targets(self, regions: int, counts: int, num_targets: int, position, targets: int, n_out: int, stream: int) -> None:
        self._check("se3mpc_ufield_targets", self._dll.se3mpc_ufield_targets(regions, counts, num_targets, self._position(position), targets, n_out, stream))

    def ufield_targets_status(self, regions: int, counts: int, num_targets: int, position, targets: int, n_out: int, stream: int) -> int:
        return self._dll.se3mpc_ufield_targets(regions, counts, num_targets, self._position(position), targets, n_out, stream)

    def _check(self, name: str, rc: int) -> None:
        if rc != 0:
            raise Se3mpcError(name, rc, self.last_error() if rc == -6 else "")


_STRUCTS = (ControllerParams, SimulatorParams, SmootherParams, MixerParams, OnboardParams, MissionParams, Params)
_default: Optional[Library] = None


def get_library() -> Library:
    """The process-wide library handle (loads on first use; raises if it is not built)."""
    global _default
    if _default is None:
        _default = Library()
    return _default
