"""Mirror of the reference's ``dart_planner.hardware.motor_mixer`` (src/dart_planner/hardware/motor_mixer.py), one vehicle: same classes,
factories, members, validation and exceptions.  ``saturation_events`` and ``last_motor_commands`` live in a one-drone device record
(SE3MPC_MIXER_STATE_WORDS doubles, include/se3mpc.h) and every number on the command path comes from the kernels of ``csrc/mixer.hip``
(``se3mpc_mixer_mix_*`` / ``se3mpc_mixer_readback_*``); the two model values ``_compute_mixing_matrix`` needs are one-element launches of
the model.  Host NumPy is used where the reference itself does set-up algebra: ``np.linalg.solve`` / ``pinv`` for the inverse -- the same
calls, so a singular layout (the plus factory's matrix has rank 3: ``solve`` raises and ``pinv`` answers) gets the reference's matrix here too -- and ``matrix_rank``.

The device mixer drives four motors.  With a ``QuadraticMotorModel`` the whole of ``mix_commands`` is one launch.  Any other ``MotorModel``
subclass (the reference's own tests wrap one written in the test file) keeps the mixer's arithmetic on the device -- allocation through the
inverse matrix, ``max(., 0)``, the non-finite guard, saturation, the idle floor, the saturation counter and the record -- in two launches,
with the foreign model's own ``pwm_from_thrust`` / ``thrust_from_pwm`` called on the host in between, as the reference calls them.  A
``motor_model`` that is no ``MotorModel`` at all raises TypeError.

For B drones at once, and for the actuated control-rate loop in one launch, use ``Ops.mixer_mix`` / ``mixer_readback`` /
``closed_loop_actuated`` (``dart_planner_amd/control/closed_loop.py``)."""
import logging
from dataclasses import dataclass, field
from enum import Enum
from typing import Any, Dict, List, Optional, Union

import numpy as np

from ..capi import MIXER_NON_FINITE, MIXER_STATE_WORDS, MixerParams
from .motor_model import _WIDE, MotorModel, QuadraticMotorModel, create_default_motor_model, motor_fields  # noqa: F401

logger = logging.getLogger(__name__)


class QuadrotorLayout(Enum):
    """Supported quadrotor layouts."""
    X_CONFIGURATION = "x"
    PLUS_CONFIGURATION = "plus"
    CUSTOM = "custom"


@dataclass
class MotorMixingConfig:
    """mixer.py:38-105.  ``mixing_matrix`` here is the matrix of rows (1, y_i, x_i, direction_i) the reference's config computes and its
    mixer never uses (MotorMixer builds its own from the motor model)."""
    layout: QuadrotorLayout = QuadrotorLayout.X_CONFIGURATION
    motor_positions: List[List[float]] = field(default_factory=lambda: [[0.15, -0.15, 0.0], [0.15, 0.15, 0.0], [-0.15, 0.15, 0.0], [-0.15, -0.15, 0.0]])
    motor_directions: List[int] = field(default_factory=lambda: [1, -1, 1, -1])
    pwm_min: float = 0.0
    pwm_max: float = 1.0
    pwm_idle: float = 0.1
    arm_length: float = 0.15
    motor_model: Any = None
    mixing_matrix: Optional[np.ndarray] = None

    def __post_init__(self):
        if self.mixing_matrix is None:
            self.mixing_matrix = self._compute_mixing_matrix()

    def _compute_mixing_matrix(self) -> np.ndarray:
        matrix = np.zeros((4, 4))
        for i, (pos, direction) in enumerate(zip(self.motor_positions, self.motor_directions)):
            x, y, z = pos
            matrix[i] = [1.0, y, x, direction]
        return matrix


class MotorMixer:
    """mixer.py:108-398 on the device, one vehicle."""

    def __init__(self, config: MotorMixingConfig, *, precision: str = "f64", device=None):
        self.config = config
        self.precision = precision
        self._device = device
        self._ops = None
        self._state = None
        if config.motor_model is None:
            self.motor_model = create_default_motor_model(precision=precision, device=device)
            logger.info("Using default motor model - consider providing calibrated model for production")
        else:
            if not isinstance(config.motor_model, MotorModel):
                raise TypeError(f"motor_model must be a MotorModel (a QuadraticMotorModel runs on the device as a whole), got {type(config.motor_model).__name__}")
            self.motor_model = config.motor_model
            logger.info("Using provided motor model")
        self._foreign = not isinstance(self.motor_model, QuadraticMotorModel)      # its numbers come from its own methods, on the host
        self.mixing_matrix = self._compute_mixing_matrix()
        self.inverse_matrix = self._compute_inverse_matrix()
        validation_issues = self.validate_configuration()
        if validation_issues:
            logger.warning(f"Motor mixer configuration issues: {validation_issues}")

    # ------------------------------------------------------------------ device plumbing
    def _get_ops(self):
        if self._ops is None:
            from ..ops import Ops, TorchBackend
            self._ops = Ops(TorchBackend(self._device))      # raises without a HIP device / built library
        return self._ops

    def _dev(self, a):
        dt = {"f32": np.float32, "f64": np.float64}[self.precision]
        return self._get_ops().be.from_host(np.ascontiguousarray(np.asarray(a, dtype=float).astype(dt)))

    def _members(self):
        if self._state is None:
            self._state = self._get_ops().mixer_state(1)
        return self._state

    def _record(self) -> np.ndarray:
        return np.array(self._get_ops().be.to_host(self._members()), dtype=float).reshape(MIXER_STATE_WORDS)

    def _write_record(self, rec) -> None:
        self._state = self._get_ops().be.from_host(np.ascontiguousarray(np.asarray(rec, float).reshape(1, MIXER_STATE_WORDS)))

    @staticmethod
    def _through(idle=(0.0, 0.0, 0.0, 0.0)) -> list:
        """Pass-through motors: thrust = pwm, no limits, so that pwm_from_thrust(x) = x for x > 0 and idle[i] for x <= 0."""
        return [dict(thrust_a=0.0, thrust_b=1.0, thrust_c=0.0, pwm_min=-_WIDE, pwm_max=_WIDE, pwm_idle=float(x), torque_coefficient=0.0, rpm_coefficient=1.0,
                     rpm_offset=0.0) for x in idle]

    def _motors(self) -> list:
        if self._foreign:
            return self._through()
        return [motor_fields(self.motor_model.get_motor_parameters(i)) for i in range(4)]     # ValueError("Unknown motor ID") as the reference's model

    def _params(self, **overrides) -> MixerParams:
        """se3mpc_mixer_params of this mixer as it stands (members assigned since the constructor are honoured, as in the reference)."""
        if self.inverse_matrix is None or np.shape(self.inverse_matrix) != (4, 4) or np.shape(self.mixing_matrix) != (4, 4):
            raise ValueError("the device mixer drives four motors: mixing_matrix and inverse_matrix must be 4 x 4")
        kw = dict(config_pwm_min=self.config.pwm_min, config_pwm_max=self.config.pwm_max, config_pwm_idle=self.config.pwm_idle)
        kw.update(overrides)
        return MixerParams.from_matrices(kw.pop("mixing", self.mixing_matrix), kw.pop("inverse", self.inverse_matrix), kw.pop("motors", None) or self._motors(),
                                         **kw)

    # ------------------------------------------------------------------ the record's members
    @property
    def saturation_events(self) -> int:
        return int(self._record()[0])

    @saturation_events.setter
    def saturation_events(self, value) -> None:
        rec = self._record()
        rec[0] = value
        self._write_record(rec)

    @property
    def last_motor_commands(self) -> np.ndarray:
        return self._record()[1:5].copy()

    @last_motor_commands.setter
    def last_motor_commands(self, value) -> None:
        rec = self._record()
        rec[1:5] = np.asarray(value, float).reshape(4)
        self._write_record(rec)

    # ------------------------------------------------------------------ the reference's interface
    def _compute_inverse_matrix(self) -> Optional[np.ndarray]:
        """mixer.py:152-166: the same NumPy calls."""
        if self.mixing_matrix is None:
            return None
        try:
            return np.linalg.solve(self.mixing_matrix, np.eye(self.mixing_matrix.shape[0]))
        except (np.linalg.LinAlgError, ValueError):
            logger.warning("Direct inverse failed, falling back to pseudo-inverse")
            return np.linalg.pinv(self.mixing_matrix)

    def mix_commands(self, thrust: float, torque: np.ndarray) -> np.ndarray:
        """mix_commands (mixer.py:168-222): one ``se3mpc_mixer_mix_*`` launch on the record."""
        if len(torque) != 3:
            raise ValueError("Torque must be 3-element array [τx, τy, τz]")
        if thrust < 0:
            logger.warning(f"Negative thrust command: {thrust} N - clamping to zero")
        ops = self._get_ops()
        th, tq = self._dev([float(thrust)]), self._dev(np.asarray(torque, float).reshape(1, 3))
        if self._foreign:
            # launch 1: max(inverse @ command, 0) behind pass-through motors and no config limits (mixer.py:192-199, :235)
            out = ops.mixer_mix(self._params(config_pwm_min=-_WIDE, config_pwm_max=_WIDE, config_pwm_idle=-_WIDE), th, tq)
        else:
            out = ops.mixer_mix(self._params(), th, tq, self._members())
        flags = int(ops.be.to_host(out["flags"])[0])
        if flags & MIXER_NON_FINITE:
            raise RuntimeError("Non-finite motor thrust command detected")
        pwm = np.array(ops.be.to_host(out["pwm"]), dtype=float).reshape(4)
        if self._foreign:
            raw = [float(self.motor_model.pwm_from_thrust(float(pwm[i]), motor_id=i)) for i in range(4)]      # :239-240, the model's own code
            pwm = self._saturate_pwm(raw, self._members())                       # launch 2: :210-221 on the record
        return pwm

    def _positive_part(self, values) -> np.ndarray:
        """np.maximum(values, 0) (mixer.py:235) on the device: pass-through motors behind an identity allocation, no config limits."""
        f = np.asarray(values, float).reshape(4)
        eye = np.eye(4)
        out = self._get_ops().mixer_mix(self._params(mixing=eye, inverse=eye, motors=self._through(), config_pwm_min=-_WIDE, config_pwm_max=_WIDE,
                                                     config_pwm_idle=-_WIDE), self._dev(f[0:1]), self._dev(f[None, 1:4]), want_flags=False)
        return np.array(self._get_ops().be.to_host(out["pwm"]), dtype=float).reshape(4)

    def _thrust_to_pwm(self, motor_thrusts: np.ndarray) -> np.ndarray:
        """mixer.py:224-242: the mix kernel with an identity allocation (the four motor thrusts ARE the command vector) and config limits
        that touch nothing."""
        if self._foreign:
            f = self._positive_part(motor_thrusts)
            return np.array([float(self.motor_model.pwm_from_thrust(float(f[i]), motor_id=i)) for i in range(4)])
        f = np.asarray(motor_thrusts, float).reshape(4)
        eye = np.eye(4)
        out = self._get_ops().mixer_mix(self._params(mixing=eye, inverse=eye, config_pwm_min=-_WIDE, config_pwm_max=_WIDE, config_pwm_idle=-_WIDE),
                                        self._dev(f[0:1]), self._dev(f[None, 1:4]), want_flags=False)
        return np.array(self._get_ops().be.to_host(out["pwm"]), dtype=float).reshape(4)

    def _saturate_pwm(self, pwm_values: np.ndarray, state=None) -> np.ndarray:
        """mixer.py:244-260: the mix kernel's saturation stage behind pass-through motors (thrust = pwm; a value <= 0 rides in as that
        motor's idle PWM).  With `state` (the record) the call also counts the saturation event and sets last_motor_commands (:213-221)."""
        v = np.asarray(pwm_values, float).reshape(4)
        through = self._through([min(x, 0.0) if x == x else 0.0 for x in v])
        eye = np.eye(4)
        out = self._get_ops().mixer_mix(self._params(mixing=eye, inverse=eye, motors=through), self._dev(v[0:1]), self._dev(v[None, 1:4]), state, want_flags=False)
        return np.array(self._get_ops().be.to_host(out["pwm"]), dtype=float).reshape(4)

    def _readback(self, motor_pwms, what: str) -> np.ndarray:
        ops = self._get_ops()
        if self._foreign:
            # the foreign model's own thrusts (mixer.py:292-294), then the matrix product on the device behind pass-through motors
            f = np.array([float(self.motor_model.thrust_from_pwm(float(p), motor_id=i)) for i, p in enumerate(np.asarray(motor_pwms, float).reshape(4))])
            if what == "motor_thrust":
                return f
            if not np.all(f >= 0.0):
                raise ValueError(f"motor thrusts {f} from {type(self.motor_model).__name__}: the device product takes non-negative thrusts")
            motor_pwms = f
        out = ops.mixer_readback(self._params(), self._dev(np.asarray(motor_pwms, float).reshape(1, 4)), want=(what,))
        return np.array(ops.be.to_host(out[what]), dtype=float).reshape(4)

    def get_control_allocation(self, motor_pwms: np.ndarray) -> np.ndarray:
        """mixer.py:262-279: the INVERSE matrix on the motor thrusts, as the reference has it."""
        if self.inverse_matrix is None:
            raise RuntimeError("Cannot compute control allocation without inverse matrix")
        return self._readback(motor_pwms, "allocation")

    def get_realised_wrench(self, motor_pwms: np.ndarray) -> np.ndarray:
        """(thrust, torque) the motors deliver under the PWMs: mixing_matrix @ motor thrusts.  Not in the reference, whose
        get_control_allocation does not compute it; a simulator behind the mixer needs it."""
        return self._readback(motor_pwms, "wrench")

    def _pwm_to_thrust(self, pwm_values: np.ndarray) -> np.ndarray:
        """mixer.py:281-296."""
        return self._readback(pwm_values, "motor_thrust")

    def validate_configuration(self) -> List[str]:
        """mixer.py:298-345."""
        issues = []
        if self.mixing_matrix is None:
            issues.append("Mixing matrix is None")
        elif self.mixing_matrix.shape != (4, 4):
            issues.append(f"Mixing matrix must be 4x4, got {self.mixing_matrix.shape}")
        else:
            rank = np.linalg.matrix_rank(self.mixing_matrix)
            if rank < 4:
                issues.append(f"Mixing matrix is rank-deficient (rank={rank})")
        if len(self.config.motor_positions) != 4:
            issues.append(f"Must have 4 motor positions, got {len(self.config.motor_positions)}")
        if len(self.config.motor_directions) != 4:
            issues.append(f"Must have 4 motor directions, got {len(self.config.motor_directions)}")
        if self.config.pwm_min >= self.config.pwm_max:
            issues.append("PWM min must be less than PWM max")
        if self.config.pwm_idle < self.config.pwm_min or self.config.pwm_idle > self.config.pwm_max:
            issues.append("PWM idle must be between PWM min and max")
        if self.config.arm_length <= 0:
            issues.append("Arm length must be positive")
        for i, pos in enumerate(self.config.motor_positions):
            if len(pos) != 3:
                issues.append(f"Motor {i} position must have 3 coordinates")
            x, y, z = pos
            if abs(x) > 1.0 or abs(y) > 1.0 or abs(z) > 0.5:
                issues.append(f"Motor {i} position {pos} seems unreasonable (units: meters)")
        return issues

    def get_motor_layout_info(self) -> Dict[str, Union[str, List, np.ndarray, int, Dict[str, str], None]]:
        """mixer.py:347-369."""
        return {"layout": self.config.layout.value, "motor_positions": self.config.motor_positions, "motor_directions": self.config.motor_directions,
                "mixing_matrix": self.mixing_matrix, "matrix_rank": np.linalg.matrix_rank(self.mixing_matrix) if self.mixing_matrix is not None else 0,
                "saturation_events": self.saturation_events,
                "units": {"thrust": "Newtons (N)", "torque": "Newton-meters (N⋅m)", "position": "meters (m)", "pwm": "normalized (0.0 to 1.0)"}}

    def reset_saturation_counter(self) -> None:
        self.saturation_events = 0

    def _compute_mixing_matrix(self) -> np.ndarray:
        """mixer.py:379-398: B with column i = (1, y_i, x_i, direction_i * k_drag_i), k_drag_i from the model's two values at config.pwm_max."""
        positions, directions = self.config.motor_positions, self.config.motor_directions
        B = np.zeros((4, len(positions)))
        for i, (pos, direction) in enumerate(zip(positions, directions)):
            x, y, _ = pos
            thrust_max = self.motor_model.thrust_from_pwm(self.config.pwm_max, motor_id=i)
            torque_max = self.motor_model.torque_from_pwm(self.config.pwm_max, motor_id=i)
            B[:, i] = [1.0, y, x, direction * (torque_max / thrust_max if thrust_max > 0 else 0.0)]
        return B


def create_x_configuration_mixer(arm_length: float = 0.15, **device_options) -> MotorMixer:
    """mixer.py:401-423: front-right, front-left, rear-left, rear-right at arm_length * 0.707."""
    d = arm_length * 0.707
    config = MotorMixingConfig(layout=QuadrotorLayout.X_CONFIGURATION, motor_positions=[[d, -d, 0.0], [d, d, 0.0], [-d, d, 0.0], [-d, -d, 0.0]],
                               motor_directions=[1, -1, 1, -1], arm_length=arm_length)
    return MotorMixer(config, **device_options)


def create_plus_configuration_mixer(arm_length: float = 0.15, **device_options) -> MotorMixer:
    """mixer.py:426-448: front, left, right, rear.  With the directions CCW, CW, CCW, CW this matrix has rank 3; its "inverse" is
    the pseudo-inverse _compute_inverse_matrix falls back to, as in the reference."""
    config = MotorMixingConfig(layout=QuadrotorLayout.PLUS_CONFIGURATION,
                               motor_positions=[[arm_length, 0.0, 0.0], [0.0, arm_length, 0.0], [0.0, -arm_length, 0.0], [-arm_length, 0.0, 0.0]],
                               motor_directions=[1, -1, 1, -1], arm_length=arm_length)
    return MotorMixer(config, **device_options)
