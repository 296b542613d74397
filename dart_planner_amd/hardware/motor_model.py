"""Mirror of the reference's ``dart_planner.hardware.motor_model`` (src/dart_planner/hardware/motor_model.py): same classes, functions,
members, validation and exceptions.  Every number a model method returns comes from the kernels of ``csrc/mixer.hip``: the scalar methods
are one-element launches (``se3mpc_mixer_readback_*`` for the forward model, ``se3mpc_mixer_mix_*`` with an identity allocation and no
config limits for ``pwm_from_thrust``).  Host NumPy is used where the reference itself does set-up algebra: ``np.polyfit`` and the means of
the calibration fit.

For B drones at once use ``Ops.mixer_mix`` / ``Ops.mixer_readback`` (``dart_planner_amd/ops.py``)."""
import logging
from abc import ABC, abstractmethod
from dataclasses import dataclass, field
from enum import Enum
from typing import Any, Dict, List, Optional

import numpy as np

from ..capi import MixerParams

logger = logging.getLogger(__name__)
_WIDE = 1.0e308            # a config limit no PWM reaches: the mixer's own clip and idle floor are then the identity


class MotorType(Enum):
    """Supported motor types."""
    BRUSHLESS_DC = "brushless_dc"
    BRUSHED_DC = "brushed_dc"
    SERVO = "servo"


@dataclass
class MotorParameters:
    """Physical parameters of one motor (model.py:27-69): thrust = a pwm^2 + b pwm + c, rpm = k pwm + offset, torque = kQ rpm^2."""
    motor_id: int
    motor_type: MotorType = MotorType.BRUSHLESS_DC
    thrust_a: float = 0.0
    thrust_b: float = 0.0
    thrust_c: float = 0.0
    torque_coefficient: float = 0.0
    rpm_coefficient: float = 0.0
    rpm_offset: float = 0.0
    pwm_min: float = 0.0
    pwm_max: float = 1.0
    pwm_idle: float = 0.1
    rpm_max: float = 10000.0
    direction: int = 1
    calibration_date: Optional[str] = None
    calibration_notes: Optional[str] = None

    def __post_init__(self):
        if self.thrust_a < 0:
            raise ValueError(f"Motor {self.motor_id}: thrust_a must be non-negative")
        if self.torque_coefficient < 0:
            raise ValueError(f"Motor {self.motor_id}: torque_coefficient must be non-negative")
        if self.rpm_coefficient <= 0:
            raise ValueError(f"Motor {self.motor_id}: rpm_coefficient must be positive")
        if self.pwm_min >= self.pwm_max:
            raise ValueError(f"Motor {self.motor_id}: pwm_min must be less than pwm_max")
        if self.direction not in [-1, 1]:
            raise ValueError(f"Motor {self.motor_id}: direction must be ±1")


@dataclass
class BenchTestData:
    """Bench test data for a calibration (model.py:72-102)."""
    motor_id: int
    pwm_values: List[float] = field(default_factory=list)
    thrust_measurements: List[float] = field(default_factory=list)
    torque_measurements: List[float] = field(default_factory=list)
    rpm_measurements: List[float] = field(default_factory=list)

    def validate(self) -> List[str]:
        errors = []
        if len(self.pwm_values) < 3:
            errors.append(f"Motor {self.motor_id}: Need at least 3 data points for quadratic fit")
        if len(self.pwm_values) != len(self.thrust_measurements):
            errors.append(f"Motor {self.motor_id}: PWM and thrust data lengths don't match")
        if len(self.pwm_values) != len(self.rpm_measurements):
            errors.append(f"Motor {self.motor_id}: PWM and RPM data lengths don't match")
        if any(a > b for a, b in zip(self.pwm_values, self.pwm_values[1:])):
            errors.append(f"Motor {self.motor_id}: PWM values must be monotonically increasing")
        if any(t < 0 for t in self.thrust_measurements):
            errors.append(f"Motor {self.motor_id}: Thrust measurements must be non-negative")
        return errors


class MotorModel(ABC):
    """Abstract interface of a motor model (model.py:105-136)."""

    @abstractmethod
    def thrust_from_pwm(self, pwm: float, motor_id: int) -> float:
        pass

    @abstractmethod
    def torque_from_pwm(self, pwm: float, motor_id: int) -> float:
        pass

    @abstractmethod
    def pwm_from_thrust(self, thrust: float, motor_id: int) -> float:
        pass

    @abstractmethod
    def rpm_from_pwm(self, pwm: float, motor_id: int) -> float:
        pass

    @abstractmethod
    def get_motor_parameters(self, motor_id: int) -> MotorParameters:
        pass

    @abstractmethod
    def validate_pwm(self, pwm: float, motor_id: int) -> bool:
        pass


def motor_fields(params: MotorParameters) -> dict:
    """One motor's part of se3mpc_mixer_params."""
    return {k: float(getattr(params, k)) for k in MixerParams.MOTOR_FIELDS}


class QuadraticMotorModel(MotorModel):
    """model.py:139-316 on the device."""

    def __init__(self, motor_parameters: Dict[int, MotorParameters], *, precision: str = "f64", device=None):
        self.motor_parameters = motor_parameters
        self.logger = logging.getLogger(f"{__name__}.{self.__class__.__name__}")
        for motor_id, params in motor_parameters.items():
            if motor_id != params.motor_id:
                raise ValueError(f"Motor ID mismatch: {motor_id} != {params.motor_id}")
        self.precision = precision
        self._device = device
        self._ops = None
        self.logger.info(f"Initialized quadratic motor model with {len(motor_parameters)} motors")

    # ------------------------------------------------------------------ device plumbing
    def _get_ops(self):
        if self._ops is None:
            from ..ops import Ops, TorchBackend
            self._ops = Ops(TorchBackend(self._device))      # raises without a HIP device / built library
        return self._ops

    def _dev(self, a):
        dt = {"f32": np.float32, "f64": np.float64}[self.precision]
        return self._get_ops().be.from_host(np.ascontiguousarray(np.asarray(a, dtype=float).astype(dt)))

    def _one_motor(self, motor_id: int) -> MixerParams:
        """Launch parameters with motor `motor_id` in every slot, identity matrices and config limits that touch nothing."""
        if motor_id not in self.motor_parameters:
            raise ValueError(f"Unknown motor ID: {motor_id}")
        eye = np.eye(4)
        return MixerParams.from_matrices(eye, eye, [motor_fields(self.motor_parameters[motor_id])] * 4, config_pwm_min=-_WIDE, config_pwm_max=_WIDE,
                                         config_pwm_idle=-_WIDE)

    def _forward(self, pwm: float, motor_id: int, what: str) -> float:
        ops = self._get_ops()
        out = ops.mixer_readback(self._one_motor(motor_id), self._dev(np.full((1, 4), float(pwm))), want=(what,))
        return float(ops.be.to_host(out[what])[0, 0])

    # ------------------------------------------------------------------ the reference's interface
    def thrust_from_pwm(self, pwm: float, motor_id: int) -> float:
        """model.py:166-190."""
        return self._forward(pwm, motor_id, "motor_thrust")

    def torque_from_pwm(self, pwm: float, motor_id: int) -> float:
        """model.py:192-217."""
        return self._forward(pwm, motor_id, "motor_torque")

    def rpm_from_pwm(self, pwm: float, motor_id: int) -> float:
        """model.py:260-282."""
        return self._forward(pwm, motor_id, "motor_rpm")

    def pwm_from_thrust(self, thrust: float, motor_id: int) -> float:
        """model.py:219-258: the mix kernel with an identity allocation, so motor 0 is asked for `thrust`.  A thrust that is not finite
        returns NaN (the kernel's non-finite guard sits before the model)."""
        ops = self._get_ops()
        out = ops.mixer_mix(self._one_motor(motor_id), self._dev([float(thrust)]), self._dev(np.zeros((1, 3))), want_flags=False)
        return float(ops.be.to_host(out["pwm"])[0, 0])

    def get_motor_parameters(self, motor_id: int) -> MotorParameters:
        if motor_id not in self.motor_parameters:
            raise ValueError(f"Unknown motor ID: {motor_id}")
        return self.motor_parameters[motor_id]

    def validate_pwm(self, pwm: float, motor_id: int) -> bool:
        if motor_id not in self.motor_parameters:
            return False
        params = self.motor_parameters[motor_id]
        return bool(params.pwm_min <= pwm <= params.pwm_max)

    def get_model_summary(self) -> Dict[str, Any]:
        summary = {"model_type": "quadratic", "motor_count": len(self.motor_parameters), "motors": {}}
        for motor_id, p in self.motor_parameters.items():
            summary["motors"][motor_id] = {
                "type": p.motor_type.value,
                "thrust_model": f"T = {p.thrust_a:.3e}*PWM² + {p.thrust_b:.3e}*PWM + {p.thrust_c:.3e}",
                "torque_model": f"τ = {p.torque_coefficient:.3e}*RPM²",
                "rpm_model": f"RPM = {p.rpm_coefficient:.1f}*PWM + {p.rpm_offset:.1f}",
                "pwm_limits": [p.pwm_min, p.pwm_max],
                "direction": p.direction,
            }
        return summary


def fit_quadratic_motor_model(bench_data: BenchTestData) -> MotorParameters:
    """model.py:319-383: the calibration fit, host set-up algebra as in the reference (np.polyfit)."""
    errors = bench_data.validate()
    if errors:
        raise ValueError(f"Invalid bench data: {'; '.join(errors)}")
    pwm, thrust, rpm = np.array(bench_data.pwm_values), np.array(bench_data.thrust_measurements), np.array(bench_data.rpm_measurements)
    thrust_a, thrust_b, thrust_c = np.polyfit(pwm, thrust, 2)
    rpm_coefficient, rpm_offset = np.polyfit(pwm, rpm, 1)
    torque = np.array(bench_data.torque_measurements) if bench_data.torque_measurements else thrust * 0.1
    torque_coefficient = np.mean(torque / (rpm**2 + 1e-6))
    pwm_min, pwm_max = np.min(pwm), np.max(pwm)
    return MotorParameters(motor_id=bench_data.motor_id, thrust_a=thrust_a, thrust_b=thrust_b, thrust_c=thrust_c,
                           torque_coefficient=float(torque_coefficient), rpm_coefficient=rpm_coefficient, rpm_offset=rpm_offset, pwm_min=pwm_min,
                           pwm_max=pwm_max, pwm_idle=pwm_min + 0.1 * (pwm_max - pwm_min), rpm_max=np.max(rpm), direction=1, calibration_date=None,
                           calibration_notes="Fitted from bench test data")


def create_default_motor_model(**device_options) -> QuadraticMotorModel:
    """model.py:386-437: four equal hobby motors, directions CCW, CW, CCW, CW."""
    return QuadraticMotorModel({i: MotorParameters(motor_id=i, thrust_a=2.5, thrust_b=1.2, thrust_c=0.1, torque_coefficient=1e-7, rpm_coefficient=8000,
                                                   rpm_offset=500, direction=d) for i, d in enumerate((1, -1, 1, -1))}, **device_options)
