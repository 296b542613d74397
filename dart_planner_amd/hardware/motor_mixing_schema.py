"""Mirror of the reference's ``dart_planner.hardware.motor_mixing_schema`` (src/dart_planner/hardware/motor_mixing_schema.py): the pydantic
model that validates a *motor_mixing* configuration section before a ``MotorMixingConfig`` is built from it.  Host-side validation only; no
number of the command path passes through it.  Same model name, fields, bounds and cross-field rules; as in the reference, keys the model
does not know are ignored (pydantic's default), so a misspelled key does not raise."""
from typing import List, Optional

from pydantic import BaseModel, Field, ValidationError, field_validator, model_validator  # noqa: F401  (ValidationError is part of the module's interface)

from .motor_mixer import QuadrotorLayout


class MotorMixingModel(BaseModel):
    layout: QuadrotorLayout = QuadrotorLayout.X_CONFIGURATION
    arm_length: float = Field(default=0.15, gt=0.0)
    motor_positions: List[List[float]]
    motor_directions: List[int]
    pwm_min: float = Field(default=0.0, ge=0.0, le=1.0)
    pwm_max: float = Field(default=1.0, ge=0.0, le=1.0)
    pwm_idle: float = Field(default=0.1, ge=0.0, le=1.0)
    pwm_scaling_factor: float = Field(default=2000.0, gt=0.0)
    thrust_coefficient: float = Field(default=1.0e-5, gt=0.0)
    torque_coefficient: float = Field(default=1.0e-7, gt=0.0)
    mixing_matrix: Optional[List[List[float]]] = None

    @field_validator("motor_directions")
    @classmethod
    def _directions(cls, v):
        if any(d not in (-1, 1) for d in v):
            raise ValueError("motor_directions must be ±1 values")
        return v

    @field_validator("motor_positions")
    @classmethod
    def _positions(cls, v):
        if len(v) != 4 or any(len(row) != 3 for row in v):
            raise ValueError("motor_positions must be 4 items of length 3")
        return v

    @field_validator("mixing_matrix")
    @classmethod
    def _matrix(cls, v):
        if v is not None and (len(v) != 4 or any(len(row) != 4 for row in v)):
            raise ValueError("mixing_matrix must be 4x4 list")
        return v

    @model_validator(mode="after")
    def _pwm_order(self):
        if self.pwm_max <= self.pwm_min:
            raise ValueError("pwm_max must be greater than pwm_min")
        if not self.pwm_min <= self.pwm_idle <= self.pwm_max:
            raise ValueError("pwm_idle must lie between pwm_min and pwm_max")
        return self
