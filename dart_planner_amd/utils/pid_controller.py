"""Mirror of the reference's ``dart_planner.utils.pid_controller.PIDController`` (src/dart_planner/utils/pid_controller.py): same constructor,
members and method names.

Inside an :class:`~dart_planner_amd.control.onboard_controller.OnboardController` a PIDController is a VIEW: its gains are read into
``se3mpc_onboard_params`` on every call, its ``integral`` and ``last_error`` are words of the controller's device record, and the arithmetic of
``update`` runs in ``csrc/edge_device.hpp`` (pid_update) as part of ``compute_control_command``.  Standing alone it is one scalar recurrence with
no batch and no hot path: ``update`` then evaluates pid.py:25-51 on the host, term by term."""
from typing import Optional


class PIDController:
    def __init__(self, Kp: float, Ki: float, Kd: float, setpoint: float = 0.0, integral_limit: Optional[float] = None) -> None:
        self.Kp, self.Ki, self.Kd = Kp, Ki, Kd
        self.setpoint = setpoint
        self.integral_limit = integral_limit
        self._owner, self._index = None, None             # the OnboardController whose record holds integral / last_error, and the PID row
        self._integral, self._last_error = 0.0, 0.0

    def _bind(self, owner, index: int) -> None:
        integral, last_error = self.integral, self.last_error
        self._owner, self._index = owner, index
        if owner._state is not None or integral != 0.0 or last_error != 0.0:      # (a record that does not exist yet starts from zeros anyway)
            self.integral, self.last_error = integral, last_error

    def _word(self, off: int) -> float:
        return float(self._owner._record()[off + self._index])

    def _set_word(self, off: int, value) -> None:
        rec = self._owner._record()
        rec[off + self._index] = float(value)
        self._owner._write_record(rec)

    @property
    def integral(self) -> float:
        return self._integral if self._owner is None else self._word(0)

    @integral.setter
    def integral(self, value) -> None:
        if self._owner is None:
            self._integral = value
        else:
            self._set_word(0, value)

    @property
    def last_error(self) -> float:
        return self._last_error if self._owner is None else self._word(6)

    @last_error.setter
    def last_error(self, value) -> None:
        if self._owner is None:
            self._last_error = value
        else:
            self._set_word(6, value)

    def update(self, measured_value: float, dt: float) -> float:
        """pid.py:25-51.  (A PID of an OnboardController is updated by the controller's kernel; calling this on one moves the same record.)"""
        if dt <= 0:
            return 0.0
        error = self.setpoint - measured_value
        p_out = self.Kp * error
        integral = self.integral + error * dt
        if self.integral_limit:
            integral = min(max(integral, -self.integral_limit), self.integral_limit)
        self.integral = integral
        i_out = self.Ki * integral
        d_out = self.Kd * ((error - self.last_error) / dt)
        self.last_error = error
        return p_out + i_out + d_out

    def reset(self) -> None:
        self.integral = 0.0
        self.last_error = 0.0
