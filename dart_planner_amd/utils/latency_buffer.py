"""Mirrors of the reference's ``dart_planner.utils.latency_buffer`` (src/dart_planner/utils/latency_buffer.py): ``LatencyBuffer``,
``DroneStateLatencyBuffer`` and ``create_latency_buffer`` with the same constructors, members and method names.

``DroneStateLatencyBuffer`` keeps the delayed states in a one-drone device ring and its counters in a one-drone device record
(SE3MPC_LATENCY_STATE_WORDS doubles, include/se3mpc.h); every number it returns comes from ``se3mpc_latency_push_*``
(``csrc/edge_loop.hip``).  For B drones at once, and for the whole edge loop in one launch, use ``Ops.latency_push`` / ``Ops.edge_loop``."""
import time
from collections import deque
from typing import Any, Generic, Optional, TypeVar

import numpy as np

from ..capi import LATENCY_STATE_WORDS
from ..common.types import DroneState
from ..common.units import to_float

T = TypeVar("T")


class LatencyBuffer(Generic[T]):
    """The generic buffer (latency.py:20-115) holds arbitrary Python objects and does no arithmetic on them: it stays a HOST container.  Only
    ``DroneStateLatencyBuffer`` below has numbers to keep on the device."""

    def __init__(self, delay_s: float, dt: float, max_buffer_size: int = 1000):
        self.delay_s, self.dt, self.max_buffer_size = delay_s, dt, max_buffer_size
        self.required_size = max(1, int(round(delay_s / dt)))        # Python's round: half to even (2.5 -> 2, 1.5 -> 2)
        self.buffer_size = min(self.required_size, max_buffer_size)
        self.buffer = deque(maxlen=self.buffer_size)
        self.last_output: Optional[T] = None
        self.last_timestamp: float = 0.0
        self.total_samples = 0
        self.missed_samples = 0
        self.actual_delay_s = 0.0

    def push(self, data: T, timestamp: Optional[float] = None) -> T:
        timestamp = time.time() if timestamp is None else timestamp
        self.total_samples += 1
        if len(self.buffer) < self.buffer_size:                      # still filling: the current data goes straight through
            self.buffer.append((timestamp, data))
            self.missed_samples += 1
            return data
        self.last_timestamp, self.last_output = self.buffer.popleft()
        self.buffer.append((timestamp, data))
        self.actual_delay_s = timestamp - self.last_timestamp
        return self.last_output

    def get_delayed_data(self) -> Optional[T]:
        return self.last_output

    def get_actual_delay(self) -> float:
        return self.actual_delay_s

    def get_statistics(self) -> dict:
        return {"requested_delay_s": self.delay_s, "actual_delay_s": self.actual_delay_s, "buffer_size": len(self.buffer),
                "required_size": self.required_size, "total_samples": self.total_samples, "missed_samples": self.missed_samples,
                "fill_percentage": len(self.buffer) / self.buffer_size * 100 if self.buffer_size > 0 else 0}

    def reset(self):
        self.buffer.clear()
        self.last_output, self.last_timestamp = None, 0.0
        self.total_samples = self.missed_samples = 0
        self.actual_delay_s = 0.0

    def is_ready(self) -> bool:
        return len(self.buffer) >= self.buffer_size


class DroneStateLatencyBuffer(LatencyBuffer):
    """latency.py:118-144 on the device, one drone.  ``push`` hands the state's twelve numbers and the push's timestamp to
    ``se3mpc_latency_push_*``; while the buffer fills it returns the state it was given (as the reference does), afterwards a DroneState built
    from the numbers the kernel popped.  ``buffer`` keeps the pushed objects' handles in step with the ring (what ``len(buffer)`` and the members
    the ring has no slot for -- the state's own timestamp, motor_rpms -- are read from); ``total_samples``, ``missed_samples`` and
    ``actual_delay_s`` are read from the device record."""

    def __init__(self, delay_s: float, dt: float, max_buffer_size: int = 1000, *, precision: str = "f64", device=None):
        super().__init__(delay_s, dt, max_buffer_size)
        self.precision, self._device, self._ops, self._buf = precision, device, None, None

    def _get_ops(self):
        if self._ops is None:
            from ..ops import Ops, TorchBackend
            self._ops = Ops(TorchBackend(self._device))              # raises without a HIP device / built library
        return self._ops

    def _ring(self):
        if self._buf is None:
            self._buf = self._get_ops().latency_buffer(1, self.buffer_size, self.precision)
        return self._buf

    def _record(self) -> np.ndarray:
        return np.array(self._get_ops().be.to_host(self._ring()["state"]), dtype=float).reshape(LATENCY_STATE_WORDS)

    def _dev(self, a, kind=None):
        dt = {"f32": np.float32, "f64": np.float64}[kind or self.precision]
        return self._get_ops().be.from_host(np.ascontiguousarray(np.asarray(to_float(a), dtype=float).astype(dt)))

    def push(self, state, timestamp: Optional[float] = None):
        if not hasattr(state, "position") or not hasattr(state, "velocity"):
            raise ValueError("State must have position and velocity attributes")
        timestamp = time.time() if timestamp is None else timestamp
        ops = self._get_ops()
        vec = lambda name: self._dev(np.asarray(to_float(getattr(state, name, np.zeros(3))), float).reshape(1, 3))
        out = ops.latency_push(self._ring(), self._dev([float(timestamp)], "f64"), vec("position"), vec("velocity"), vec("attitude"), vec("angular_velocity"))
        if len(self.buffer) < self.buffer_size:
            self.buffer.append((timestamp, state))
            return state
        _, old = self.buffer.popleft()
        self.buffer.append((timestamp, state))
        host = lambda k: np.array(ops.be.to_host(out[k]), dtype=float).reshape(-1)
        self.last_timestamp = float(host("time")[0])
        self.last_output = DroneState(timestamp=getattr(old, "timestamp", self.last_timestamp), position=host("pos"), velocity=host("vel"), attitude=host("att"),
                                      angular_velocity=host("omega"), motor_rpms=getattr(old, "motor_rpms", None))
        return self.last_output

    def reset(self):
        self.buffer.clear()
        self.last_output, self.last_timestamp = None, 0.0
        self._buf = None                                             # a fresh ring and a zeroed record (se3mpc_latency_reset) at the next push

    # The three statistics live in the device record.  Assigning total_samples or actual_delay_s, as code written against the reference may,
    # writes the record's word; missed_samples follows from total_samples (min(total_samples, buffer_size)) and refuses any other value.
    def _set_word(self, index: int, value) -> None:
        if getattr(self, "_buf", None) is None and value == 0:
            return                                                   # (no ring yet: it starts from a zeroed record anyway)
        rec = self._record()
        rec[index] = float(value)
        self._ring()["state"] = self._get_ops().be.from_host(rec.reshape(1, LATENCY_STATE_WORDS))

    def _set_missed(self, value) -> None:
        if value != self.missed_samples:
            raise AttributeError("missed_samples is min(total_samples, buffer_size) of the device record: assign total_samples instead")

    total_samples = property(lambda self: int(self._record()[2]) if getattr(self, "_buf", None) is not None else 0, lambda self, v: self._set_word(2, v))
    missed_samples = property(lambda self: min(self.total_samples, self.buffer_size), _set_missed)
    actual_delay_s = property(lambda self: float(self._record()[3]) if getattr(self, "_buf", None) is not None else 0.0, lambda self, v: self._set_word(3, v))


def create_latency_buffer(delay_ms: float, dt_ms: float, state_type: str = "generic") -> LatencyBuffer:
    """latency.py:147-165."""
    cls = DroneStateLatencyBuffer if state_type == "drone_state" else LatencyBuffer
    return cls(delay_ms / 1000.0, dt_ms / 1000.0)
