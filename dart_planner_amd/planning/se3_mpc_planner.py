"""SE3MPCPlanner -- host-side mirror of the reference planner, backed by the HIP solver.

Same class / method names, arguments and error behaviour as
``src/dart_planner/planning/se3_mpc_planner.py`` of DART-Planner ("planner.py" below), so the
Planner->Controller contract (tests/test_planner_controller_contract.py of the reference) holds
unchanged: ``plan_trajectory(state, goal) -> Trajectory``.  Everything the reference computes with
NumPy loops + ``scipy.optimize.minimize(method="L-BFGS-B")`` between ``sense`` and ``act`` --
cold start, box, objective/gradient, the L-BFGS-B iterations, accelerations / attitudes / body
rates / thrust magnitudes -- runs in ONE launch of ``se3mpc_solve_*`` (dart_planner_amd/csrc/
solve_kernel.hip) on the MI355X.  There is no CPU fallback: without a HIP device or the built
library the first plan raises.

Beyond the reference (its own construct): ``plan_batch`` solves B
independent (state, goal) problems in one launch and ``plan_with_restarts`` runs R perturbed cold
starts of one problem and returns the best -- restart 0 is always the reference's cold start.
"""
from __future__ import annotations

import functools
import logging
import math
import ctypes
import time
from dataclasses import dataclass, fields
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from ..capi import Params, TASK_MESSAGES
from ..common.types import DroneState, Trajectory
from ..common.units import ensure_units, to_float
from .base_planner import BasePlanner, PlannerFactory

_log = logging.getLogger(__name__)


@dataclass(frozen=True)
class SE3MPCConfig:
    """planner.py:36-79 -- same fields and defaults; limits are SI magnitudes (a pint Quantity is
    accepted and converted)."""
    prediction_horizon: int = 6
    dt: float = 0.125                       # overridden by the timing manager (planner.py:99-105)
    max_velocity: float = 10.0              # m/s
    max_acceleration: float = 15.0          # m/s^2
    max_jerk: float = 20.0                  # m/s^3   (never read by the solver, as in the reference)
    max_thrust: float = 25.0                # N
    min_thrust: float = 2.0                 # N
    max_tilt_angle: float = math.pi / 4     # rad
    max_angular_velocity: float = 4.0       # rad/s   (never read)
    position_weight: float = 100.0
    velocity_weight: float = 10.0
    acceleration_weight: float = 1.0
    thrust_weight: float = 0.1
    angular_weight: float = 10.0            # never read
    obstacle_weight: float = 1000.0         # never read (planner.py:63)
    safety_margin: float = 1.5              # m
    max_iterations: int = 15
    convergence_tolerance: float = 5e-2

    def __post_init__(self):
        for name, unit in (("max_velocity", "m/s"), ("max_acceleration", "m/s^2"), ("max_jerk", "m/s^3"),
                           ("max_thrust", "N"), ("min_thrust", "N"), ("max_tilt_angle", "rad"),
                           ("max_angular_velocity", "rad/s"), ("safety_margin", "m")):
            object.__setattr__(self, name, float(ensure_units(getattr(self, name), unit, f"SE3MPCConfig.{name}")))


class SE3MPCPlanner(BasePlanner):
    """planner.py:82-757."""

    def __init__(self, config: Optional[SE3MPCConfig] = None, *, precision: str = "f64", device=None,
                 receding_horizon: bool = False) -> None:
        if config is None:
            config = SE3MPCConfig()
        elif isinstance(config, dict):      # PlannerFactory.create hands over a dict (base_planner.py:131)
            known = {f.name for f in fields(SE3MPCConfig)}
            config = SE3MPCConfig(**{k: v for k, v in config.items() if k in known})
        from ..common.timing_alignment import get_timing_manager
        aligned_dt = get_timing_manager().get_planner_dt()                      # planner.py:99-105
        config = SE3MPCConfig(**{**{f.name: getattr(config, f.name) for f in fields(SE3MPCConfig)}, "dt": aligned_dt})
        super().__init__({f.name: getattr(config, f.name) for f in fields(SE3MPCConfig)})   # planner.py:124-145
        self.se3_config = config
        self.mass = 1.5                                                          # planner.py:149-151
        self.gravity = 9.81
        self.hover_thrust = self.mass * self.gravity
        self.goal_position: Optional[np.ndarray] = None
        self.obstacles: List[Tuple[np.ndarray, float]] = []
        self.moving_obstacles: List[Tuple[np.ndarray, float, np.ndarray, float]] = []      # (centre, radius, velocity, timestamp)
        self.tracked_obstacles: List[Tuple[np.ndarray, np.ndarray, float]] = []            # (times (n,), centres (n, 3), radius)
        # planner.py:158-159.  The reference never assigns last_solution, so its warm start
        # (_create_warm_start, :294-327) is dead code and every solve is a cold start.  With
        # receding_horizon=True this planner does what that code intended: it keeps the last solution
        # and hands the shifted plan to the solver as x0.  Default: off = reference behaviour.
        self.last_solution: Optional[Dict[str, np.ndarray]] = None
        self.warm_start_enabled = True
        self.receding_horizon = bool(receding_horizon)
        self.planning_times: List[float] = []
        self.plan_count = 0
        self.convergence_history: List[bool] = []
        self.last_result: Dict[str, Any] = {}
        if precision not in ("f32", "f64"):
            raise ValueError("precision must be 'f32' or 'f64'")
        self.precision = precision
        self._device = device
        self._ops = None
        self._io = {}
        self._params_sig = None
        self._params_cached = None
        self.host_mapped_max_problems = 16      # at most this many problems: zero-copy through pinned host memory
        self.logger = _log

    # ------------------------------------------------------------------ device plumbing
    def _get_ops(self):
        if self._ops is None:
            from ..ops import Ops, TorchBackend
            self._ops = Ops(TorchBackend(self._device))      # raises without a HIP device / built library
        return self._ops

    def _params(self, **overrides) -> Params:
        c = self.se3_config
        has_goal = int(self.goal_position is not None)
        # the struct is rebuilt only when something it carries changed: the (frozen) config object itself, the vehicle constants, the goal's presence
        sig = (c, self.mass, self.gravity, has_goal)
        if self._params_sig != sig:
            self._params_cached = Params.reference_defaults(
                horizon=c.prediction_horizon, dt=c.dt, mass=self.mass, gravity=self.gravity,
                position_weight=c.position_weight, velocity_weight=c.velocity_weight,
                acceleration_weight=c.acceleration_weight, thrust_weight=c.thrust_weight,
                max_velocity=c.max_velocity, max_acceleration=c.max_acceleration, max_thrust=c.max_thrust,
                min_thrust=c.min_thrust, max_tilt_angle=c.max_tilt_angle, safety_margin=c.safety_margin,
                max_iterations=c.max_iterations, pgtol=c.convergence_tolerance, ftol=10 * c.convergence_tolerance,
                has_goal=has_goal)
            self._params_sig = sig
        if overrides and any(getattr(self._params_cached, k) != v for k, v in overrides.items()):
            return self._params_cached.copy(**overrides)
        return self._params_cached                            # (an override that repeats the cached value costs no copy: the per-plan path)

    # ------------------------------------------------------------------ planner.py:175-228
    def set_goal(self, goal_position) -> None:
        self.goal_position = np.array(ensure_units(goal_position, "m", "SE3MPCPlanner.set_goal"), dtype=float)
        self.logger.debug("SE(3) MPC goal set to: %s", self.goal_position)

    def add_obstacle(self, center, radius) -> None:
        c = np.array(ensure_units(center, "m", "SE3MPCPlanner.add_obstacle center"), dtype=float)
        r = float(ensure_units(radius, "m", "SE3MPCPlanner.add_obstacle radius"))
        self.obstacles.append((c, r))

    def add_moving_obstacle(self, center, radius, velocity, timestamp: float) -> None:
        """A sphere that moves with constant `velocity` (m/s): its centre is `center` at `timestamp`, on the clock of
        ``DroneState.timestamp``.  :meth:`plan_mppi` and :meth:`plan_batch_mppi` penalise every step of the horizon against the centre at
        that step's time (``se3mpc_mppi_moving_*``) and :meth:`obstacle_clearance` evaluates it at each row's timestamp;
        :meth:`plan_shooting` and the constraint helpers of the L-BFGS-B path see a snapshot at the state's timestamp."""
        c = np.array(ensure_units(center, "m", "SE3MPCPlanner.add_moving_obstacle center"), dtype=float)
        r = float(ensure_units(radius, "m", "SE3MPCPlanner.add_moving_obstacle radius"))
        v = np.array(to_float(velocity), dtype=float).reshape(3)
        self.moving_obstacles.append((c, r, v, float(timestamp)))

    def add_tracked_obstacle(self, times, centres, radius) -> None:
        """A sphere with a PREDICTED PATH -- a pedestrian track, another vehicle's published trajectory: its centre is `centres[i]` (n, 3) at
        `times[i]` (n,), rising, on the clock of ``DroneState.timestamp``; linear in between, held at both ends.  :meth:`plan_mppi` and
        :meth:`plan_batch_mppi` resample the polyline on the host, in float64, at the plan's step times and penalise every step of the horizon
        against the centre at that step (``se3mpc_mppi_tracks_*``; at most SE3MPC_MAX_TRACKS = 16 of them).  The other
        planning paths and the constraint helpers do not see tracked obstacles."""
        t = np.asarray(to_float(times), dtype=float).reshape(-1)
        c = np.array(ensure_units(centres, "m", "SE3MPCPlanner.add_tracked_obstacle centres"), dtype=float).reshape(-1, 3)
        r = float(ensure_units(radius, "m", "SE3MPCPlanner.add_tracked_obstacle radius"))
        if len(t) < 1 or len(t) != len(c) or np.any(np.diff(t) <= 0) or not (np.all(np.isfinite(t)) and np.all(np.isfinite(c))):
            raise ValueError("add_tracked_obstacle: times must be (n,) finite and strictly rising, centres (n, 3) finite, n >= 1")
        self.tracked_obstacles.append((t, c, r))

    def _tracked_obstacle_slab(self, obstacles, now: float) -> Optional[np.ndarray]:
        """(N, Kt, 4) rows (x, y, z, r) for the entries of tracked spheres: row [k][j] = tracked obstacle j at the plan's step k, i.e. k * dt
        seconds after `now` (the state's timestamp).  The polyline's times are rebased to `now` in float64 first, as
        :meth:`_moving_obstacle_table` rebases centres, then sampled linearly, held at both ends.  None when there is none, or when
        `obstacles` names a table of its own (or False)."""
        if not self.tracked_obstacles or not (obstacles is None or obstacles is True):
            return None
        N, dt = self.se3_config.prediction_horizon, self.se3_config.dt
        tau = np.arange(N, dtype=float) * dt
        slab = np.empty((N, len(self.tracked_obstacles), 4))
        for j, (t, c, r) in enumerate(self.tracked_obstacles):
            rel = t - float(now)
            for a in range(3):
                slab[:, j, a] = np.interp(tau, rel, c[:, a])
            slab[:, j, 3] = r
        return slab

    def clear_obstacles(self) -> None:
        self.obstacles.clear()
        self.moving_obstacles.clear()
        self.tracked_obstacles.clear()

    def sense(self, current_state: DroneState, goal_position):
        goal_position = ensure_units(goal_position, "m", "SE3MPCPlanner.sense goal_position")
        g = self.goal_position
        if g is not None:
            # (set_goal stores a float ndarray; an attribute written from outside may be anything)
            d = (g if type(g) is np.ndarray and g.dtype == np.float64 else np.asarray(to_float(g), float)) - goal_position
        if g is None or float(d @ d) > 0.25:                                    # planner.py:197-201 (norm > 0.5 m)
            self.goal_position = np.array(goal_position, dtype=float)           # = set_goal on the magnitudes already checked above
            if self.logger.isEnabledFor(logging.DEBUG):
                self.logger.debug("SE(3) MPC goal set to: %s", self.goal_position)
        return current_state, self.goal_position, list(self.obstacles)

    def plan(self, current_state: DroneState) -> Dict[str, np.ndarray]:
        return self._solve_se3_mpc(current_state)

    def act(self, solution: Dict[str, np.ndarray], current_state: DroneState, start_time: float) -> Trajectory:
        return self._create_trajectory_from_solution(solution, start_time)

    def plan_trajectory(self, current_state: DroneState, goal_position) -> Trajectory:
        t0 = time.perf_counter()
        current_state, _, _ = self.sense(current_state, goal_position)
        solution = self.plan(current_state)
        trajectory = self.act(solution, current_state, time.time())
        ms = (time.perf_counter() - t0) * 1e3
        self.planning_times.append(ms)
        self.plan_count += 1
        self._update_planning_stats(ms, bool(self.convergence_history[-1]))
        return trajectory

    # ------------------------------------------------------------------ planner.py:230-280 on the GPU
    def _solve_se3_mpc(self, current_state: DroneState) -> Dict[str, np.ndarray]:
        x0 = None
        if self.warm_start_enabled and self.last_solution is not None:          # planner.py:287-289
            x0 = self._create_warm_start(current_state, self.se3_config.prediction_horizon).reshape(1, -1)
        io = self._io
        N = self.se3_config.prediction_horizon
        if io.get("one_wave") and io["key"] == (1, N, "f32" if self.precision == "f32" else "f64", True) and self.host_mapped_max_problems >= 1:
            # steady state of the per-plan path: the three 3-vectors go straight into the pinned input rows (NumPy casts and broadcasts on assignment)
            sol, (fun, nit, nfev, status, task) = self._solve_one(io, to_float(current_state.position), to_float(current_state.velocity),
                                                                 None if self.goal_position is None else to_float(self.goal_position), x0, N)
        else:
            p0 = np.asarray(to_float(current_state.position), dtype=float).reshape(1, 3)
            v0 = np.asarray(to_float(current_state.velocity), dtype=float).reshape(1, 3)
            goal = None if self.goal_position is None else np.asarray(self.goal_position, float).reshape(1, 3)
            res = self._solve_batch(p0, v0, goal, x0, self.precision)
            fun, nit, nfev, status, task = res["info"][0].item()                 # (fun, nit, nfev, status, task): Python scalars in one call
            sol = {k: res[k][0] for k in ("positions", "velocities", "thrust_vectors", "accelerations", "attitudes", "body_rates", "thrusts")}
        converged = status == 0                                                  # result.success
        self.convergence_history.append(converged)
        self.last_result = dict(nit=nit, nfev=nfev, status=status, fun=fun, message=TASK_MESSAGES.get(task, ""))
        if not converged:
            self.logger.warning("SE(3) MPC optimization did not converge: %s", self.last_result["message"])
        if self.receding_horizon:
            self.last_solution = {k: sol[k].copy() for k in ("positions", "velocities", "thrust_vectors")}
        return sol

    def _solve_one(self, io, p0, v0, goal, x0, N):
        """The steady state of ONE plan (what `_solve_batch` does for B = 1 once its pinned buffers exist, without its general-case bookkeeping):
        inputs into the pinned buffer, `se3mpc_plan_host_*` (launch + completion ticket), one copy of the packed result, views into the copy."""
        prm = self._params(has_goal=int(goal is not None))
        hin = io["h_in_np"]
        hin[0] = p0; hin[1] = v0
        if goal is not None:
            hin[2] = goal
        hx0 = 0
        if x0 is not None:
            io["h_x0_np"][...] = x0
            hx0 = io["ptr_x0"]
        pin = io["ptr_in"]
        io["ticket"] = ticket = io["ticket"] + 1
        rc = io["plan_fn"](ctypes.byref(prm), 1, pin[0], pin[1], pin[2] if prm.has_goal else 0, hx0, *io["ptr_out"], io["ptr_done"], ticket, 2000.0,
                           io["plan_stream_handle"])
        if rc != 0:
            self._get_ops().lib._check("se3mpc_plan_host", rc)
        fast = io.get("fast")
        if fast is None:                                      # views of the pinned result, formed once per buffer set
            suf = io["key"][2]
            esz, dt = (4, np.float32) if suf == "f32" else (8, np.float64)
            o_x, o_acc, o_att, o_rates, o_thr, o_info, _ = self._get_ops()._packed_offsets(1, N, esz)
            nfl = (o_thr + N * esz) // esz
            fl = np.frombuffer(io["h_out_np"], dtype=dt, count=nfl)
            from ..ops import INFO_DTYPE
            fast = io["fast"] = (fl, np.frombuffer(io["h_out_np"], dtype=INFO_DTYPE, count=1, offset=o_info), o_acc // esz, o_att // esz, o_rates // esz, o_thr // esz,
                                 esz == 4)
        fl, info, a_acc, a_att, a_rates, a_thr, widen = fast
        allf = fl.astype(np.float64) if widen else fl.copy()                     # ONE copy: the arrays below do not alias the pinned buffer
        rows = allf[:18 * N].reshape(6 * N, 3)                                   # [P | V | T | acc | att | rates], N rows of 3 each (B = 1: the fields are adjacent)
        sol = {"positions": rows[0:N], "velocities": rows[N:2 * N], "thrust_vectors": rows[2 * N:3 * N], "accelerations": rows[3 * N:4 * N],
               "attitudes": rows[4 * N:5 * N], "body_rates": rows[5 * N:6 * N], "thrusts": allf[a_thr:a_thr + N]}
        return sol, info[0].item()

    def _solve_batch(self, p0, v0, goal, x0, precision, want_trajectory=True) -> Dict[str, np.ndarray]:
        """B problems in one launch; host float64 arrays in, host float64 arrays out.  Steady state: the
        stacked (p0, v0, goal) is written into a pinned host buffer, then either (a handful of problems)
        the kernel works on the pinned buffers in place, or ONE async H2D copy, one launch and ONE async D2H
        copy of the packed result; one stream synchronise; the returned arrays are fresh copies decoded from
        the pinned result buffer."""
        import torch
        ops = self._get_ops()
        dev = ops.be.device
        suf = "f32" if precision == "f32" else "f64"
        dt = torch.float32 if suf == "f32" else torch.float64
        B, N = p0.shape[0], self.se3_config.prediction_horizon
        prm = self._params(has_goal=int(goal is not None))
        mapped = B <= self.host_mapped_max_problems
        key = (B, N, suf, mapped)
        io = self._io
        if io.get("key") != key:
            pin = dev.type == "cuda"
            nbytes = ops.packed_size(B, N, suf)
            io = self._io = dict(key=key,
                                 h_in=torch.empty((3, B, 3), dtype=dt, pin_memory=pin),
                                 h_out=torch.empty((nbytes,), dtype=torch.uint8, pin_memory=pin))
            if mapped:
                io["h_x0"] = torch.empty((B, 9 * N), dtype=dt, pin_memory=pin)
                io["h_x0_np"] = io["h_x0"].numpy()
            else:
                io["d_in"] = torch.empty((3, B, 3), dtype=dt, device=dev)
                io["d_out"] = ops.be.empty((nbytes,), "u8")
            io["h_in_np"] = io["h_in"].numpy()
            io["h_out_np"] = io["h_out"].numpy()
            if mapped:
                # the raw addresses of the per-plan call (se3mpc_solve_* on the pinned buffers), computed once per buffer set
                esz = 4 if suf == "f32" else 8
                o_x, o_acc, o_att, o_rates, o_thr, o_info, _ = ops._packed_offsets(B, N, esz)
                pin, base, stepb = io["h_in"].data_ptr(), io["h_out"].data_ptr(), B * 3 * esz
                io["ptr_in"] = (pin, pin + stepb, pin + 2 * stepb)
                io["ptr_out"] = (base + o_x, base + o_info, base + o_acc, base + o_att, base + o_rates, base + o_thr)
                io["ptr_x0"] = io["h_x0"].data_ptr()
                # the host-latency entry point (se3mpc_plan_host_*: launch + spin on a completion word the kernel stores last) serves
                # batches that fit ONE wavefront: a lone problem, or 64 / lanes-per-problem of them
                lanes = 64 if B == 1 else (8 if N <= 8 else 16 if N <= 16 else 32 if N <= 32 else 64)
                io["one_wave"] = B * lanes <= 64
                io["h_done"] = torch.zeros((8,), dtype=torch.int64, pin_memory=dev.type == "cuda")
                io["ptr_done"] = io["h_done"].data_ptr()
                io["ticket"] = 0
                io["plan_fn"] = getattr(ops.lib._dll, f"se3mpc_plan_host_{suf}")
                # the launch touches nothing but this planner's own pinned buffers: a stream of its own (no ordering against the caller's
                # work, no per-plan current-stream lookup)
                io["plan_stream"] = torch.cuda.Stream(dev) if (io["one_wave"] and dev.type == "cuda") else None
                io["plan_stream_handle"] = None if io["plan_stream"] is None else io["plan_stream"].cuda_stream
        if mapped and io["one_wave"]:
            cur, stream_handle = None, io["plan_stream_handle"]
        else:
            cur = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
            stream_handle = None if cur is None else cur.cuda_stream
        hin = io["h_in_np"]
        hin[0] = p0; hin[1] = v0
        hin[2] = goal if goal is not None else 0.0
        if mapped:
            # a handful of problems: the kernel reads the pinned inputs and writes the pinned result in place
            hx0 = None
            if x0 is not None:
                io["h_x0_np"][...] = x0
                hx0 = io["h_x0"]
            pin = io["ptr_in"]
            if io["one_wave"]:
                # launch + wait in ONE C call (no hipStreamSynchronize: the kernel's last store is the completion ticket the call spins on)
                io["ticket"] = ticket = io["ticket"] + 1
                rc = io["plan_fn"](ctypes.byref(prm), B, pin[0], pin[1], pin[2] if prm.has_goal else 0, io["ptr_x0"] if hx0 is not None else 0,
                                   *io["ptr_out"], io["ptr_done"], ticket, 2000.0, stream_handle)
                if rc != 0:
                    ops.lib._check(f"se3mpc_plan_host_{suf}", rc)
                cur = None                                    # nothing left to wait for
            else:
                ops.lib.call("solve", suf, B, pin[0], pin[1], pin[2] if prm.has_goal else 0, io["ptr_x0"] if hx0 is not None else 0, *io["ptr_out"],
                             stream_handle, params=prm)     # = ops.solve_packed(host_mapped=True) without re-validating the same buffers every plan
        else:
            io["d_in"].copy_(io["h_in"], non_blocking=True)
            dx0 = None if x0 is None else torch.from_numpy(np.ascontiguousarray(x0)).to(device=dev, dtype=dt)
            ops.solve_packed(prm, io["d_in"], x0=dx0, out=io["d_out"])
            io["h_out"].copy_(io["d_out"], non_blocking=True)
        if cur is not None:
            cur.synchronize()
        res = ops.unpack_solution(io["h_out_np"], B, N, suf)
        x = res["x"]
        res.update(positions=x[:, :3 * N].reshape(B, N, 3), velocities=x[:, 3 * N:6 * N].reshape(B, N, 3),
                   thrust_vectors=x[:, 6 * N:].reshape(B, N, 3))
        return res

    # ------------------------------------------------------------------ batched extensions
    def plan_batch(self, positions, velocities, goals, x0=None, precision: Optional[str] = None) -> Dict[str, np.ndarray]:
        """Solve B independent problems (the reference would loop plan_trajectory B times).
        positions, velocities, goals: (B, 3).  Returns arrays with a leading B axis plus ``info``
        (structured: fun, nit, nfev, status, task)."""
        p0 = np.asarray(to_float(positions), float).reshape(-1, 3)
        v0 = np.asarray(to_float(velocities), float).reshape(-1, 3)
        g = np.asarray(to_float(goals), float).reshape(-1, 3)
        if not (p0.shape == v0.shape == g.shape):
            raise ValueError("positions, velocities and goals must all be (B, 3)")
        return self._solve_batch(p0, v0, g, x0, precision or "f32")

    def plan_with_restarts(self, current_state: DroneState, goal_position, n_restarts: int = 256, sigma: float = 1.0,
                           seed: int = 0, precision: Optional[str] = None, mapper=None, safety_margin: float = 1.0,
                           occupancy_threshold: float = 0.6) -> Trajectory:
        """R cold starts of ONE problem: restart 0 is the reference's straight-line start, restarts
        1..R-1 add N(0, sigma) newtons to its thrust block (the solver projects into the box);
        the restart with the lowest final objective wins.  With a `mapper` (the device
        ExplicitGeometricMapper) the winner is taken among the restarts whose positions pass its
        is_trajectory_safe check (mapper.py:195-219, all R plans in one launch) -- what
        cloud/main_improved_se3.py:128 does to a single plan after the fact; if none passes, the lowest
        objective wins as before and ``last_result["n_safe"]`` is 0."""
        current_state, _, _ = self.sense(current_state, goal_position)
        N, R = self.se3_config.prediction_horizon, int(n_restarts)
        p0 = np.tile(np.asarray(to_float(current_state.position), float), (R, 1))
        v0 = np.tile(np.asarray(to_float(current_state.velocity), float), (R, 1))
        g = np.tile(self.goal_position, (R, 1))
        x0 = np.tile(self._cold_start(p0[0], v0[0], self.goal_position), (R, 1))
        rng = np.random.default_rng(seed)
        x0[1:, 6 * N:] += rng.normal(0.0, sigma, (R - 1, 3 * N))
        res = self._solve_batch(p0, v0, g, x0, precision or self.precision)
        fun = np.array(res["info"]["fun"], dtype=float)
        self.last_result = dict(fun_cold_start=float(fun[0]))
        if mapper is not None:
            safe, _ = mapper.trajectories_safe(res["positions"], safety_margin, occupancy_threshold)
            self.last_result["n_safe"] = int(safe.sum())
            if safe.any():
                fun = np.where(safe, fun, np.inf)
        best = int(np.argmin(fun))
        self.last_result.update(best_restart=best, fun=float(res["info"]["fun"][best]))
        sol = {k: res[k][best] for k in ("positions", "velocities", "thrust_vectors", "accelerations", "attitudes",
                                         "body_rates", "thrusts")}
        return self._create_trajectory_from_solution(sol, time.time())

    def _obstacle_table(self, obstacles) -> Optional[np.ndarray]:
        """(K, 4) rows (cx, cy, cz, r) for the obstacle-aware loop: None / True = the planner's own list (add_obstacle, planner.py:183-187 --
        what the cloud loop refreshes from the mapper every cycle, cloud/main_improved_threelayer.py:381-398), False = ignore it, an array =
        those spheres.  None when there is nothing to avoid."""
        if obstacles is False:
            return None
        if obstacles is None or obstacles is True:
            if not self.obstacles:
                return None
            return np.array([[*np.asarray(to_float(c), float).reshape(3), float(r)] for c, r in self.obstacles], dtype=float)
        sph = np.asarray(obstacles, float).reshape(-1, 4)
        return sph if len(sph) else None

    def _moving_obstacle_table(self, obstacles, now: float) -> Optional[np.ndarray]:
        """(K, 7) rows (cx, cy, cz, r, vx, vy, vz) holding at time `now` (the state's timestamp), for the entries of moving spheres, which
        then take sphere_t0 = 0: `obstacles` as in :meth:`_obstacle_table`, the planner's own list being its static obstacles (zero velocity)
        followed by its moving ones, each centre rebased in float64 on the host, c + v * (now - timestamp) -- the kernels round times to
        their own type, and a float32 epoch time has an ulp of minutes.  An array may be (K, 4) (static) or (K, 7) (taken to hold at
        `now`).  None when there is nothing to avoid."""
        if obstacles is False:
            return None
        if obstacles is None or obstacles is True:
            rows = [[*np.asarray(to_float(c), float).reshape(3), float(r), 0.0, 0.0, 0.0] for c, r in self.obstacles]
            rows += [[*(c + v * (float(now) - t)), r, *v] for c, r, v, t in self.moving_obstacles]
            return np.array(rows, dtype=float) if rows else None
        a = np.asarray(obstacles, float)
        if a.ndim == 2 and a.shape[1] == 7:
            return a.copy() if len(a) else None
        sph = a.reshape(-1, 4)
        return np.concatenate([sph, np.zeros((len(sph), 3))], axis=1) if len(sph) else None

    def plan_shooting(self, current_state: DroneState, goal_position, n_samples: int = 8192, iters: int = 16, step: float = 0.9,
                      sigma: float = 2.0, seed: int = 0, precision: str = "f32", obstacles=None,
                      obstacle_weight: Optional[float] = None) -> Trajectory:
        """The shooting-form counterpart of :meth:`plan_trajectory` (the build's construct, like the restarts): `n_samples` thrust
        sequences around hover are each descended `iters` projected-gradient iterations on the device (ONE launch,
        ``se3mpc_rollout_iterate_*``; with several ranks the samples shard and one all-reduce(MIN) picks the winner,
        ``distributed.sharded_shooting_plan``), the best one is rolled out (``se3mpc_rollout_cost_grad_*`` with states) and its
        accelerations / attitudes / body rates / thrust magnitudes extracted (``se3mpc_extract_*``).  Unlike the reference's solve, whose
        dynamics constraints never reach the optimiser, this plan satisfies the dynamics by construction.
        obstacles: the sphere list the descent avoids (``_obstacle_table``: by default the planner's own, which the reference keeps and
        never uses) through the obstacle-aware loop ``se3mpc_rollout_iterate_obstacles_*``: the objective gains
        obstacle_weight * sum max(0, -(|P_k - c_j|^2 - (r_j + safety_margin)^2))^2 (obstacle_weight defaults to the config's, planner.py:63);
        ``last_result["penalty"]`` is what is left of it at the returned plan (0 = every margin kept).  Moving obstacles
        (:meth:`add_moving_obstacle`) are a snapshot at the state's timestamp: the descent does not move them along the horizon."""
        import torch
        import torch.distributed as dist
        from ..distributed import sharded_shooting_plan
        current_state, _, _ = self.sense(current_state, goal_position)
        ops = self._get_ops()
        prm = self._params()
        N = self.se3_config.prediction_horizon
        p0 = np.asarray(to_float(current_state.position), float)
        v0 = np.asarray(to_float(current_state.velocity), float)
        if (self.moving_obstacles and (obstacles is None or obstacles is True)) or (np.ndim(obstacles) == 2 and np.shape(obstacles)[1] == 7):
            sph = self._mppi_tables(obstacles, current_state.timestamp)[0]          # the snapshot at the state's timestamp
        else:
            sph = self._obstacle_table(obstacles)
        w_obs = float(self.se3_config.obstacle_weight if obstacle_weight is None else obstacle_weight)
        single = not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
        if single and getattr(ops.be, "graph_capable", False):
            return self._plan_shooting_captured(ops, prm, p0, v0, int(n_samples), int(iters), float(step), float(sigma), int(seed), precision, sph, w_obs)
        best = sharded_shooting_plan(ops, prm, p0, v0, self.goal_position, n_samples, iters, step, sigma, seed, precision, spheres=sph,
                                     obstacle_weight=w_obs)
        dev = ops.be.device
        col = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, float).reshape(-1, 1))).to(dev)
        T = col(best["T"].reshape(-1))
        cost, _, P, V = ops.rollout_cost_grad(prm, col(p0), col(v0), col(self.goal_position), T, want_grad=False, want_states=True)
        acc, att, rates, thr = ops.extract(prm, T)
        h = lambda a, shape: ops.be.to_host(a)[:, 0].reshape(shape).astype(float)
        self.last_result = dict(cost=float(ops.be.to_host(cost)[0]), sample=int(best["sample"]), owner=int(best["owner"]), n_samples=int(n_samples),
                                iters=int(iters), T=best["T"])
        if sph is not None:
            # what is left of the penalty at the returned plan (0 = every sphere's margin kept at every step)
            o = ops.rollout_iterate(prm, col(p0), col(v0), col(self.goal_position), T, 0, 0.0, want_grad=False, spheres=col(sph.reshape(-1)).reshape(-1, 4).contiguous(),
                                    obstacle_weight=w_obs)
            self.last_result.update(penalty=float(ops.be.to_host(o["penalty"])[0]), cost_with_penalty=float(ops.be.to_host(o["cost"])[0]))
        sol = {"positions": h(P, (N, 3)), "velocities": h(V, (N, 3)), "thrust_vectors": best["T"], "accelerations": h(acc, (N, 3)),
               "attitudes": h(att, (N, 3)), "body_rates": h(rates, (N, 3)), "thrusts": h(thr, (N,))}
        return self._create_trajectory_from_solution(sol, time.time())

    def _plan_shooting_captured(self, ops, prm, p0, v0, n_samples, iters, step, sigma, seed, precision, sph=None, w_obs=1000.0) -> Trajectory:
        """plan_shooting on one rank as ONE hipGraph replay: 72 B in through a pinned buffer, the sample set (fixed by its seed) resident,
        descend (``se3mpc_rollout_iterate_*`` / ``_obstacles_*``) -> ``se3mpc_shooting_finish_*`` (fold the argmin keys, roll the winner's thrust
        column out in float64 with states, extract, one packed result stored into a pinned buffer); the host synchronises once.  Same winner and
        thrust sequence as the eager path (`distributed.sharded_shooting_plan` + rollout + extract), without its ~10 host round trips."""
        import torch
        from ..distributed import shooting_samples
        N = prm.horizon
        K = 0 if sph is None else len(sph)
        key = (N, n_samples, iters, step, sigma, seed, precision, bytes(prm), K, w_obs)
        g = self._shooting_graphs.get(key) if hasattr(self, "_shooting_graphs") else None
        if g is None:
            if not hasattr(self, "_shooting_graphs"):
                self._shooting_graphs = {}
            dev = ops.be.device
            dt = torch.float32 if precision == "f32" else torch.float64
            io = dict(h_in=torch.zeros(9, dtype=torch.float64).pin_memory(), d_in=torch.zeros(9, dtype=torch.float64, device=dev),
                      h_out=torch.zeros(19 * N + 3, dtype=torch.float64).pin_memory(), h_key=torch.zeros(1, dtype=torch.int64).pin_memory(),
                      samples=shooting_samples(prm, n_samples, sigma, seed, dev, dt), wk=torch.zeros(((n_samples + 63) // 64,), dtype=torch.int64, device=dev))
            if K:                                                                  # the sphere table travels with every plan (the mapper refreshes it each cycle)
                io.update(h_sph=torch.zeros((K, 4), dtype=torch.float64).pin_memory(), d_sph=torch.zeros((K, 4), dtype=torch.float64, device=dev))

            io["wide"] = torch.empty((3, 3, n_samples), dtype=dt, device=dev)      # (p0, v0, goal) of every sample: the lane layout of the descent
            io["h_in_np"], io["h_out_np"], io["h_key_np"] = io["h_in"].numpy(), io["h_out"].numpy(), io["h_key"].numpy()
            if K:
                io["h_sph_np"] = io["h_sph"].numpy()

            def body():
                io["d_in"].copy_(io["h_in"], non_blocking=True)
                wide = io["wide"]
                wide.copy_(io["d_in"].view(3, 3, 1).expand(3, 3, n_samples))     # cast + broadcast in one kernel
                sph_d = None
                if K:
                    io["d_sph"].copy_(io["h_sph"], non_blocking=True)
                    sph_d = io["d_sph"].to(dt)
                out = ops.rollout_iterate(prm, wide[0], wide[1], wide[2], io["samples"], iters, step, want_grad=False, wave_keys=io["wk"], index_base=0,
                                          spheres=sph_d, obstacle_weight=w_obs, want_penalty=False)
                # the tail in ONE launch (se3mpc_shooting_finish_*): fold the keys, roll the winner out in float64 with states, extract, the penalty left
                # at it; the packed result and the key are stored straight into the pinned host buffers
                ops.shooting_finish(prm, out["T"], io["wk"], io["d_in"], io["h_out"], key_out=io["h_key"], spheres=io["d_sph"] if K else None,
                                    obstacle_weight=w_obs)

            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                body()                                                             # warm-up outside the capture
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                body()
            if len(self._shooting_graphs) >= 4:                                    # a new seed / sample count is a new resident sample set and a new capture
                self._shooting_graphs.pop(next(iter(self._shooting_graphs)))
            g = self._shooting_graphs[key] = (graph, io)
        graph, io = g
        hin = io["h_in_np"]
        hin[0:3] = p0; hin[3:6] = v0; hin[6:9] = self.goal_position
        if K:
            io["h_sph_np"][...] = sph
        graph.replay()
        torch.cuda.current_stream(ops.be.device).synchronize()
        r = io["h_out_np"]
        kh = int(io["h_key_np"][0]) & 0xFFFFFFFFFFFFFFFF
        blk = lambda i: r[3 * N * i:3 * N * (i + 1)].reshape(N, 3).copy()
        self.last_result = dict(cost=float(r[19 * N]), sample=int(ops.lib.key_index(kh)), owner=0, n_samples=n_samples, iters=iters, T=blk(2))
        if K:
            self.last_result.update(penalty=float(r[19 * N + 1]), cost_with_penalty=float(r[19 * N + 2]))
        sol = {"positions": blk(0), "velocities": blk(1), "thrust_vectors": blk(2), "accelerations": blk(3), "attitudes": blk(4),
               "body_rates": blk(5), "thrusts": r[18 * N:19 * N].copy()}
        return self._create_trajectory_from_solution(sol, time.time())

    # ------------------------------------------------------------------ MPPI (the build's sampling planner)
    # Defaults from the (sigma, temperature, iters) sweep of DESIGN.md 5.8 (profiles/mppi_tuning.json, tools/gpu_probe_mppi.py, 1024 samples):
    # on the obstacle scene (10 Hz, N = 30) sigma = 4 N, temperature = 100 reaches the lowest cost of the 8-iteration grid (ends 0.8 m from the
    # goal, safe); sigma = 1 N barely leaves hover in 8 iterations and temperature = 10^4 averages the samples flat.  On the cfg-2 distribution
    # (dt = 0.1) sigma = 4 N is again best and temperatures 10 .. 1000 agree within 0.3 %.  8 iterations: 1.2 ms per plan (16 halve the
    # distance left to the goal for twice the time).
    MPPI_SAMPLES = 1024
    MPPI_ITERS = 8
    MPPI_SIGMA = 4.0
    MPPI_TEMPERATURE = 100.0

    def _mppi_nominal(self, N: int, warm_start: bool):
        """The nominal thrust sequence (N, 3) this cycle starts from and the shift applied: the last cycle's nominal shifted like the warm start
        (oracle.warm_start / _create_warm_start: drop step 0, append hover) when it exists for this horizon and goal, else hover."""
        st = getattr(self, "_mppi_state", None)
        hover = np.tile([0.0, 0.0, self.hover_thrust], (N, 1))
        if not warm_start or st is None or st["U"].shape[0] != N or not np.array_equal(st["goal"], self.goal_position):
            return hover, 0
        U = np.empty((N, 3))
        U[:N - 1] = st["U"][1:]
        U[N - 1] = hover[0]
        return U, 1

    MPPI_SPLIT_SAMPLES = 256          # splits="auto": one workgroup per 256 samples (one chunk each)
    MPPI_SPLIT_WORKGROUPS = 1024      # ... and at most 4 workgroups per CU x 256 CUs over a batch, the residency of __launch_bounds__(256, 4)

    @classmethod
    def _mppi_splits(cls, splits, n_samples: int, n_problems: int = 1) -> Optional[int]:
        """The `splits` argument of the MPPI entry points resolved: None (one workgroup per problem, ``se3mpc_mppi_*``) or the number of
        workgroups per problem for ``se3mpc_mppi_split_*``.  "auto": n_samples // 256, at most 1024 workgroups over the batch, lowered to the
        next count that gives every split whole wavefronts; where that leaves one split, None: the same bytes from one launch instead of
        iters + 1 (measured 3 % faster)."""
        if splits is None:
            return None
        if splits == "auto":
            g = max(1, min(int(n_samples) // cls.MPPI_SPLIT_SAMPLES, cls.MPPI_SPLIT_WORKGROUPS // max(int(n_problems), 1)))
            while g > 1 and int(n_samples) % (64 * g):
                g -= 1
            return g if g > 1 else None
        if isinstance(splits, (bool, str)) or int(splits) != splits:
            raise ValueError(f"splits: expected None, \"auto\" or an integer, got {splits!r}")
        return int(splits)

    @staticmethod
    def _mppi_op(ops, splits, *a, workspace=None, **kw):
        """``Ops.mppi`` (splits None) or ``Ops.mppi_split``: the one place the two paths of the planner differ."""
        if splits is None:
            return ops.mppi(*a, **kw)
        return ops.mppi_split(*a, splits=splits, workspace=workspace, **kw)

    def plan_mppi(self, current_state: DroneState, goal_position, n_samples: int = MPPI_SAMPLES, iters: int = MPPI_ITERS,
                  sigma: float = MPPI_SIGMA, temperature: float = MPPI_TEMPERATURE, seed: int = 0, precision: str = "f32", obstacles=None,
                  obstacle_weight: Optional[float] = None, warm_start: bool = True, splits=None) -> Trajectory:
        """MPPI, the sampling counterpart of :meth:`plan_shooting` (the build's construct): `iters` iterations of perturb-the-nominal (Philox
        normals of std `sigma` newtons) / roll out `n_samples` samples / weight by exp(-(cost - min) / temperature) / move the nominal to the
        weighted mean, in ONE launch of ``se3mpc_mppi_*``; the nominal is then rolled out in float64 with states and extracted
        (``se3mpc_shooting_finish_*`` through the kernel's argmin key).  The nominal is kept between calls: with ``warm_start`` the next
        plan starts from it shifted by one step (hover appended), a goal change through ``sense`` resets it to hover, and every call draws
        fresh noise (the iteration counter advances).  obstacles / obstacle_weight as :meth:`plan_shooting`.  ``last_result``: cost (the
        running cost at the plan), penalty, cost_with_penalty, trace (the minimum sample cost per iteration), shift (1 = warm-started),
        iter_base, n_samples, iters, splits.  With a graph-capable backend the whole plan is one hipGraph replay.
        ``splits``: None = one workgroup, one launch; an integer spreads the samples over that many workgroups (``se3mpc_mppi_split_*``,
        one launch per iteration and one more; n_samples must be a multiple of 64 * splits); "auto" = n_samples // 256, and the one-launch
        path where that is 1.
        The split plan differs from the unsplit one in the last bits of its float64 sums only (``splits`` = 1: not at all).
        Tracked obstacles (:meth:`add_tracked_obstacle`) take the same eager path through ``se3mpc_mppi_tracks_*``, the planner's whole
        table as its moving rows (zero velocities where nothing moves); ``splits`` raises there too.
        Moving obstacles (:meth:`add_moving_obstacle`, or an ``obstacles`` array of (K, 7) rows (cx, cy, cz, r, vx, vy, vz) holding at the
        state's timestamp): with at least one non-zero velocity the plan is ``se3mpc_mppi_moving_*`` on the table rebased to the state's
        timestamp (:meth:`_moving_obstacle_table`), launch by launch -- the EAGER path even on a graph-capable backend, since the rebased
        table changes every call and the captured graph's pinned input does not carry it.  ``se3mpc_shooting_finish_*`` knows only static
        spheres, so it runs without them: ``cost_with_penalty`` is the MPPI entry's own cost of the nominal (the moving penalty included),
        ``cost`` the finish's running cost and ``penalty`` their difference.  The split form is not built: ``splits`` then raises
        ValueError."""
        current_state, _, _ = self.sense(current_state, goal_position)
        ops = self._get_ops()
        prm = self._params()
        N = self.se3_config.prediction_horizon
        p0 = np.asarray(to_float(current_state.position), float)
        v0 = np.asarray(to_float(current_state.velocity), float)
        sph, moving = self._mppi_tables(obstacles, current_state.timestamp)
        w_obs = float(self.se3_config.obstacle_weight if obstacle_weight is None else obstacle_weight)
        U0, shift = self._mppi_nominal(N, warm_start)
        it_base = getattr(self, "_mppi_iter_base", 0)
        splits = self._mppi_splits(splits, n_samples)
        if moving is not None and splits is not None:
            raise ValueError("plan_mppi: the split form is not built for moving obstacles (se3mpc_mppi_moving_* has no split entry): use splits=None")
        slab = self._tracked_obstacle_slab(obstacles, current_state.timestamp)
        if slab is not None and splits is not None:
            raise ValueError("plan_mppi: the split form is not built for tracked obstacles (se3mpc_mppi_tracks_* has no split entry): use splits=None")
        args = (ops, prm, p0, v0, U0, int(n_samples), int(iters), float(sigma), float(temperature), int(seed), precision, sph, w_obs, it_base, splits)
        if slab is not None:                                          # the tracked rows come behind the whole table, moving or not
            tab = self._moving_obstacle_table(obstacles, current_state.timestamp)
            r, trace = self._plan_mppi_eager(*args, moving=np.zeros((0, 7)) if tab is None else tab, tracks=slab)
        elif moving is not None:
            r, trace = self._plan_mppi_eager(*args, moving=moving)
        elif getattr(ops.be, "graph_capable", False):
            r, trace = self._plan_mppi_captured(*args)
        else:
            r, trace = self._plan_mppi_eager(*args)
        self._mppi_iter_base = (it_base + int(iters)) & 0xFFFFFFFF
        blk = lambda i: r[3 * N * i:3 * N * (i + 1)].reshape(N, 3).copy()
        self._mppi_state = dict(U=blk(2), goal=np.array(self.goal_position, dtype=float))
        self.last_result = dict(cost=float(r[19 * N]), penalty=float(r[19 * N + 1]), cost_with_penalty=float(r[19 * N + 2]), trace=trace,
                                shift=shift, iter_base=it_base, n_samples=int(n_samples), iters=int(iters), U=blk(2), splits=splits)
        sol = {"positions": blk(0), "velocities": blk(1), "thrust_vectors": blk(2), "accelerations": blk(3), "attitudes": blk(4),
               "body_rates": blk(5), "thrusts": r[18 * N:19 * N].copy()}
        return self._create_trajectory_from_solution(sol, time.time())

    def _mppi_tables(self, obstacles, now: float):
        """What the MPPI entries take: (the (K, 4) table for ``se3mpc_mppi_*`` | None, the (K, 7) table of :meth:`_moving_obstacle_table`
        for ``se3mpc_mppi_moving_*`` when at least one sphere moves | None)."""
        tab = self._moving_obstacle_table(obstacles, now)
        if tab is None:
            return None, None
        return np.ascontiguousarray(tab[:, :4]), (tab if np.any(tab[:, 4:] != 0.0) else None)

    def _plan_mppi_eager(self, ops, prm, p0, v0, U0, n_samples, iters, sigma, temperature, seed, precision, sph, w_obs, it_base, splits=None,
                         moving=None, tracks=None):
        """plan_mppi launch by launch (any backend): -> (packed float64 result of se3mpc_shooting_finish_*, trace).  moving: the (K, 7)
        table of :meth:`_moving_obstacle_table` -- ``se3mpc_mppi_moving_*`` with sphere_t0 = 0, the finish without spheres and the packed
        (cost, penalty, cost_with_penalty) completed from the MPPI entry's own cost.  tracks: the (N, Kt, 4) slab of
        :meth:`_tracked_obstacle_slab` behind that table (``se3mpc_mppi_tracks_*``)."""
        N = prm.horizon
        be = ops.be
        suf = "f32" if precision == "f32" else "f64"
        col = lambda a, kind: be.from_host(np.ascontiguousarray(np.asarray(a, float).reshape(-1, 1).astype(np.float32 if kind == "f32" else np.float64)))
        state = be.from_host(np.concatenate([p0, v0, self.goal_position]).astype(np.float64))
        if moving is not None:
            npdt = np.float32 if suf == "f32" else np.float64
            dev = lambda a: be.from_host(np.ascontiguousarray(a.astype(npdt)))
            tables = dict(spheres=dev(moving[:, :4]) if len(moving) else None, sphere_vel=dev(moving[:, 4:]) if len(moving) else None, sphere_t0=0.0)
            entry = ops.mppi if tracks is None else functools.partial(ops.mppi_tracks, tracks=dev(tracks))
            out = entry(prm, col(p0, suf), col(v0, suf), col(self.goal_position, suf), col(U0, suf), n_samples, iters, sigma, temperature, seed=seed,
                        iter_base=it_base, obstacle_weight=w_obs, **tables)
            res = be.empty((19 * N + 3,), "f64")
            ops.shooting_finish(prm, out["U"], out["keys"], state, res)
            r = np.asarray(be.to_host(res), dtype=float).copy()
            r[19 * N + 2] = float(np.asarray(be.to_host(out["cost"]), dtype=float)[0])
            r[19 * N + 1] = r[19 * N + 2] - r[19 * N]
            return r, np.asarray(be.to_host(out["trace"]), dtype=float)[:, 0].copy()
        sph_r = None if sph is None else be.from_host(np.ascontiguousarray(sph.astype(np.float32 if suf == "f32" else np.float64)))
        out = self._mppi_op(ops, splits, prm, col(p0, suf), col(v0, suf), col(self.goal_position, suf), col(U0, suf), n_samples, iters, sigma,
                            temperature, seed=seed, iter_base=it_base, spheres=sph_r, obstacle_weight=w_obs)
        res = be.empty((19 * N + 3,), "f64")
        sph_d = None if sph is None else be.from_host(np.ascontiguousarray(sph.astype(np.float64)))
        ops.shooting_finish(prm, out["U"], out["keys"], state, res, spheres=sph_d, obstacle_weight=w_obs)
        return np.asarray(be.to_host(res), dtype=float).copy(), np.asarray(be.to_host(out["trace"]), dtype=float)[:, 0].copy()

    def _plan_mppi_captured(self, ops, prm, p0, v0, U0, n_samples, iters, sigma, temperature, seed, precision, sph, w_obs, it_base, splits=None):
        """plan_mppi as ONE hipGraph replay: state, nominal and iteration counter in through pinned buffers -> ``se3mpc_mppi_*`` (the counter read
        from a device word, so one capture serves every cycle) -> ``se3mpc_shooting_finish_*`` on its key -> packed result and trace out through
        pinned buffers; the host synchronises once.  Same numbers as :meth:`_plan_mppi_eager`.  With `splits` the graph holds the
        ``iters`` + 1 launches of ``se3mpc_mppi_split_*`` in place of the one, and their workspace."""
        import torch
        N = prm.horizon
        K = 0 if sph is None else len(sph)
        key = (N, n_samples, iters, sigma, temperature, seed, precision, bytes(prm), K, w_obs, splits)
        graphs = self.__dict__.setdefault("_mppi_graphs", {})
        g = graphs.get(key)
        if g is None:
            dev = ops.be.device
            dt = torch.float32 if precision == "f32" else torch.float64
            pin = lambda n, t=torch.float64: torch.zeros(n, dtype=t).pin_memory()
            io = dict(h_in=pin(9 + 3 * N), d_in=torch.zeros(9 + 3 * N, dtype=torch.float64, device=dev), h_it=pin(1, torch.int32),
                      d_it=torch.zeros(1, dtype=torch.int32, device=dev), h_out=pin(19 * N + 3), h_trace=pin(max(iters, 1), dt),
                      d_U=torch.empty((3 * N, 1), dtype=dt, device=dev), d_cost=torch.empty(1, dtype=dt, device=dev),
                      d_trace=torch.empty((max(iters, 1), 1), dtype=dt, device=dev), d_keys=torch.empty(1, dtype=torch.int64, device=dev),
                      d_s=torch.empty((3, 3, 1), dtype=dt, device=dev), d_U0=torch.empty((3 * N, 1), dtype=dt, device=dev))
            if K:
                io.update(h_sph=pin((K, 4)), d_sph=torch.zeros((K, 4), dtype=torch.float64, device=dev), d_sph_r=torch.empty((K, 4), dtype=dt, device=dev))
            io["d_ws"] = None if splits is None else ops.mppi_split_workspace(prm, 1, splits)
            io["h_in_np"], io["h_it_np"], io["h_out_np"], io["h_trace_np"] = (io[k].numpy() for k in ("h_in", "h_it", "h_out", "h_trace"))
            if K:
                io["h_sph_np"] = io["h_sph"].numpy()

            def body():
                io["d_in"].copy_(io["h_in"], non_blocking=True)
                io["d_it"].copy_(io["h_it"], non_blocking=True)
                io["d_s"].copy_(io["d_in"][:9].view(3, 3, 1))                 # (p0, v0, goal) in the kernel's type
                io["d_U0"].copy_(io["d_in"][9:].view(3 * N, 1))
                if K:
                    io["d_sph"].copy_(io["h_sph"], non_blocking=True)
                    io["d_sph_r"].copy_(io["d_sph"])
                self._mppi_op(ops, splits, prm, io["d_s"][0], io["d_s"][1], io["d_s"][2], io["d_U0"], n_samples, iters, sigma, temperature, seed=seed,
                              iter_base=0, iter_offset=io["d_it"], spheres=io["d_sph_r"] if K else None, obstacle_weight=w_obs,
                              out=(io["d_U"], io["d_cost"], io["d_trace"], io["d_keys"]), workspace=io["d_ws"])
                ops.shooting_finish(prm, io["d_U"], io["d_keys"], io["d_in"], io["h_out"], spheres=io["d_sph"] if K else None, obstacle_weight=w_obs)
                io["h_trace"].copy_(io["d_trace"].view(-1), non_blocking=True)

            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                body()                                                             # warm-up outside the capture
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                body()
            if len(graphs) >= 4:
                graphs.pop(next(iter(graphs)))
            g = graphs[key] = (graph, io)
        graph, io = g
        hin = io["h_in_np"]
        hin[0:3] = p0; hin[3:6] = v0; hin[6:9] = self.goal_position; hin[9:] = U0.reshape(-1)
        io["h_it_np"][0] = np.array(it_base, dtype=np.uint32).view(np.int32)        # the kernel reads the word as uint32
        if K:
            io["h_sph_np"][...] = sph
        graph.replay()
        torch.cuda.current_stream(ops.be.device).synchronize()
        return io["h_out_np"].copy(), io["h_trace_np"][:iters].astype(float)

    def plan_batch_mppi(self, positions, velocities, goals, n_samples: int = MPPI_SAMPLES, iters: int = MPPI_ITERS, sigma: float = MPPI_SIGMA,
                        temperature: float = MPPI_TEMPERATURE, seed: int = 0, precision: Optional[str] = None, obstacles=None,
                        obstacle_weight: Optional[float] = None, nominal=None, iter_base: int = 0, splits=None,
                        timestamp: float = 0.0) -> Dict[str, np.ndarray]:
        """MPPI for B independent (state, goal) problems in ONE launch (problem b draws the noise of index b): positions, velocities, goals (B, 3);
        nominal (B, N, 3) or None = hover.  Returns arrays with a leading B axis: positions, velocities, thrust_vectors, accelerations,
        attitudes, body_rates (B, N, 3), thrusts (B, N), cost (B,) with the penalty, trace (B, iters).  ``splits`` as :meth:`plan_mppi`; "auto"
        also keeps B * splits within 1024 workgroups.  Moving obstacles as :meth:`plan_mppi`: ``timestamp`` is the time all B states hold
        (rebasing the planner's own moving obstacles); with a non-zero velocity the launch is ``se3mpc_mppi_moving_*`` and ``splits`` raises.
        Tracked obstacles (:meth:`add_tracked_obstacle`) are resampled at `timestamp` and shared by all B problems (one slab,
        ``se3mpc_mppi_tracks_*``); ``splits`` raises."""
        p0 = np.asarray(to_float(positions), float).reshape(-1, 3)
        v0 = np.asarray(to_float(velocities), float).reshape(-1, 3)
        g = np.asarray(to_float(goals), float).reshape(-1, 3)
        if not (p0.shape == v0.shape == g.shape):
            raise ValueError("positions, velocities and goals must all be (B, 3)")
        B, N = len(p0), self.se3_config.prediction_horizon
        U = np.tile([0.0, 0.0, self.hover_thrust], (B, N, 1)) if nominal is None else np.asarray(nominal, float).reshape(B, N, 3)
        ops = self._get_ops()
        be = ops.be
        prm = self._params(has_goal=1)
        npdt = np.float32 if (precision or "f32") == "f32" else np.float64
        lane = lambda a: be.from_host(np.ascontiguousarray(np.asarray(a, float).reshape(B, -1).T.astype(npdt)))
        sph, moving = self._mppi_tables(obstacles, timestamp)
        w_obs = float(self.se3_config.obstacle_weight if obstacle_weight is None else obstacle_weight)
        lp0, lv0, lg = lane(p0), lane(v0), lane(g)
        more = {}
        if moving is not None:
            if self._mppi_splits(splits, n_samples, B) is not None:
                raise ValueError("plan_batch_mppi: the split form is not built for moving obstacles: use splits=None")
            more = dict(sphere_vel=be.from_host(np.ascontiguousarray(moving[:, 4:].astype(npdt))), sphere_t0=0.0)
        slab = self._tracked_obstacle_slab(obstacles, timestamp)
        sph_d = None if sph is None else be.from_host(np.ascontiguousarray(sph.astype(npdt)))
        if slab is not None:
            if self._mppi_splits(splits, n_samples, B) is not None:
                raise ValueError("plan_batch_mppi: the split form is not built for tracked obstacles: use splits=None")
            vel = None if sph is None else be.from_host(np.ascontiguousarray(self._moving_obstacle_table(obstacles, timestamp)[:, 4:].astype(npdt)))
            out = ops.mppi_tracks(prm, lp0, lv0, lg, lane(U), n_samples, iters, sigma, temperature, be.from_host(np.ascontiguousarray(slab.astype(npdt))),
                                  seed=seed, iter_base=iter_base, spheres=sph_d, obstacle_weight=w_obs, want_keys=False, sphere_vel=vel, sphere_t0=0.0)
        else:
            out = self._mppi_op(ops, self._mppi_splits(splits, n_samples, B), prm, lp0, lv0, lg, lane(U), n_samples, iters, sigma, temperature, seed=seed,
                                iter_base=iter_base, spheres=sph_d, obstacle_weight=w_obs, want_keys=False, **more)
        _, _, P, V = ops.rollout_cost_grad(prm, lp0, lv0, lg, out["U"], want_grad=False, want_states=True)
        acc, att, rates, thr = ops.extract(prm, out["U"])
        h = lambda a, shape: np.asarray(be.to_host(a), dtype=float).T.reshape(shape).copy()
        return dict(positions=h(P, (B, N, 3)), velocities=h(V, (B, N, 3)), thrust_vectors=h(out["U"], (B, N, 3)), accelerations=h(acc, (B, N, 3)),
                    attitudes=h(att, (B, N, 3)), body_rates=h(rates, (B, N, 3)), thrusts=h(thr, (B, N)), cost=h(out["cost"], (B,)),
                    trace=h(out["trace"], (B, iters)) if iters > 0 else np.zeros((B, 0)))

    def _create_warm_start(self, current_state: DroneState, N: int) -> np.ndarray:
        """planner.py:294-327: shift the previous solution by one step, re-anchor step 0 at the current
        state, extend to the goal with hover thrust."""
        prev = self.last_solution
        P = np.zeros((N, 3)); V = np.zeros((N, 3)); T = np.zeros((N, 3))
        P[0] = to_float(current_state.position)
        V[0] = to_float(current_state.velocity)
        plen = len(prev["positions"]) if prev is not None else 0
        shift = 0
        if prev is not None and plen > 1:
            shift = min(N - 1, plen - 1)
            P[1:shift + 1] = prev["positions"][1:shift + 1]
            V[1:shift + 1] = prev["velocities"][1:shift + 1]
            T[:shift] = prev["thrust_vectors"][1:shift + 1]
        if self.goal_position is not None:
            shift = min(N - 1, plen - 1) if prev is not None else 0
            for i in range(shift + 1, N):
                alpha = (i - shift) / max(N - shift, 1)
                P[i] = (1 - alpha) * P[shift] + alpha * self.goal_position
                T[i] = (0.0, 0.0, self.hover_thrust)
        return np.concatenate([P.ravel(), V.ravel(), T.ravel()])

    def _cold_start(self, p0, v0, goal) -> np.ndarray:
        """planner.py:329-359 on the host (only to seed restarts; the solver has its own)."""
        N, dt = self.se3_config.prediction_horizon, self.se3_config.dt
        P = np.zeros((N, 3)); V = np.zeros((N, 3)); T = np.zeros((N, 3))
        for i in range(N):
            a = i / max(N - 1, 1)
            P[i] = (1 - a) * p0 + a * goal
            if i > 0:
                V[i] = (P[i] - P[i - 1]) / dt
        V[0] = v0
        T[:, 2] = self.hover_thrust
        return np.concatenate([P.ravel(), V.ravel(), T.ravel()])

    def refresh_obstacles_from_grid(self, grid_positions, occupancies, threshold: float = 0.6, target: int = 20,
                                    radius: float = 1.0) -> int:
        """What the cloud loop does between mapper and planner
        (cloud/main_improved_threelayer.py:381-398 ``_refresh_se3_obstacles_from_mapper``): clear the obstacle
        list and refill it with every step-th occupied grid cell as a sphere of fixed radius -- selected on
        the device (``se3mpc_spheres_from_grid_*``).  ``grid_positions`` / ``occupancies`` are the two
        arrays ``ExplicitGeometricMapper.get_local_occupancy_grid`` returns (any shape that flattens to
        (M, 3) / (M,)).  Returns the number of obstacles."""
        import torch
        ops = self._get_ops()
        dev = ops.be.device
        pos = torch.as_tensor(np.ascontiguousarray(np.asarray(to_float(grid_positions), float).reshape(-1, 3))).to(dev)
        occ = torch.as_tensor(np.ascontiguousarray(np.asarray(to_float(occupancies), float).reshape(-1))).to(dev)
        spheres, count = ops.spheres_from_grid(pos, occ, threshold=threshold, target=target, radius=radius,
                                               cap=max(2 * target, 1))
        k = int(count.cpu()[0])
        sp = spheres[:k].cpu().numpy()
        self.clear_obstacles()
        for row in sp:
            self.add_obstacle(row[:3].copy(), float(row[3]))
        return k

    def obstacle_clearance(self, trajectory: Trajectory) -> Dict[str, float]:
        """planner.py:499-514 evaluated on a planned trajectory with the obstacle kernel: the minimum
        of |p_k - c_j|^2 - (r_j + margin)^2 over steps and obstacles (>= 0 means clear) and the summed
        violation.  (The reference builds these constraints and never passes them to the solver.)  Moving obstacles
        (:meth:`add_moving_obstacle`) are evaluated on the host at each row's own timestamp, c + v * (trajectory.timestamps[k] - timestamp),
        with the same residual and the same violation sum_k sum_j max(0, -residual)."""
        import torch
        if self.moving_obstacles:
            P = np.asarray(to_float(trajectory.positions), float).reshape(-1, 3)
            ts = np.asarray(trajectory.timestamps, float).reshape(-1)
            margin = float(self.se3_config.safety_margin)
            res = [np.sum((P - np.asarray(to_float(c), float).reshape(3)) ** 2, axis=1) - (float(r) + margin) ** 2 for c, r in self.obstacles]
            res += [np.sum((P - (c[None] + v[None] * (ts - t)[:, None])) ** 2, axis=1) - (r + margin) ** 2 for c, r, v, t in self.moving_obstacles]
            res = np.stack(res, axis=1)
            return dict(min_residual=float(res.min()), violation=float(np.sum(np.maximum(0.0, -res))))
        if not self.obstacles:
            return dict(min_residual=float("inf"), violation=0.0)
        ops = self._get_ops()
        N = len(trajectory.positions)
        X = torch.zeros(9 * N, 1, dtype=torch.float64, device=ops.be.device)
        X[:3 * N, 0] = torch.from_numpy(np.asarray(trajectory.positions, float).ravel()).to(ops.be.device)
        sph = torch.tensor([[*c, r] for c, r in self.obstacles], dtype=torch.float64, device=ops.be.device)
        _, cmin, viol = ops.obstacle_residual(self._params(horizon=N), X, sph, materialize=False)
        return dict(min_residual=float(cmin[0]), violation=float(viol[0]))

    # ------------------------------------------------------------------ planner.py:329-654: the path's own functions
    # Same names and arguments as the reference's private methods; each is one call into the lane-layout kernel that
    # replaces it (one trajectory = one lane), float64, host arrays in and out.  The solver does not go through these
    # (it has them fused in one launch); they are here for callers and tests that use the reference's method names.
    def _lane1(self, x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(np.asarray(to_float(x), float).reshape(-1, 1))).to(self._get_ops().be.device)

    def _pack_variables(self, positions, velocities, thrust_vectors) -> np.ndarray:              # :361-367
        return np.concatenate([np.asarray(positions).flatten(), np.asarray(velocities).flatten(), np.asarray(thrust_vectors).flatten()])

    def _unpack_variables(self, x, N: int):                                                         # :369-376
        x = np.asarray(x)
        return x[:N * 3].reshape(N, 3), x[N * 3:2 * N * 3].reshape(N, 3), x[2 * N * 3:3 * N * 3].reshape(N, 3)

    def _create_straight_line_initialization(self, current_state: DroneState, N: int) -> np.ndarray:   # :329-359
        ops = self._get_ops()
        goal = self.goal_position if self.goal_position is not None else np.zeros(3)
        X0 = ops.init(self._params(horizon=N), self._lane1(current_state.position), self._lane1(current_state.velocity), self._lane1(goal))
        return ops.be.to_host(X0)[:, 0].astype(float)

    def _initialize_optimization_variables(self, current_state: DroneState, N: int) -> np.ndarray:     # :282-292
        if self.warm_start_enabled and self.last_solution is not None:
            return self._create_warm_start(current_state, N)
        return self._create_straight_line_initialization(current_state, N)

    def _setup_optimization_bounds(self, N: int) -> List[Tuple[float, float]]:                      # :378-402
        c = self.se3_config
        txy = c.max_thrust * np.sin(c.max_tilt_angle)
        return ([(-100.0, 100.0)] * (3 * N) + [(-c.max_velocity, c.max_velocity)] * (3 * N)
                + [(-txy, txy), (-txy, txy), (c.min_thrust, c.max_thrust)] * N)

    def _setup_optimization_constraints(self, current_state: DroneState, N: int) -> List[Dict]:       # :404-424
        cons = [{"type": "eq", "fun": lambda x: self._dynamics_constraints(x, current_state, N)}]
        if self.obstacles:
            cons.append({"type": "ineq", "fun": lambda x: self._obstacle_constraints(x, N)})
        if self.moving_obstacles:                                    # a snapshot at the state's timestamp (the reference has no moving obstacles)
            snap = self._moving_obstacle_table(None, current_state.timestamp)[len(self.obstacles):, :4]
            cons.append({"type": "ineq", "fun": lambda x: self._obstacle_constraints(x, N, snap)})
        return cons

    def _dynamics_constraints(self, x, current_state: DroneState, N: int) -> np.ndarray:             # :426-462
        ops = self._get_ops()
        R = ops.dynamics_residual(self._params(horizon=N), self._lane1(x), self._lane1(current_state.position),
                                  self._lane1(current_state.velocity))
        return ops.be.to_host(R)[:, 0].astype(float)

    def _dynamics_constraints_jacobian(self, x, current_state: DroneState, N: int):                   # :464-470
        return None

    def _physical_constraints(self, x, N: int) -> np.ndarray:                                        # :472-497
        ops = self._get_ops()
        return ops.be.to_host(ops.physical_constraints(self._params(horizon=N), self._lane1(x)))[:, 0].astype(float)

    def _obstacle_constraints(self, x, N: int, table=None) -> np.ndarray:                            # :499-514
        import torch
        if table is None and not self.obstacles:
            return np.array([])
        ops = self._get_ops()
        sph = torch.tensor([[*c, r] for c, r in self.obstacles] if table is None else np.asarray(table, float).tolist(), dtype=torch.float64,
                           device=ops.be.device)
        C, _, _ = ops.obstacle_residual(self._params(horizon=N), self._lane1(x), sph, materialize=True)
        return ops.be.to_host(C)[:, 0].astype(float)

    def _objective_function(self, x) -> float:                                                       # :516-550
        ops = self._get_ops()
        N = self.se3_config.prediction_horizon
        goal = None if self.goal_position is None else self._lane1(self.goal_position)
        f, _ = ops.cost_grad(self._params(horizon=N), self._lane1(x), goal, want_grad=False)
        return float(ops.be.to_host(f)[0])

    def _objective_gradient(self, x) -> np.ndarray:                                                  # :552-580
        ops = self._get_ops()
        N = self.se3_config.prediction_horizon
        goal = None if self.goal_position is None else self._lane1(self.goal_position)
        _, g = ops.cost_grad(self._params(horizon=N), self._lane1(x), goal)
        return ops.be.to_host(g)[:, 0].astype(float)

    def _compute_attitudes_and_rates(self, thrust_vectors, velocities=None):                          # :604-654
        ops = self._get_ops()
        T = np.asarray(to_float(thrust_vectors), float)
        N = len(T)
        _, att, rates, _ = ops.extract(self._params(horizon=N), self._lane1(T))
        return ops.be.to_host(att)[:, 0].reshape(N, 3).astype(float), ops.be.to_host(rates)[:, 0].reshape(N, 3).astype(float)

    def _extract_solution_from_result(self, x, N: int) -> Dict[str, np.ndarray]:                     # :582-602
        ops = self._get_ops()
        P, V, T = self._unpack_variables(np.asarray(x, float), N)
        acc, att, rates, thr = ops.extract(self._params(horizon=N), self._lane1(T))
        h = lambda a, shape: ops.be.to_host(a)[:, 0].reshape(shape).astype(float)
        return {"positions": P, "velocities": V, "thrust_vectors": T, "accelerations": h(acc, (N, 3)), "attitudes": h(att, (N, 3)),
                "body_rates": h(rates, (N, 3)), "thrusts": h(thr, (N,))}

    # ------------------------------------------------------------------ planner.py:656-757
    def _create_trajectory_from_solution(self, solution: Dict[str, np.ndarray], start_time: float) -> Trajectory:
        N = len(solution["positions"])
        key = (N, self.se3_config.dt)
        if getattr(self, "_stamp_key", None) != key:                            # k * dt of the horizon, formed once per (N, dt)
            self._stamp_key, self._stamp_offsets = key, np.arange(N) * self.se3_config.dt
        timestamps = start_time + self._stamp_offsets
        return Trajectory(timestamps=timestamps, positions=solution["positions"], velocities=solution["velocities"],
                          accelerations=solution["accelerations"], attitudes=solution["attitudes"],
                          body_rates=solution["body_rates"], thrusts=solution["thrusts"],
                          yaws=solution["attitudes"][:, 2], yaw_rates=solution["body_rates"][:, 2])

    def _generate_emergency_trajectory(self, current_state: DroneState) -> Trajectory:
        self.logger.warning("Generating emergency hover trajectory")
        N, dt = self.se3_config.prediction_horizon, self.se3_config.dt
        return Trajectory(timestamps=current_state.timestamp + np.arange(N) * dt,
                          positions=np.tile(np.asarray(to_float(current_state.position), float), (N, 1)),
                          velocities=np.zeros((N, 3)), accelerations=np.zeros((N, 3)))

    def get_planning_stats(self) -> Dict[str, Any]:
        if not self.planning_times:
            return {}
        return {"mean_planning_time_ms": float(np.mean(self.planning_times)),
                "max_planning_time_ms": float(np.max(self.planning_times)),
                "success_rate": float(np.mean(self.convergence_history)) if self.convergence_history else 0.0,
                "total_plans": self.plan_count}

    def reset_performance_tracking(self) -> None:
        self.planning_times.clear()
        self.convergence_history.clear()
        self.plan_count = 0

    def is_plan_valid(self, trajectory: Trajectory) -> bool:
        if trajectory is None or len(trajectory.positions) == 0:
            return False
        P = np.asarray(trajectory.positions, float)
        if np.any(np.isnan(P)) or np.any(np.isinf(P)) or np.any(P[:, 2] < 0.1):
            return False
        if trajectory.velocities is not None and np.any(np.abs(np.asarray(trajectory.velocities, float)) > 20.0):
            return False
        return True

    def update_plan(self, current_state: DroneState, obstacles: List[Dict[str, Any]]) -> Trajectory:
        self.clear_obstacles()
        for ob in obstacles:
            if "position" in ob and "radius" in ob:
                self.add_obstacle(np.array(ob["position"], float), ob["radius"])
        if self.goal_position is not None:
            return self.plan_trajectory(current_state, self.goal_position)
        return self._generate_emergency_trajectory(current_state)

    def get_config(self) -> SE3MPCConfig:
        return self.se3_config


PlannerFactory.register("se3_mpc", SE3MPCPlanner)      # planner.py:761-762
