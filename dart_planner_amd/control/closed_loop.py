"""Batched closed loop on the device: planner -> (plan sample -> geometric controller -> simulator) for many drones at once.

What the reference's closed-loop tests do one drone and one Python call at a time
(tests/test_planner_controller_contract.py:115-162, :255-316; tests/test_monte_carlo_sim.py:24-72) runs here as two launches
per planning cycle for B drones: ``se3mpc_solve_*`` (every drone re-plans from its own state) and ``se3mpc_closed_loop_*``
(``substeps`` control + simulator steps against the fresh plan, which is read in place from the solver's outputs).  No host
arithmetic, no copies between the two; the only host work per cycle is the N plan stamps (planner.py:661: start + arange(N)*dt).
``run_mppi`` / ``run_mppi_fused`` close the same loop with MPPI as the planner (``se3mpc_mppi_closed_loop_*``: plan, control and simulate
inside one kernel, the plan handed over in LDS).  ``run(..., smoother=SmootherParams)`` / ``run_mppi(..., smoother=...)`` put the reference's
TrajectorySmoother between plan and controller, as its edge loop does (edge/main_improved.py:96-152): plan -> ``se3mpc_smoother_update_*`` ->
``se3mpc_closed_loop_smoothed_*`` per cycle.  ``mixer=MixerParams`` (with or without the
smoother) puts the reference's MotorMixer and motor model behind the controller: the act phase becomes ``se3mpc_closed_loop_actuated_*`` and the
simulator flies under what the motors deliver, ``motor_health`` scaling each motor's thrust.  ``run_fused_staged`` flies both
stages inside the one-launch solver-based Monte-Carlo (``se3mpc_monte_carlo_staged_*``), ``run_mppi_fused_staged`` inside the
one-launch MPPI Monte-Carlo, where the clearance to the spheres is measured too (``se3mpc_mppi_closed_loop_staged_*``);
``run_fused``, ``run_mppi_fused`` and ``capture`` do not have them.  ``run_edge`` flies the reference's OTHER edge loop (edge/main.py:21-112) under the
same planner: a latency buffer between the drone's state and its controller, and the cascaded-PID OnboardController in place of the geometric one
(``se3mpc_edge_loop_*``); ``run_edge_fused`` flies it inside one launch (``se3mpc_monte_carlo_edge_*``).
``run_mppi_edge`` / ``run_mppi_edge_fused`` fly that edge loop under the MPPI planner, as a chain and in one launch
(``se3mpc_mppi_closed_loop_edge_*``): the one form where the delay and the obstacle clearance meet.
``run_mission`` / ``run_mission_fused`` fly waypoint missions: the goal of every cycle comes from the reference's
GlobalMissionPlanner.get_current_goal on the drone's own position (``se3mpc_mission_goal_*``, ``se3mpc_monte_carlo_mission_*``)
where every other method holds one goal for the whole run.
"""
import functools
import math
from typing import Optional

from ..capi import ControllerParams, MixerParams, OnboardParams, Params, SimulatorParams, SmootherParams


class ClosedLoopMonteCarlo:
    """Receding-horizon Monte-Carlo over B drones (BASELINE.json config 5's named test shape).

    ops: dart_planner_amd.ops.Ops;  params: se3mpc_params of the planner (horizon N, dt);  controller / simulator: the
    C-ABI parameter structs (defaults: the reference's "sitl_optimized" controller and DroneSimulator())."""

    def __init__(self, ops, params: Params, controller: Optional[ControllerParams] = None, simulator: Optional[SimulatorParams] = None):
        self.ops, self.params = ops, params
        self.controller = controller if controller is not None else ops.lib.controller_default_params()
        self.simulator = simulator if simulator is not None else ops.lib.simulator_default_params()

    @staticmethod
    def _no_smoother(smoother, what: str) -> None:
        if smoother is not None:
            raise ValueError(f"{what} has no trajectory smoother (the one-launch kernels keep one plan per drone on the chip, DESIGN.md 5.7c): "
                             "use run / run_mppi with smoother=")

    @staticmethod
    def _no_mixer(mixer, motor_health, what: str) -> None:
        if mixer is not None or motor_health is not None:
            raise ValueError(f"{what} has no motor mixer (the one-launch kernels hand the simulator the commanded wrench, DESIGN.md 5.7d): "
                             "use run / run_mppi with mixer=")

    @staticmethod
    def _no_moving(sphere_velocities, what: str) -> None:
        if sphere_velocities is not None:
            raise ValueError(f"{what}: moving spheres are not built for this form (DESIGN.md 5.8f): use run_mppi or run_mppi_fused")

    @staticmethod
    def _mixer_option(mixer, motor_health) -> None:
        if motor_health is not None and mixer is None:
            raise ValueError("motor_health scales what the mixer's motors deliver: it needs mixer=")

    def _start(self, p0, v0, smoother=None):
        """Every method's start: -> st (fresh controller records), sm (fresh smoother records, None without a smoother) and the drones'
        flight state fl = (time, pos, vel, att, omega): zero clocks, clones of p0 / v0, zero attitudes and body rates."""
        import torch
        ops = self.ops
        B = p0.shape[0]
        pos, vel = p0.clone(), v0.clone()
        att, om = torch.zeros_like(p0), torch.zeros_like(p0)
        time = torch.zeros(B, dtype=torch.float64, device=ops.be.device)
        st = ops.controller_state(self.controller, B)
        return st, (ops.smoother_state(B) if smoother is not None else None), (time, pos, vel, att, om)

    def _actor(self, smoother, st, sm, fl, strides, substeps: int, sim_dt: float, wind, mixer=None, mx=None, motor_health=None):
        """-> act(plan, log): `substeps` control + simulator steps of every drone against plan = (stamps, P, V, A) with `strides`, as one
        ``se3mpc_closed_loop_*`` launch -- or, with a smoother, update_trajectory against the plan of the call before (None at first; the
        caller keeps that plan's tensors alive and unchanged until then) and one ``se3mpc_closed_loop_smoothed_*`` launch.  With a mixer
        (records mx) the launch is ``se3mpc_closed_loop_actuated_*`` in either case."""
        ops, old = self.ops, [None]

        def act(plan, log: bool = False):
            if smoother is not None:
                ops.smoother_update(smoother, sm, fl[0], *plan, strides=strides, old=old[0], old_strides=strides)   # the wall clock of update_trajectory = the drones' clocks
                old[0] = plan
            if mixer is not None:
                return ops.closed_loop_actuated(mixer, self.controller, self.simulator, st, mx, *fl, *plan, nsteps=substeps, sim_dt=sim_dt, strides=strides,
                                                smoother=smoother, smoother_state=sm, motor_health=motor_health, wind=wind, log=log)
            if smoother is None:
                return ops.closed_loop(self.controller, self.simulator, st, *fl, *plan, nsteps=substeps, sim_dt=sim_dt, strides=strides, wind=wind,
                                       stop_at_plan_end=False, log=log)
            return ops.closed_loop_smoothed(smoother, self.controller, self.simulator, st, sm, *fl, *plan, nsteps=substeps, sim_dt=sim_dt,
                                            strides=strides, wind=wind, log=log)
        return act

    @staticmethod
    def _result(st, sm, fl, **more):
        time, pos, vel, att, om = fl
        mx = more.pop("mixer_state", None)
        res = dict(pos=pos, vel=vel, att=att, omega=om, time=time, controller_state=st, **more)
        if sm is not None:
            res["smoother_state"] = sm
        if mx is not None:
            res["mixer_state"] = mx
        return res

    def run(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, wind=None, log: bool = False,
            smoother: Optional[SmootherParams] = None, mixer: Optional[MixerParams] = None, motor_health=None):
        """p0, v0, goal: (B, 3) device tensors (float32 or float64: the precision of the whole loop); wind: None, (3,) or (B, 3) newtons.
        smoother: None, or the parameters of the reference's TrajectorySmoother: every fresh plan then goes through update_trajectory
        (against the previous cycle's plan, so the plan tensors alternate between two sets) and every control step takes its target from
        get_desired_state.  mixer: None, or the parameters of the reference's MotorMixer and motor model: the controller's command goes
        through mix_commands and the simulator runs under the wrench the motors deliver; motor_health: None, (4,) or (B, 4) factors on
        each motor's thrust (needs `mixer`).  -> dict(pos, vel, att, omega (B, 3), time (B,), controller_state (B, 12), logs = [(solve
        outputs, closed-loop outputs)] if log[, smoother_state (B, 25)][, mixer_state (B, 5)])."""
        import torch
        ops, prm = self.ops, self.params
        N = prm.horizon
        self._mixer_option(mixer, motor_health)
        st, sm, fl = self._start(p0, v0, smoother)
        mx = ops.mixer_state(p0.shape[0]) if mixer is not None else None
        act = self._actor(smoother, st, sm, fl, (9 * N, 9 * N, 3 * N), substeps, sim_dt, wind, mixer, mx, motor_health)
        k = torch.arange(N, dtype=torch.float64, device=ops.be.device)
        logs = []
        # without logs every cycle writes the same plan tensors again (the closed-loop launch of a cycle is ordered before the next solve); a
        # smoother still reads the previous cycle's plan, so two sets alternate
        sols = [None] if smoother is None else [None, None]
        for c in range(cycles):
            slot = c % len(sols)
            sol = sols[slot] = ops.solve(prm, fl[1], fl[2], goal, want_trajectory=True if log else "accelerations", out=None if log else sols[slot])
            X = sol["x"]
            out = act(((c * substeps * sim_dt) + k * prm.dt, X, X[:, 3 * N:], sol["accelerations"]), log)
            if log:
                logs.append((sol, out))
        return self._result(st, sm, fl, logs=logs, mixer_state=mx)

    def run_edge(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, latency_depth: int = 5, onboard: Optional[OnboardParams] = None,
                 wind=None, log: bool = False):
        """The receding-horizon Monte-Carlo on the reference's edge loop (edge/main.py:80-95): per cycle one solve launch, as :meth:`run`,
        then ONE ``se3mpc_edge_loop_*`` launch of `substeps` x (latency push -> OnboardController.compute_control_command -> DroneSimulator.step)
        that reads the plan in place.  latency_depth: slots of the estimator -> controller buffer (5 = hardware.yaml's 25 ms at 5 ms; 0 = no
        buffer); onboard: the controller's parameters (None: OnboardController()).  The first popped state is older than the controller's
        clock, so with a buffer every drone gets one zero command (thrust 0, torque 0) at step `latency_depth` of the first cycle.
        -> dict(pos, vel, att, omega (B, 3), time (B,), onboard_state (B, 14), latency = the buffer (Ops.latency_buffer), zero_thrust_steps
        int32 (B,) = the steps whose commanded thrust was exactly 0, logs = [(solve outputs, edge-loop outputs)] if log).
        :meth:`run_edge_fused` is the same run in one launch (``se3mpc_monte_carlo_edge_*``; measured at 0.74 - 0.79 of this chain's time for 4096 drones, 0.87 for 64: DESIGN.md 5.7g)."""
        import torch
        ops, prm = self.ops, self.params
        B, N = p0.shape[0], prm.horizon
        op = onboard if onboard is not None else ops.lib.onboard_default_params()
        _, _, fl = self._start(p0, v0)
        st = ops.onboard_state(B)
        buf = ops.latency_buffer(B, latency_depth, ops.be.suffix(p0))
        zeros = torch.zeros(B, dtype=torch.int32, device=ops.be.device)
        k = torch.arange(N, dtype=torch.float64, device=ops.be.device)
        logs, sol = [], None
        for c in range(cycles):
            sol = ops.solve(prm, fl[1], fl[2], goal, want_trajectory=True if log else "accelerations", out=None if log else sol)
            X = sol["x"]
            out = ops.edge_loop(op, self.simulator, st, buf, *fl, (c * substeps * sim_dt) + k * prm.dt, X, X[:, 3 * N:], sol["accelerations"], nsteps=substeps,
                                sim_dt=sim_dt, strides=(9 * N, 9 * N, 3 * N), wind=wind, log=log, zero_thrust_steps=zeros)
            if log:
                logs.append((sol, out))
        time, pos, vel, att, om = fl
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, onboard_state=st, latency=buf, zero_thrust_steps=zeros, logs=logs)

    def run_edge_fused(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, latency_depth: int = 5,
                       onboard: Optional[OnboardParams] = None, wind=None, want_last_plan: bool = False):
        """:meth:`run_edge` in ONE launch (``se3mpc_monte_carlo_edge_*``): every cycle's solve and its `substeps` x (latency push ->
        OnboardController -> DroneSimulator.step) inside one kernel, where :meth:`run_edge` makes two launches per cycle.  Same code, same bits
        and the same result keys as :meth:`run_edge` (no logs), plus last_plan as :meth:`run_fused`.  All cross-cycle state is in the returned
        operands (onboard_state, latency, time), so ``Ops.monte_carlo_edge`` with ``first_cycle=cycles`` continues the run.  If a solve needed
        more L-BFGS memory than the launch's LDS image holds (never with the reference's options) the run is repeated by :meth:`run_edge`.

        Measured on an MI355X (``profiles/monte_carlo_edge.json``; 4096 drones, 33 cycles x 15 steps, horizon 6): 1.49 ms
        (float32) / 1.58 ms (float64) without a buffer and 1.76 / 1.93 ms at depth 5, against 1.97 / 2.13 and 2.24 / 2.49 ms for the 66 launches of
        :meth:`run_edge` -- 0.74 - 0.79 of the chain's time; at 64 drones, depth 5, 1.73 / 1.87 against 1.97 / 2.15 ms (0.87 - 0.88).  The launch is bound
        by one drone's dependent chain (64 drones take as long as 4096), the chain by its launches and by the wait for the slowest solve.  Use this form
        at both batch sizes; beyond 8192 drones at horizon 6 the launch's wavefronts no longer all run at once and neither form is measured there;
        :meth:`run_edge` stays the form with per-step logs."""
        import torch
        ops = self.ops
        B = p0.shape[0]
        op = onboard if onboard is not None else ops.lib.onboard_default_params()
        # the flight state of _start, without the geometric controller's records: this loop has none
        fl = (torch.zeros(B, dtype=torch.float64, device=ops.be.device), p0.clone(), v0.clone(), torch.zeros_like(p0), torch.zeros_like(p0))
        st = ops.onboard_state(B)
        buf = ops.latency_buffer(B, latency_depth, ops.be.suffix(p0))
        zeros = torch.zeros(B, dtype=torch.int32, device=ops.be.device)
        out = ops.monte_carlo_edge(self.params, op, self.simulator, st, buf, *fl, goal, cycles, substeps, sim_dt, wind=wind, zero_thrust_steps=zeros,
                                   want_last_plan=want_last_plan)
        if int(ops.be.to_host(out["overflowed"])[0]) != 0:
            return self.run_edge(p0, v0, goal, cycles, substeps, sim_dt, latency_depth=latency_depth, onboard=onboard, wind=wind)
        time, pos, vel, att, om = fl
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, onboard_state=st, latency=buf, zero_thrust_steps=zeros, logs=[],
                    last_plan=out if want_last_plan else None)

    def run_fused(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, wind=None, want_last_plan: bool = False, smoother=None,
                  mixer=None, motor_health=None):
        """The same Monte-Carlo in ONE launch (``se3mpc_monte_carlo_*``: every cycle's solve and control / simulator steps inside one kernel,
        each drone paying only for its own slow solves instead of waiting, 2 x `cycles` times, at a kernel boundary for the slowest drone of
        the batch).  Same code, same bits as :meth:`run`.  One host synchronise at the end reads the overflow counter; if a solve needed more
        L-BFGS memory than the launch's LDS image holds (never with the reference's options) the run is repeated by :meth:`run`."""
        self._no_smoother(smoother, "run_fused")
        self._no_mixer(mixer, motor_health, "run_fused")
        ops = self.ops
        st, sm, fl = self._start(p0, v0)
        out = ops.monte_carlo(self.params, self.controller, self.simulator, st, *fl, goal, cycles, substeps, sim_dt, wind=wind,
                              want_last_plan=want_last_plan)
        if int(ops.be.to_host(out["overflowed"])[0]) != 0:
            return self.run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind)
        return self._result(st, sm, fl, logs=[], last_plan=out if want_last_plan else None)

    _MISSION_UNBUILT = ("smoother", "mixer", "motor_health", "latency_depth", "onboard", "swarm_size", "neighbours", "mate_radius", "sphere_velocities")

    @classmethod
    def _no_mission_form(cls, options: dict, what: str) -> None:
        bad = sorted(k for k in options if k in cls._MISSION_UNBUILT and options[k] is not None)
        if bad:
            raise ValueError(f"{what}: missions are not built under the smoother, mixer, edge, swarm or moving-sphere forms ({', '.join(bad)}; "
                             "DESIGN.md 5.10): fly them with planner='solve' or planner='mppi' alone")

    @staticmethod
    def _mission_field(field):
        """field: None, the mirror's UncertaintyField or a capi.UFieldDesc -> (descriptor or None, the resolution the stamps are made for)."""
        if field is None:
            return None, 1.0
        desc = getattr(field, "_desc", field)
        return desc, float(desc.resolution)

    def _mission_result(self, st, fl, ms, goal, **more):
        """The result of a mission run: :meth:`run`'s keys, the mission records, the last goal, and phase / waypoint_index as int32 copies of
        the records' first two words."""
        import torch
        return self._result(st, None, fl, mission_state=ms, goal=goal, phase=ms[:, 0].to(torch.int32), waypoint_index=ms[:, 1].to(torch.int32), **more)

    def run_mission(self, p0, v0, waypoints, labels, cycles: int, substeps: int, sim_dt: float, mission=None, planner: str = "solve",
                    epoch: float = 1000.0, field=None, wind=None, log: bool = False, n_samples: int = 0, iters: int = 0, sigma: float = 0.0,
                    temperature: float = 1.0, seed: int = 0, spheres=None, obstacle_weight: float = 0.0, shift: Optional[int] = None, nominal=None,
                    **unbuilt):
        """The receding-horizon Monte-Carlo flying waypoint missions: before every plan the goal comes from the reference's
        GlobalMissionPlanner.get_current_goal on the drone's own position (``se3mpc_mission_goal_*``), where every other form holds one goal
        for the whole run.  waypoints: float64 (W, 3) shared by all drones or (B, W, 3); labels: int32 (W,) or (B, W), 0 = any label, 1 =
        "obstacle", 2 = "landing_pad", 3 = "doorway"; mission: capi.MissionParams (None: the reference's literals).  Per cycle, in order:
        one mission-goal launch with now = the drones' clocks + `epoch` (the default exceeds the replan period, so the first call makes a
        global plan, as against a real wall clock); with `field` (the mirror's UncertaintyField, or a capi.UFieldDesc) one
        ``se3mpc_ufield_stamp`` launch over the B rows the global plans stamped -- the drones share one scene, row order = B sequential calls;
        then the cycle of :meth:`run` (planner="solve") or of :meth:`run_mppi` (planner="mppi", with its arguments; the clearance continues in
        place from call to call).  No host round trip: the goal is a device tensor from launch to launch.
        -> what :meth:`run` / :meth:`run_mppi` returns, plus mission_state (B, 4), goal (B, 3) = the last cycle's, phase and waypoint_index
        int32 (B,); with `log` also goals (cycles, B, 3) and phases int32 (cycles, B), each cycle's after its mission call."""
        import torch
        self._no_mission_form(unbuilt, "run_mission")
        if set(unbuilt) - set(self._MISSION_UNBUILT):
            raise TypeError(f"run_mission: unexpected arguments {sorted(set(unbuilt) - set(self._MISSION_UNBUILT))}")
        if planner not in ("solve", "mppi"):
            raise ValueError(f"run_mission: planner {planner!r} (\"solve\" or \"mppi\")")
        ops, prm = self.ops, self.params
        B, N = p0.shape[0], prm.horizon
        mp = mission if mission is not None else ops.lib.mission_default_params()
        desc, resolution = self._mission_field(field)
        st, _, fl = self._start(p0, v0)
        ms = ops.mission_state(B)
        goal, stamps = torch.zeros_like(p0), ops.mission_stamps(B)
        goals, phases, logs, traces, out, clr, sols = [], [], [], [], None, None, [None]
        if planner == "solve":
            act = self._actor(None, st, None, fl, (9 * N, 9 * N, 3 * N), substeps, sim_dt, wind)
            k = torch.arange(N, dtype=torch.float64, device=ops.be.device)
        else:
            U = self._mppi_start(p0, nominal)
            sh = self.resolve_shift(substeps, sim_dt, shift)
        for c in range(cycles):
            ops.mission_goal(mp, ms, fl[0] + epoch, fl[1], waypoints, labels, resolution, goal=goal, stamps=stamps)
            if desc is not None:
                ops.ufield_stamp(desc, stamps["centres"], stamps["radius"], stamps["radius_voxels"], stamps["factor"])
            if log:
                goals.append(goal.clone())
                phases.append(ms[:, 0].to(torch.int32))
            if planner == "solve":
                sol = sols[0] = ops.solve(prm, fl[1], fl[2], goal, want_trajectory=True if log else "accelerations", out=None if log else sols[0])
                X = sol["x"]
                flown = act(((c * substeps * sim_dt) + k * prm.dt, X, X[:, 3 * N:], sol["accelerations"]), log)
                if log:
                    logs.append((sol, flown))
            else:
                out = ops.mppi_closed_loop(prm, self.controller, self.simulator, st, *fl, goal, U, 1, substeps, sim_dt, n_samples, iters, sigma, temperature,
                                           seed=seed, cycle_base=c, shift=sh, spheres=spheres, obstacle_weight=obstacle_weight, wind=wind, want_plan=log,
                                           clearance=clr)
                clr = out["clearance"]
                traces.append(out["trace"])
                if log:
                    logs.append(dict(plan_last=out["plan_last"], trace=out["trace"], cost=out["cost"]))
        more = dict(logs=logs)
        if planner == "mppi":
            trace = torch.cat(traces, dim=1) if traces else torch.zeros(B, 0, max(int(iters), 0), dtype=p0.dtype, device=ops.be.device)
            more.update(U=U, cost=None if out is None else out["cost"], trace=trace, clearance=clr)
        if log:
            more.update(goals=torch.stack(goals) if goals else torch.zeros(0, B, 3, dtype=p0.dtype, device=ops.be.device),
                        phases=torch.stack(phases) if phases else torch.zeros(0, B, dtype=torch.int32, device=ops.be.device))
        return self._mission_result(st, fl, ms, goal, **more)

    def run_mission_fused(self, p0, v0, waypoints, labels, cycles: int, substeps: int, sim_dt: float, mission=None, epoch: float = 1000.0,
                          field=None, wind=None, want_last_plan: bool = False, first_cycle: int = 0, resume=None, **unbuilt):
        """:meth:`run_mission` with planner="solve" in ONE launch (``se3mpc_monte_carlo_mission_*``): every cycle's mission call,
        solve and control / simulator steps inside one kernel, where :meth:`run_mission` makes three launches per cycle.  Same code, same bits
        and the same result keys as :meth:`run_mission` (no logs), plus last_plan as :meth:`run_fused`.  The stamps cannot be applied inside
        the launch -- they are ordered writes to a grid all drones share, and the phase machine never reads it: with `field` the kernel logs
        them and ONE ``se3mpc_ufield_stamp`` call of cycles x B rows applies them afterwards, in the chain's order (cycle-major, drone-minor),
        so the grids come out with the chain's bytes.  All cross-cycle state is in the returned operands: ``resume=`` a result of this method
        with ``first_cycle=`` the cycles it flew continues that run (p0, v0 are then not read).  If a solve needed more L-BFGS memory than
        the launch's LDS image holds (never with the reference's options) the run is repeated by :meth:`run_mission`.

        Measured on an MI355X: DESIGN.md 5.10 (``tools/gpu_probe_mission.py``, ``profiles/mission.json``)."""
        self._no_mission_form(unbuilt, "run_mission_fused")
        if set(unbuilt) - set(self._MISSION_UNBUILT):
            raise TypeError(f"run_mission_fused: unexpected arguments {sorted(set(unbuilt) - set(self._MISSION_UNBUILT))}")
        ops = self.ops
        mp = mission if mission is not None else ops.lib.mission_default_params()
        desc, resolution = self._mission_field(field)
        if resume is None:
            st, _, fl = self._start(p0, v0)
            ms, goal = ops.mission_state(p0.shape[0]), None
        else:
            st, ms, goal = resume["controller_state"], resume["mission_state"], resume["goal"]
            fl = tuple(resume[k] for k in ("time", "pos", "vel", "att", "omega"))
        out = ops.monte_carlo_mission(self.params, self.controller, self.simulator, mp, st, ms, *fl, waypoints, labels, cycles, substeps, sim_dt,
                                      epoch=epoch, resolution=resolution, wind=wind, first_cycle=first_cycle, goal=goal, want_stamps=desc is not None,
                                      want_last_plan=want_last_plan)
        if int(ops.be.to_host(out["overflowed"])[0]) != 0:
            if resume is not None:
                raise RuntimeError("run_mission_fused: a solve overflowed the launch's LDS image in a resumed run; fly the whole run with run_mission")
            return self.run_mission(p0, v0, waypoints, labels, cycles, substeps, sim_dt, mission=mission, epoch=epoch, field=field, wind=wind)
        if desc is not None and cycles > 0:
            s = out["stamps"]
            ops.ufield_stamp(desc, s["centres"], s["radius"], s["radius_voxels"], s["factor"])
        return self._mission_result(st, fl, ms, out["goal"], logs=[], last_plan=out if want_last_plan else None)

    def run_fused_staged(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, wind=None, want_last_plan: bool = False,
                         smoother: Optional[SmootherParams] = None, mixer: Optional[MixerParams] = None, motor_health=None):
        """:meth:`run` with `smoother` and / or `mixer` (and `motor_health`) in ONE launch (``se3mpc_monte_carlo_staged_*``): every cycle's
        solve, update_trajectory and control / mixer / simulator steps inside one kernel, where :meth:`run` makes three launches per cycle.
        Same code, same bits and the same result keys as :meth:`run` (no logs), plus last_plan as :meth:`run_fused`; without both stages it
        is :meth:`run_fused`.  The kernel keeps ONE plan per drone on the chip: update_trajectory reads the plan being followed only at the
        drone's clock, so that one sample is taken before the next solve overwrites the plan -- which is also why a run
        cannot be continued by a second call.  If a solve needed more L-BFGS memory than the launch's LDS image holds (never with the
        reference's options) the run is repeated by :meth:`run`.

        Measured on an MI355X (``profiles/monte_carlo_staged.json``; 4096 drones, 33 cycles x 15 steps, horizon 6, both stages):
        4.16 ms (float32) / 5.40 ms (float64) against 3.90 / 4.72 ms for the 99 launches of :meth:`run` -- at this shape the one launch is 7 - 15 %
        SLOWER (one lane per drone flies the act phase, which the two stages make the larger part of a cycle; the chain's act kernel flies 64
        drones per wavefront).  For thousands of drones with the stages drive :meth:`run`; use this form for small batches, where the chain is
        launch-bound, or where one enqueue is what you need."""
        self._mixer_option(mixer, motor_health)
        ops = self.ops
        st, sm, fl = self._start(p0, v0, smoother)
        mx = ops.mixer_state(p0.shape[0]) if mixer is not None else None
        out = ops.monte_carlo_staged(self.params, self.controller, self.simulator, st, *fl, goal, cycles, substeps, sim_dt, wind=wind,
                                     want_last_plan=want_last_plan, smoother=smoother, smoother_state=sm, mixer=mixer, mixer_state=mx,
                                     motor_health=motor_health)
        if int(ops.be.to_host(out["overflowed"])[0]) != 0:
            return self.run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind, smoother=smoother, mixer=mixer, motor_health=motor_health)
        return self._result(st, sm, fl, logs=[], last_plan=out if want_last_plan else None, mixer_state=mx)

    def resolve_shift(self, substeps: int, sim_dt: float, shift: Optional[int] = None) -> int:
        """Rows the MPPI nominal moves forward per planning cycle.  None: the plan steps one act phase covers, rounded half up,
        ``floor(substeps * sim_dt / params.dt + 0.5)`` clipped to [0, N]."""
        N = self.params.horizon
        if shift is None:
            shift = int(math.floor(substeps * sim_dt / self.params.dt + 0.5))
        return max(0, min(N, int(shift)))

    def _mppi_start(self, p0, nominal):
        """The MPPI nominal the run starts from: a clone of `nominal`, or hover."""
        import torch
        if nominal is not None:
            return nominal.clone()
        prm = self.params
        U = torch.zeros(p0.shape[0], prm.horizon, 3, dtype=p0.dtype, device=self.ops.be.device)
        U[:, :, 2] = prm.mass * prm.gravity
        return U

    def run_mppi(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float, temperature: float,
                 seed: int = 0, spheres=None, obstacle_weight: float = 0.0, wind=None, shift: Optional[int] = None, nominal=None,
                 log: bool = False, smoother: Optional[SmootherParams] = None, mixer: Optional[MixerParams] = None, motor_health=None,
                 sphere_velocities=None, sphere_t0: float = 0.0):
        """The receding-horizon Monte-Carlo with MPPI as the planner (``se3mpc_mppi_closed_loop_*``), one call per planning cycle: each
        cycle runs `iters` MPPI iterations of `n_samples` samples from the drone's own state on its nominal thrust sequence (hover, or
        `nominal` (B, N, 3)), hands the plan to the controller on the chip, takes `substeps` control + simulator steps and moves the
        nominal forward by `shift` rows.  spheres: (K, 4) rows (cx, cy, cz, r) for the planner's penalty (`obstacle_weight`) and for the
        clearance output.  shift=None resolves to ``floor(substeps * sim_dt / params.dt + 0.5)`` clipped to [0, N]: the plan steps one act
        phase covers, rounded half up.
        -> what :meth:`run` returns, plus U (B, N, 3) = the next cycle's nominal, cost (B,) at the last cycle's nominal, trace
        (B, cycles, iters) = the minimum sample cost per iteration, clearance (B,) = min over every simulator step and sphere of
        |pos - c| - r (None without spheres); logs = [dict(plan_last, trace, cost)] per cycle if `log`.
        smoother: None, or the parameters of the reference's TrajectorySmoother: each cycle is then the planner alone
        (``se3mpc_mppi_closed_loop_*`` with no simulator steps), update_trajectory against the previous cycle's plan and `substeps` steps of
        ``se3mpc_closed_loop_smoothed_*``; clearance is None (only the fused act phase measures it), smoother_state (B, 25) is added.
        mixer, motor_health: as in :meth:`run`; the act phase is then ``se3mpc_closed_loop_actuated_*`` on the handed-over plan, with or
        without the smoother (clearance None likewise), and mixer_state (B, 5) is added.
        sphere_velocities: None, or (K, 3) rows (vx, vy, vz): the spheres move with constant velocity from the centres the table holds
        `sphere_t0` seconds before the run starts (``se3mpc_mppi_closed_loop_moving_*``): every plan step is penalised and
        every simulator step's clearance measured against the centres at that step's time.  With a smoother or a mixer the planner-only
        call gets the velocities and the time of its cycle's start; clearance stays None."""
        import torch
        ops, prm = self.ops, self.params
        B, N = p0.shape[0], prm.horizon
        self._mixer_option(mixer, motor_health)
        smoothed = smoother is not None or mixer is not None        # the act phase is a launch of its own
        st, sm, fl = self._start(p0, v0, smoother)
        mx = ops.mixer_state(B) if mixer is not None else None
        U = self._mppi_start(p0, nominal)
        sh = self.resolve_shift(substeps, sim_dt, shift)
        act = self._actor(smoother, st, sm, fl, (9 * N, 9 * N, 9 * N), substeps, sim_dt, wind, mixer, mx, motor_health)
        k = torch.arange(N, dtype=torch.float64, device=ops.be.device) if smoothed else None
        logs, traces, out, clr = [], [], None, None
        for c in range(cycles):
            # without a smoother the kernel flies the act phase itself; with one it only plans, and every cycle's plan is a tensor of its own
            out = ops.mppi_closed_loop(prm, self.controller, self.simulator, st, *fl, goal, U, 1, 0 if smoothed else substeps, sim_dt, n_samples, iters,
                                       sigma, temperature, seed=seed, cycle_base=c, shift=sh, spheres=spheres, obstacle_weight=obstacle_weight, wind=wind,
                                       want_plan=log or smoothed, clearance=clr, want_clearance=not smoothed, sphere_vel=sphere_velocities,
                                       sphere_t0=sphere_t0 + (c * substeps) * sim_dt if smoothed else sphere_t0)
            clr = out["clearance"]
            traces.append(out["trace"])
            if smoothed:
                flat = out["plan_last"].view(B, 9 * N)            # (P, V, A) of drone b: 3N values each, 9N apart from drone to drone
                act(((c * substeps * sim_dt) + k * prm.dt, flat, flat[:, 3 * N:], flat[:, 6 * N:]))
            if log:
                logs.append(dict(plan_last=out["plan_last"], trace=out["trace"], cost=out["cost"]))
        trace = torch.cat(traces, dim=1) if traces else torch.zeros(B, 0, max(int(iters), 0), dtype=p0.dtype, device=ops.be.device)
        return self._result(st, sm, fl, logs=logs, U=U, cost=None if out is None else out["cost"], trace=trace, clearance=clr, mixer_state=mx)

    def run_mppi_fused(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float,
                       temperature: float, seed: int = 0, spheres=None, obstacle_weight: float = 0.0, wind=None, shift: Optional[int] = None,
                       nominal=None, log: bool = False, smoother=None, mixer=None, motor_health=None, sphere_velocities=None,
                       sphere_t0: float = 0.0, tracks=None):
        """:meth:`run_mppi` in ONE launch: every drone's `cycles` planning cycles inside one kernel, the plan never leaving the chip.  Same
        code, same bits as :meth:`run_mppi`, same arguments and the same shift rule (shift=None: ``floor(substeps * sim_dt / params.dt +
        0.5)`` clipped to [0, N]).  `log` keeps the last cycle's plan only: logs = [dict(plan_last, trace, cost)] with one entry.

        Measured on an MI355X (256 samples, 8 iterations, N = 30, 33 cycles x 15 steps): at 256 drones this is the fastest
        form, 9 - 16 % ahead of the per-cycle chain of se3mpc_mppi_* + se3mpc_rollout_cost_grad_* + se3mpc_extract_* + se3mpc_closed_loop_*.
        At 4096 drones it is 17 - 27 % SLOWER than that chain (the kernel holds the controller's registers, so the MPPI phase runs at three
        (float32) / two (float64) wavefronts per SIMD instead of four, and one lane per workgroup flies while the others wait): for thousands of
        drones drive the chain (``tools/gpu_probe_mppi_closed_loop.py``, ``chain_form``) unless the clearance output is what you need.
        sphere_velocities, sphere_t0: as in :meth:`run_mppi` -- the table advances through all `cycles` inside the one kernel.
        tracks: None, or (cycles, B, N, Kt, 4) rows (x, y, z, r): spheres with a predicted path, renewed every cycle, behind the moving ones
        (``se3mpc_mppi_closed_loop_tracks_*``): row [c][b][k][j] is sphere j at the time of the state before step k of
        drone b's plan in cycle c.  The clearance does not see them."""
        self._no_smoother(smoother, "run_mppi_fused")
        self._no_mixer(mixer, motor_health, "run_mppi_fused")
        st, sm, fl = self._start(p0, v0)
        U = self._mppi_start(p0, nominal)
        sh = self.resolve_shift(substeps, sim_dt, shift)
        entry = self.ops.mppi_closed_loop if tracks is None else functools.partial(self.ops.mppi_closed_loop_tracks, tracks=tracks)
        out = entry(self.params, self.controller, self.simulator, st, *fl, goal, U, cycles, substeps, sim_dt,
                    n_samples, iters, sigma, temperature, seed=seed, cycle_base=0, shift=sh, spheres=spheres,
                    obstacle_weight=obstacle_weight, wind=wind, want_plan=log, sphere_vel=sphere_velocities, sphere_t0=sphere_t0)
        logs = [dict(plan_last=out["plan_last"], trace=out["trace"], cost=out["cost"])] if log else []
        return self._result(st, sm, fl, logs=logs, U=U, cost=out["cost"], trace=out["trace"], clearance=out["clearance"])

    def run_mppi_swarm(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float,
                       temperature: float, seed: int = 0, spheres=None, obstacle_weight: float = 0.0, wind=None, shift: Optional[int] = None,
                       nominal=None, log: bool = False, smoother=None, mixer=None, motor_health=None, sphere_velocities=None,
                       sphere_t0: float = 0.0, swarm_size: int = 1, neighbours: int = 0, mate_radius: float = 0.0,
                       want_neighbours: bool = False, share_plans: bool = False):
        """:meth:`run_mppi_fused` for swarms (``se3mpc_mppi_closed_loop_swarm_*``): the B drones are B / `swarm_size` swarms
        of `swarm_size` consecutive drones, and every drone plans around its `neighbours` nearest swarm-mates as spheres of radius
        `mate_radius` that keep the velocity they have when the cycle starts (`obstacle_weight` weighs them like the shared `spheres`).
        One call enqueues every cycle (one launch each, the drones' states handed over through a snapshot between launches), then
        ``se3mpc_swarm_separation_*`` on the final state.  -> what :meth:`run_mppi_fused` returns (clearance: against the shared spheres
        only), plus separation (B,) = the minimum over the cycle starts and the final state of the distance to the nearest mate, and
        neighbours (B, `neighbours`) int32 = the mates chosen in the last cycle (None unless `want_neighbours`).  With swarm_size = 1 it is
        :meth:`run_mppi_fused`, bit for bit.  There is no staged or edge form.
        share_plans: the mates are shown as their plans, not as their velocities (``se3mpc_mppi_closed_loop_swarm_intent_*``, DESIGN.md
        5.8h): a mate's sphere at step k of the horizon is where the rollout of its own nominal puts it; `neighbours` <= 16."""
        self._no_smoother(smoother, "run_mppi_swarm")
        self._no_mixer(mixer, motor_health, "run_mppi_swarm")
        st, sm, fl = self._start(p0, v0)
        U = self._mppi_start(p0, nominal)
        sh = self.resolve_shift(substeps, sim_dt, shift)
        out = self.ops.mppi_closed_loop_swarm(self.params, self.controller, self.simulator, st, *fl, goal, U, cycles, substeps, sim_dt,
                                              n_samples, iters, sigma, temperature, swarm_size=swarm_size, neighbours=neighbours,
                                              mate_radius=mate_radius, seed=seed, cycle_base=0, shift=sh, spheres=spheres,
                                              obstacle_weight=obstacle_weight, wind=wind, want_plan=log, sphere_vel=sphere_velocities,
                                              sphere_t0=sphere_t0, want_neighbours=want_neighbours, share_plans=share_plans)
        sep = self.ops.swarm_separation(fl[1], fl[2], swarm_size, separation=out["separation"])
        logs = [dict(plan_last=out["plan_last"], trace=out["trace"], cost=out["cost"])] if log else []
        return self._result(st, sm, fl, logs=logs, U=U, cost=out["cost"], trace=out["trace"], clearance=out["clearance"], separation=sep,
                            neighbours=out["neighbours"])

    def run_mppi_fused_staged(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float,
                              temperature: float, seed: int = 0, spheres=None, obstacle_weight: float = 0.0, wind=None,
                              shift: Optional[int] = None, nominal=None, log: bool = False, smoother: Optional[SmootherParams] = None,
                              mixer: Optional[MixerParams] = None, motor_health=None, sphere_velocities=None, sphere_t0: float = 0.0):
        """:meth:`run_mppi` with `smoother` and / or `mixer` (and `motor_health`) in ONE launch (``se3mpc_mppi_closed_loop_staged_*``): every
        cycle's MPPI iterations, update_trajectory and control / mixer / simulator steps inside one kernel, where :meth:`run_mppi` makes
        three launches per cycle -- and with ``clearance`` (B,) filled in whenever there are spheres, which the chain cannot measure.  Same
        code, same bits, same arguments, shift rule and result keys as :meth:`run_mppi`; `log` keeps the last cycle's plan only, as
        :meth:`run_mppi_fused`; without both stages it is :meth:`run_mppi_fused`.  The kernel keeps ONE plan per drone on the chip:
        update_trajectory reads the plan being followed only at the drone's clock, so that one sample is taken before the next plan
        overwrites it; the sample comes back as ``followed`` (B, 9) with a smoother, and ``Ops.mppi_closed_loop_staged``
        takes it to continue a run.

        Which form at which batch size: not measured (``tools/gpu_probe_mppi_closed_loop_staged.py`` is the probe: 256 and 4096 drones, 256 samples,
        8 iterations, N = 30, 16 spheres, 33 cycles x 15 steps, both stages, against the 99 launches of :meth:`run_mppi`).  What the neighbouring
        forms measured suggests this one for small batches, where the chain is launch-bound, and :meth:`run_mppi` for
        thousands of drones -- one lane per workgroup flies the act phase, and with both stages the MPPI phase runs at two (float32) / one
        (float64) wavefront per SIMD -- unless the clearance, which only this form measures with the stages, or one enqueue is what you need."""
        self._no_moving(sphere_velocities, "run_mppi_fused_staged")
        self._mixer_option(mixer, motor_health)
        ops = self.ops
        st, sm, fl = self._start(p0, v0, smoother)
        mx = ops.mixer_state(p0.shape[0]) if mixer is not None else None
        U = self._mppi_start(p0, nominal)
        sh = self.resolve_shift(substeps, sim_dt, shift)
        out = ops.mppi_closed_loop_staged(self.params, self.controller, self.simulator, st, *fl, goal, U, cycles, substeps, sim_dt, n_samples, iters,
                                          sigma, temperature, seed=seed, cycle_base=0, shift=sh, spheres=spheres, obstacle_weight=obstacle_weight,
                                          wind=wind, want_plan=log, smoother=smoother, smoother_state=sm, mixer=mixer, mixer_state=mx,
                                          motor_health=motor_health)
        logs = [dict(plan_last=out["plan_last"], trace=out["trace"], cost=out["cost"])] if log else []
        more = dict(followed=out["followed"]) if smoother is not None else {}
        return self._result(st, sm, fl, logs=logs, U=U, cost=out["cost"], trace=out["trace"], clearance=out["clearance"], mixer_state=mx, **more)

    def run_mppi_edge(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float, temperature: float,
                      seed: int = 0, spheres=None, obstacle_weight: float = 0.0, wind=None, shift: Optional[int] = None, nominal=None,
                      latency_depth: int = 5, onboard: Optional[OnboardParams] = None, log: bool = False, sphere_velocities=None,
                      sphere_t0: float = 0.0):
        """The receding-horizon Monte-Carlo with MPPI as the planner on the reference's edge loop (edge/main.py:80-95), as a chain of two
        launches per cycle: ``se3mpc_mppi_closed_loop_*`` as the planner alone (one cycle, no simulator steps, on a scratch geometric-controller
        record it leaves untouched; arguments and shift rule as :meth:`run_mppi`), then ONE ``se3mpc_edge_loop_*`` launch of `substeps` x
        (latency push -> OnboardController.compute_control_command -> DroneSimulator.step) that reads the handed-over plan in place
        (latency_depth, onboard and the stale-state zero command as :meth:`run_edge`).
        -> the keys of :meth:`run_edge` (pos, vel, att, omega, time, onboard_state, latency, zero_thrust_steps, logs) plus U (B, N, 3) = the
        next cycle's nominal, cost (B,) at the last cycle's nominal, trace (B, cycles, iters) and clearance = None (no launch of this chain
        measures it); logs = [(planner outputs, edge-loop outputs)] per cycle if `log`.
        :meth:`run_mppi_edge_fused` is the same run in one launch, with the clearance (``se3mpc_mppi_closed_loop_edge_*``; measured at 0.92 - 0.97 of
        this chain's time for 256 drones and 0.98 - 1.05 for 4096 at 256 samples x 8 iterations, N = 30: DESIGN.md 5.8e; other shapes: not measured);
        this chain stays the form with per-step logs."""
        import torch
        self._no_moving(sphere_velocities, "run_mppi_edge")
        ops, prm = self.ops, self.params
        B, N = p0.shape[0], prm.horizon
        op = onboard if onboard is not None else ops.lib.onboard_default_params()
        scratch, _, fl = self._start(p0, v0)                  # the planner's entry point wants a controller record; with no steps it never reads it
        st = ops.onboard_state(B)
        buf = ops.latency_buffer(B, latency_depth, ops.be.suffix(p0))
        zeros = torch.zeros(B, dtype=torch.int32, device=ops.be.device)
        U = self._mppi_start(p0, nominal)
        sh = self.resolve_shift(substeps, sim_dt, shift)
        k = torch.arange(N, dtype=torch.float64, device=ops.be.device)
        logs, traces, out = [], [], None
        for c in range(cycles):
            out = ops.mppi_closed_loop(prm, self.controller, self.simulator, scratch, *fl, goal, U, 1, 0, sim_dt, n_samples, iters, sigma, temperature,
                                       seed=seed, cycle_base=c, shift=sh, spheres=spheres, obstacle_weight=obstacle_weight, wind=wind, want_plan=True,
                                       want_clearance=False)
            traces.append(out["trace"])
            flat = out["plan_last"].view(B, 9 * N)                # (P, V, A) of drone b: 3N values each, 9N apart from drone to drone
            flown = ops.edge_loop(op, self.simulator, st, buf, *fl, (c * substeps * sim_dt) + k * prm.dt, flat, flat[:, 3 * N:], flat[:, 6 * N:],
                                  nsteps=substeps, sim_dt=sim_dt, strides=(9 * N, 9 * N, 9 * N), wind=wind, log=log, zero_thrust_steps=zeros)
            if log:
                logs.append((out, flown))
        trace = torch.cat(traces, dim=1) if traces else torch.zeros(B, 0, max(int(iters), 0), dtype=p0.dtype, device=ops.be.device)
        time, pos, vel, att, om = fl
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, onboard_state=st, latency=buf, zero_thrust_steps=zeros, logs=logs, U=U,
                    cost=None if out is None else out["cost"], trace=trace, clearance=None)

    def run_mppi_edge_fused(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float,
                            temperature: float, seed: int = 0, spheres=None, obstacle_weight: float = 0.0, wind=None, shift: Optional[int] = None,
                            nominal=None, latency_depth: int = 5, onboard: Optional[OnboardParams] = None, want_last_plan: bool = False,
                            sphere_velocities=None, sphere_t0: float = 0.0):
        """:meth:`run_mppi_edge` in ONE launch (``se3mpc_mppi_closed_loop_edge_*``): every cycle's MPPI iterations and its
        `substeps` x (latency push -> OnboardController -> DroneSimulator.step) inside one kernel, the plan never leaving the chip, where
        :meth:`run_mppi_edge` makes two launches per cycle -- and with ``clearance`` (B,) filled in whenever there are spheres, which the chain
        cannot measure: the one form that says what the delay costs the sampling planner in clearance.  Same code, same bits, same arguments
        and shift rule as :meth:`run_mppi_edge` (no logs); the same result keys, plus plan_last (B, 3, N, 3) = the last cycle's plan if
        `want_last_plan`, else None.  All cross-cycle state is in the returned operands (U, onboard_state, latency, time, zero_thrust_steps,
        clearance), so ``Ops.mppi_closed_loop_edge`` with ``cycle_base=cycles`` continues the run.

        Measured on an MI355X (``profiles/mppi_closed_loop_edge.json``; 256 samples, 8 iterations, N = 30, 33 cycles x 15 steps, 0 and 16
        spheres, depth 0 and 5): at 256 drones 10.95 - 19.16 ms (float32) / 20.71 - 29.24 ms (float64) against 11.78 - 20.15 / 21.54 - 30.05 ms for the 66
        launches of :meth:`run_mppi_edge` -- 0.92 - 0.97 of the chain's time; at 4096 drones 90.8 - 125.1 / 236.9 - 304.1 ms against 88.0 - 125.8 / 232.0 -
        300.1 ms -- 1.02 - 1.05 without spheres, 0.98 - 1.01 with 16 (one lane per workgroup flies the act phase while the others wait; the chain's
        planner is the same three / two wavefronts per SIMD kernel, so the gap is small).  Use this form for hundreds of drones, and at any size when
        the clearance or one enqueue is what you need; for thousands of drones without spheres :meth:`run_mppi_edge` is a few per cent faster.  Other
        batch sizes, sample counts and horizons: not measured; :meth:`run_mppi_edge` stays the form with per-step logs."""
        import torch
        self._no_moving(sphere_velocities, "run_mppi_edge_fused")
        ops = self.ops
        B = p0.shape[0]
        op = onboard if onboard is not None else ops.lib.onboard_default_params()
        # the flight state of _start, without the geometric controller's records: this loop has none
        fl = (torch.zeros(B, dtype=torch.float64, device=ops.be.device), p0.clone(), v0.clone(), torch.zeros_like(p0), torch.zeros_like(p0))
        st = ops.onboard_state(B)
        buf = ops.latency_buffer(B, latency_depth, ops.be.suffix(p0))
        zeros = torch.zeros(B, dtype=torch.int32, device=ops.be.device)
        U = self._mppi_start(p0, nominal)
        sh = self.resolve_shift(substeps, sim_dt, shift)
        out = ops.mppi_closed_loop_edge(self.params, op, self.simulator, st, buf, *fl, goal, U, cycles, substeps, sim_dt, n_samples, iters, sigma,
                                        temperature, seed=seed, cycle_base=0, shift=sh, spheres=spheres, obstacle_weight=obstacle_weight, wind=wind,
                                        want_plan=want_last_plan, zero_thrust_steps=zeros)
        time, pos, vel, att, om = fl
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, onboard_state=st, latency=buf, zero_thrust_steps=zeros, logs=[], U=U,
                    cost=out["cost"], trace=out["trace"], clearance=out["clearance"], plan_last=out["plan_last"])

    def capture(self, B: int, dtype, cycles: int, substeps: int, sim_dt: float, with_wind: bool = True, smoother=None, mixer=None,
                motor_health=None):
        """The whole Monte-Carlo (2 x `cycles` kernel launches + the plan stamps) captured ONCE into a hipGraph; each call of the
        returned function copies new initial conditions into the graph's static inputs, replays it and returns the static outputs
        (overwritten by the next call).  Removes the per-launch host cost (~30 us of Python + launch per call, 66 calls per run)."""
        import torch
        self._no_smoother(smoother, "capture")
        self._no_mixer(mixer, motor_health, "capture")
        dev = self.ops.be.device
        static = dict(p0=torch.zeros(B, 3, dtype=dtype, device=dev), v0=torch.zeros(B, 3, dtype=dtype, device=dev),
                      goal=torch.zeros(B, 3, dtype=dtype, device=dev), wind=torch.zeros(B, 3, dtype=dtype, device=dev) if with_wind else None)
        run = lambda: self.run(static["p0"], static["v0"], static["goal"], cycles, substeps, sim_dt, wind=static["wind"])
        run()                                                    # warm-up outside the capture (library load, allocator pools)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                out = run()
        torch.cuda.current_stream().wait_stream(side)

        def replay(p0, v0, goal, wind=None):
            static["p0"].copy_(p0); static["v0"].copy_(v0); static["goal"].copy_(goal)
            if with_wind:
                static["wind"].copy_(wind) if wind is not None else static["wind"].zero_()
            graph.replay()
            return out
        replay.graph = graph
        return replay
