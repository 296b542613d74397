"""Batched closed loop on the device: planner -> (plan sample -> geometric controller -> simulator) for many drones at once.

What the reference's closed-loop tests do one drone and one Python call at a time
(tests/test_planner_controller_contract.py:115-162, :255-316; tests/test_monte_carlo_sim.py:24-72) runs here as two launches
per planning cycle for B drones: ``se3mpc_solve_*`` (every drone re-plans from its own state) and ``se3mpc_closed_loop_*``
(``substeps`` control + simulator steps against the fresh plan, which is read in place from the solver's outputs).  No host
arithmetic, no copies between the two; the only host work per cycle is the N plan stamps (planner.py:661: start + arange(N)*dt).
``run_mppi`` / ``run_mppi_fused`` close the same loop with MPPI as the planner (``se3mpc_mppi_closed_loop_*``: plan, control and simulate
inside one kernel, the plan handed over in LDS).  ``run(..., smoother=SmootherParams)`` / ``run_mppi(..., smoother=...)`` put the reference's
TrajectorySmoother between plan and controller, as its edge loop does (edge/main_improved.py:96-152): plan -> ``se3mpc_smoother_update_*`` ->
``se3mpc_closed_loop_smoothed_*`` per cycle; the one-launch forms do not have it.
"""
import math
from typing import Optional

from ..capi import ControllerParams, Params, SimulatorParams, SmootherParams


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

    def run(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, wind=None, log: bool = False,
            smoother: Optional[SmootherParams] = None):
        """p0, v0, goal: (B, 3) device tensors (float32 or float64: the precision of the whole loop); wind: None, (3,) or (B, 3) newtons.
        smoother: None, or the parameters of the reference's TrajectorySmoother: every fresh plan then goes through update_trajectory
        (against the previous cycle's plan, so the plan tensors alternate between two sets) and every control step takes its target from
        get_desired_state.  -> dict(pos, vel, att, omega (B, 3), time (B,), controller_state (B, 12), logs = [(solve outputs, closed-loop
        outputs)] if log[, smoother_state (B, 25)])."""
        import torch
        if smoother is not None:
            return self._run_smoothed(smoother, p0, v0, goal, cycles, substeps, sim_dt, wind, log)
        ops, prm = self.ops, self.params
        dev = ops.be.device
        B, N = p0.shape[0], prm.horizon
        pos, vel = p0.clone(), v0.clone()
        att, om = torch.zeros_like(p0), torch.zeros_like(p0)
        time = torch.zeros(B, dtype=torch.float64, device=dev)
        st = ops.controller_state(self.controller, B)
        k = torch.arange(N, dtype=torch.float64, device=dev)
        logs = []
        sol = None
        for c in range(cycles):
            # without logs every cycle writes the same plan tensors again (the closed-loop launch of a cycle is ordered before the next solve)
            sol = ops.solve(prm, pos, vel, goal, want_trajectory=True if log else "accelerations", out=None if log else sol)
            stamps = (c * substeps * sim_dt) + k * prm.dt
            X = sol["x"]
            out = ops.closed_loop(self.controller, self.simulator, st, time, pos, vel, att, om, stamps, X, X[:, 3 * N:], sol["accelerations"],
                                  nsteps=substeps, sim_dt=sim_dt, strides=(9 * N, 9 * N, 3 * N), wind=wind, stop_at_plan_end=False, log=log)
            if log:
                logs.append((sol, out))
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, controller_state=st, logs=logs)

    def _run_smoothed(self, smoother, p0, v0, goal, cycles, substeps, sim_dt, wind, log):
        import torch
        ops, prm = self.ops, self.params
        dev = ops.be.device
        B, N = p0.shape[0], prm.horizon
        pos, vel = p0.clone(), v0.clone()
        att, om = torch.zeros_like(p0), torch.zeros_like(p0)
        time = torch.zeros(B, dtype=torch.float64, device=dev)
        st, sm = ops.controller_state(self.controller, B), ops.smoother_state(B)
        k = torch.arange(N, dtype=torch.float64, device=dev)
        strides = (9 * N, 9 * N, 3 * N)
        logs, sols, old = [], [None, None], None
        for c in range(cycles):
            sol = ops.solve(prm, pos, vel, goal, want_trajectory=True if log else "accelerations", out=None if log else sols[c % 2])
            sols[c % 2] = sol
            X = sol["x"]
            new = ((c * substeps * sim_dt) + k * prm.dt, X, X[:, 3 * N:], sol["accelerations"])
            ops.smoother_update(smoother, sm, time, *new, strides=strides, old=old, old_strides=strides)      # the wall clock of update_trajectory = the drones' clocks
            out = ops.closed_loop_smoothed(smoother, self.controller, self.simulator, st, sm, time, pos, vel, att, om, *new, nsteps=substeps,
                                           sim_dt=sim_dt, strides=strides, wind=wind, log=log)
            old = new
            if log:
                logs.append((sol, out))
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, controller_state=st, logs=logs, smoother_state=sm)

    def run_fused(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, wind=None, want_last_plan: bool = False, smoother=None):
        """The same Monte-Carlo in ONE launch (``se3mpc_monte_carlo_*``: every cycle's solve and control / simulator steps inside one kernel,
        each drone paying only for its own slow solves instead of waiting, 2 x `cycles` times, at a kernel boundary for the slowest drone of
        the batch).  Same code, same bits as :meth:`run`.  One host synchronise at the end reads the overflow counter; if a solve needed more
        L-BFGS memory than the launch's LDS image holds (never with the reference's options) the run is repeated by :meth:`run`."""
        import torch
        self._no_smoother(smoother, "run_fused")
        ops = self.ops
        dev = ops.be.device
        B = p0.shape[0]
        pos, vel = p0.clone(), v0.clone()
        att, om = torch.zeros_like(p0), torch.zeros_like(p0)
        time = torch.zeros(B, dtype=torch.float64, device=dev)
        st = ops.controller_state(self.controller, B)
        out = ops.monte_carlo(self.params, self.controller, self.simulator, st, time, pos, vel, att, om, goal, cycles, substeps, sim_dt, wind=wind,
                              want_last_plan=want_last_plan)
        if int(ops.be.to_host(out["overflowed"])[0]) != 0:
            return self.run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind)
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, controller_state=st, logs=[], last_plan=out if want_last_plan else None)

    def resolve_shift(self, substeps: int, sim_dt: float, shift: Optional[int] = None) -> int:
        """Rows the MPPI nominal moves forward per planning cycle.  None: the plan steps one act phase covers, rounded half up,
        ``floor(substeps * sim_dt / params.dt + 0.5)`` clipped to [0, N]."""
        N = self.params.horizon
        if shift is None:
            shift = int(math.floor(substeps * sim_dt / self.params.dt + 0.5))
        return max(0, min(N, int(shift)))

    def _mppi_start(self, p0, v0, nominal):
        import torch
        ops, prm = self.ops, self.params
        B, N = p0.shape[0], prm.horizon
        pos, vel = p0.clone(), v0.clone()
        att, om = torch.zeros_like(p0), torch.zeros_like(p0)
        time = torch.zeros(B, dtype=torch.float64, device=ops.be.device)
        st = ops.controller_state(self.controller, B)
        if nominal is None:
            U = torch.zeros(B, N, 3, dtype=p0.dtype, device=ops.be.device)
            U[:, :, 2] = prm.mass * prm.gravity
        else:
            U = nominal.clone()
        return pos, vel, att, om, time, st, U

    def run_mppi(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float, temperature: float,
                 seed: int = 0, spheres=None, obstacle_weight: float = 0.0, wind=None, shift: Optional[int] = None, nominal=None,
                 log: bool = False, smoother: Optional[SmootherParams] = None):
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
        ``se3mpc_closed_loop_smoothed_*``; clearance is None (only the fused act phase measures it), smoother_state (B, 25) is added."""
        import torch
        ops = self.ops
        pos, vel, att, om, time, st, U = self._mppi_start(p0, v0, nominal)
        sh = self.resolve_shift(substeps, sim_dt, shift)
        if smoother is not None:
            return self._run_mppi_smoothed(smoother, pos, vel, att, om, time, st, U, sh, goal, cycles, substeps, sim_dt, n_samples, iters, sigma,
                                           temperature, seed, spheres, obstacle_weight, wind, log)
        logs, traces, out, clr = [], [], None, None
        for c in range(cycles):
            out = ops.mppi_closed_loop(self.params, self.controller, self.simulator, st, time, pos, vel, att, om, goal, U, 1, substeps, sim_dt,
                                       n_samples, iters, sigma, temperature, seed=seed, cycle_base=c, shift=sh, spheres=spheres,
                                       obstacle_weight=obstacle_weight, wind=wind, want_plan=log, clearance=clr)
            clr = out["clearance"]
            traces.append(out["trace"])
            if log:
                logs.append(dict(plan_last=out["plan_last"], trace=out["trace"], cost=out["cost"]))
        trace = torch.cat(traces, dim=1) if traces else torch.zeros(p0.shape[0], 0, max(int(iters), 0), dtype=p0.dtype, device=ops.be.device)
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, controller_state=st, logs=logs, U=U, cost=None if out is None else out["cost"],
                    trace=trace, clearance=clr)

    def _run_mppi_smoothed(self, smoother, pos, vel, att, om, time, st, U, sh, goal, cycles, substeps, sim_dt, n_samples, iters, sigma, temperature,
                           seed, spheres, obstacle_weight, wind, log):
        import torch
        ops, prm = self.ops, self.params
        B, N = pos.shape[0], prm.horizon
        sm = ops.smoother_state(B)
        k = torch.arange(N, dtype=torch.float64, device=ops.be.device)
        strides = (9 * N, 9 * N, 9 * N)
        logs, traces, out, old = [], [], None, None
        for c in range(cycles):
            out = ops.mppi_closed_loop(prm, self.controller, self.simulator, st, time, pos, vel, att, om, goal, U, 1, 0, sim_dt, n_samples, iters, sigma,
                                       temperature, seed=seed, cycle_base=c, shift=sh, spheres=spheres, obstacle_weight=obstacle_weight, wind=wind,
                                       want_plan=True, want_clearance=False)
            traces.append(out["trace"])
            flat = out["plan_last"].view(B, 9 * N)                # (P, V, A) of drone b: 3N values each, 9N apart from drone to drone
            new = ((c * substeps * sim_dt) + k * prm.dt, flat, flat[:, 3 * N:], flat[:, 6 * N:])
            ops.smoother_update(smoother, sm, time, *new, strides=strides, old=old, old_strides=strides)
            ops.closed_loop_smoothed(smoother, self.controller, self.simulator, st, sm, time, pos, vel, att, om, *new, nsteps=substeps, sim_dt=sim_dt,
                                     strides=strides, wind=wind)
            old = new
            if log:
                logs.append(dict(plan_last=out["plan_last"], trace=out["trace"], cost=out["cost"]))
        trace = torch.cat(traces, dim=1) if traces else torch.zeros(B, 0, max(int(iters), 0), dtype=pos.dtype, device=ops.be.device)
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, controller_state=st, logs=logs, U=U, cost=None if out is None else out["cost"],
                    trace=trace, clearance=None, smoother_state=sm)

    def run_mppi_fused(self, p0, v0, goal, cycles: int, substeps: int, sim_dt: float, n_samples: int, iters: int, sigma: float,
                       temperature: float, seed: int = 0, spheres=None, obstacle_weight: float = 0.0, wind=None, shift: Optional[int] = None,
                       nominal=None, log: bool = False, smoother=None):
        """:meth:`run_mppi` in ONE launch: every drone's `cycles` planning cycles inside one kernel, the plan never leaving the chip.  Same
        code, same bits as :meth:`run_mppi`, same arguments and the same shift rule (shift=None: ``floor(substeps * sim_dt / params.dt +
        0.5)`` clipped to [0, N]).  `log` keeps the last cycle's plan only: logs = [dict(plan_last, trace, cost)] with one entry.

        Measured on an MI355X (256 samples, 8 iterations, N = 30, 33 cycles x 15 steps): at 256 drones this is the fastest
        form, 9 - 16 % ahead of the per-cycle chain of se3mpc_mppi_* + se3mpc_rollout_cost_grad_* + se3mpc_extract_* + se3mpc_closed_loop_*.
        At 4096 drones it is 17 - 27 % SLOWER than that chain (the kernel holds the controller's registers, so the MPPI phase runs at three
        (float32) / two (float64) wavefronts per SIMD instead of four, and one lane per workgroup flies while the others wait): for thousands of
        drones drive the chain (``tools/gpu_probe_mppi_closed_loop.py``, ``chain_form``) unless the clearance output is what you need."""
        self._no_smoother(smoother, "run_mppi_fused")
        ops = self.ops
        pos, vel, att, om, time, st, U = self._mppi_start(p0, v0, nominal)
        sh = self.resolve_shift(substeps, sim_dt, shift)
        out = ops.mppi_closed_loop(self.params, self.controller, self.simulator, st, time, pos, vel, att, om, goal, U, cycles, substeps, sim_dt,
                                   n_samples, iters, sigma, temperature, seed=seed, cycle_base=0, shift=sh, spheres=spheres,
                                   obstacle_weight=obstacle_weight, wind=wind, want_plan=log)
        logs = [dict(plan_last=out["plan_last"], trace=out["trace"], cost=out["cost"])] if log else []
        return dict(pos=pos, vel=vel, att=att, omega=om, time=time, controller_state=st, logs=logs, U=U, cost=out["cost"], trace=out["trace"],
                    clearance=out["clearance"])

    def capture(self, B: int, dtype, cycles: int, substeps: int, sim_dt: float, with_wind: bool = True, smoother=None):
        """The whole Monte-Carlo (2 x `cycles` kernel launches + the plan stamps) captured ONCE into a hipGraph; each call of the
        returned function copies new initial conditions into the graph's static inputs, replays it and returns the static outputs
        (overwritten by the next call).  Removes the per-launch host cost (~30 us of Python + launch per call, 66 calls per run)."""
        import torch
        self._no_smoother(smoother, "capture")
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
