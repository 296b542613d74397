#!/usr/bin/env python3
"""Golden vectors for the TrajectorySmoother, produced by RUNNING THE REFERENCE'S OWN CLASS in the build container
(/root/reference/src/dart_planner/control/trajectory_smoother.py) with the identity-units stand-in of make_golden.py, logging disabled and the
smoother module's ``time.time`` pinned (update_trajectory reads the wall clock, :122):

* call sequences on fresh smoothers: ``get_desired_state`` every 10 ms with ``update_trajectory`` calls in between; after EVERY call the returned
  triple and every member of the state record (SE3MPC_SMOOTHER_STATE_WORDS, include/se3mpc.h) are recorded;
* the private methods' returns at recorded arguments (``_interpolate_trajectory``, ``_generate_transition_state``, ``_get_failsafe_trajectory``,
  ``_apply_trajectory_limits``, ``_smooth_trajectory_point``);
* closed loops of the reference's smoother + ``GeometricController`` + ``DroneSimulator`` at 1 kHz around three plans 100 ms apart, one of
  them with the second plan's start switched by (2, 1, 0) m; for that one the largest one-step change of the commanded position with the
  smoother and of the raw plan sample without it.

The generator asserts (through tests/smoother_oracle.py, which it also compares to the reference call by call) that every branch code and
every clamp is hit at least 5 times and that every discontinuous decision keeps a relative margin of 1e-6 from its threshold, so that a
last-bit difference cannot flip a case.  Only inputs and outputs of the reference go into the files.  Writes smoother_cases.npz / .json.
"""
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.environ.get("SE3MPC_GOLDEN_OUT", HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _install_standins  # noqa: E402
import smoother_oracle as so  # noqa: E402

MARGIN = 1e-6
CALL_DT = 0.01


def main():
    tmp = _install_standins()
    try:
        import logging
        logging.disable(logging.CRITICAL)
        import dart_planner.control.trajectory_smoother as sm_mod
        from dart_planner.control.trajectory_smoother import TrajectorySmoother
        from dart_planner.control.geometric_controller import GeometricController
        from dart_planner.utils.drone_simulator import DroneSimulator
        from dart_planner.common.types import DroneState, Trajectory

        clock = {"t": 0.0}
        sm_mod.time.time = lambda: clock["t"]

        def mkstate(t, p, v, a=(0, 0, 0), w=(0, 0, 0)):
            return DroneState(timestamp=float(t), position=np.array(p, float), velocity=np.array(v, float), attitude=np.array(a, float),
                              angular_velocity=np.array(w, float))

        def record(s):
            bits = (1 if s.current_trajectory is not None else 0) | (2 if s.in_transition else 0)
            return np.concatenate([s.last_filtered_pos, s.last_filtered_vel, s.last_filtered_acc, s.transition_start_pos, s.transition_start_vel,
                                   s.transition_target_pos, s.transition_target_vel,
                                   [s.transition_start_time, s.last_cloud_update, s.trajectory_start_time, bits]]).astype(float)

        def traj(plan):
            ts, P, V, A = plan
            return Trajectory(timestamps=np.array(ts, float), positions=np.array(P, float), velocities=None if V is None else np.array(V, float),
                              accelerations=None if A is None else np.array(A, float))

        def oracle_params(s):
            return so.params(transition_time=s.transition_time, velocity_limit=s.velocity_limit, acceleration_limit=s.acceleration_limit,
                             jerk_limit=s.jerk_limit)

        out, meta = {}, {"sequences": [], "loops": []}
        rng = np.random.default_rng(20261018)
        hits = {"branch": np.zeros(5, int), "clamps": np.zeros(5, int)}
        worst = {"margin": np.inf, "oracle_error": 0.0}

        def line_plan(N, dt, p0, v, a=None, t_first=0.0, with_v=True, with_a=True, wobble=0.0):
            k = np.arange(N)[:, None] * dt
            a = np.zeros(3) if a is None else np.asarray(a, float)
            P = np.asarray(p0, float) + np.asarray(v, float) * k + 0.5 * a * k * k + wobble * rng.normal(0, 1, (N, 3))
            V = np.asarray(v, float) + a * k + wobble * rng.normal(0, 1, (N, 3))
            A = np.broadcast_to(a, (N, 3)) + wobble * rng.normal(0, 1, (N, 3))
            return (t_first + np.arange(N) * dt, P, V if with_v else None, A if with_a else None)

        class Tracker:
            """The oracle on the same calls: coverage, margins and its own error against the reference."""
            def __init__(self, s):
                self.state, self.plan = so.reset(1), None
                self.s = s

            def update(self, now, plan):
                d = {}
                so.update(oracle_params(self.s), self.state, np.array([now]), self.plan, plan, diag=d)
                self.plan = plan
                worst["margin"] = min(worst["margin"], float(d["margin"][0]))
                return d

            def desired(self, now, pos, vel, ref_out, ref_rec):
                d = {}
                x, br = so.desired(oracle_params(self.s), self.state, np.array([now]), pos[None], vel[None], self.plan, diag=d)
                worst["margin"] = min(worst["margin"], float(d["margin"][0]))
                worst["oracle_error"] = max(worst["oracle_error"], float(np.max(np.abs(x[0] - ref_out))), float(np.max(np.abs(self.state[0] - ref_rec))))
                hits["branch"][br[0]] += 1
                hits["clamps"] += d["clamps"][0]
                return int(br[0])

        # ------------------------------------------------------------------ A. call sequences
        def sequence(tag, ncalls, t0, plans, updates, pos0, vel0=(0.0, 0.0, 0.0), moving=False, transition_time=0.5, **members):
            """updates: [(call index, clock offset, plan index)]: before that get_desired_state call the wall clock is pinned to
            t_call + offset and update_trajectory(plans[plan index]) runs."""
            s = TrajectorySmoother(transition_time=transition_time)
            for k, v in members.items():
                assert hasattr(s, k)
                setattr(s, k, v)
            trk = Tracker(s)
            ev = {k: [] for k in ("kind", "t", "plan", "pos", "vel", "out", "branch", "state")}
            pos, vel = np.array(pos0, float), np.array(vel0, float)
            # every update gets an offset of its own: the time between two updates is no multiple of the call period or a plan step
            pending = sorted((k, off + 0.00013 * i, pi) for i, (k, off, pi) in enumerate(sorted(updates)))
            for k in range(ncalls):
                t = t0 + k * CALL_DT
                while pending and pending[0][0] == k:
                    _, off, pi = pending.pop(0)
                    clock["t"] = t + off
                    s.update_trajectory(traj(plans[pi]), mkstate(t, pos, vel))
                    trk.update(clock["t"], plans[pi])
                    rec = record(s)
                    assert np.array_equal(rec, trk.state[0]) or np.max(np.abs(rec - trk.state[0])) <= 1e-10
                    for nm, v in (("kind", 1), ("t", clock["t"]), ("plan", pi), ("pos", pos), ("vel", vel), ("out", np.full(9, np.nan)), ("branch", -1),
                                  ("state", rec)):
                        ev[nm].append(np.array(v))
                if moving:
                    pos = pos + rng.normal(0, 0.02, 3); vel = vel + rng.normal(0, 0.05, 3)
                r = s.get_desired_state(t, mkstate(t, pos, vel))
                res = np.concatenate([np.array(x, float) for x in r])
                rec = record(s)
                br = trk.desired(t, pos, vel, res, rec)
                for nm, v in (("kind", 0), ("t", t), ("plan", -1), ("pos", pos), ("vel", vel), ("out", res), ("branch", br), ("state", rec)):
                    ev[nm].append(np.array(v))
            key = f"q{len(meta['sequences']):02d}_"
            for nm, v in ev.items():
                out[key + nm] = np.array(v)
            for pi, (ts, P, V, A) in enumerate(plans):
                out[f"{key}pl{pi}_ts"], out[f"{key}pl{pi}_P"] = np.array(ts, float), np.array(P, float).reshape(-1, 3)
                if V is not None:
                    out[f"{key}pl{pi}_V"] = np.array(V, float)
                if A is not None:
                    out[f"{key}pl{pi}_A"] = np.array(A, float)
            meta["sequences"].append(dict(key=key, tag=tag, calls=ncalls, events=len(ev["kind"]), plans=len(plans), transition_time=transition_time,
                                          members={k: float(v) for k, v in members.items()}))

        OFF = 0.0037                                             # updates fall between two calls: no decision lands on a call's grid
        sequence("no_trajectory_then_failsafe", 150, 1.0037, [], [], (1.0, -2.0, 3.0), (0.8, -0.4, 0.2), moving=True)
        sequence("failsafe_through_the_decay_cap", 80, 6.5, [], [], (0.5, 0.5, 2.0), (1.5, 0.3, -0.6), moving=True)
        sequence("one_row_plans", 60, 10.0, [line_plan(1, 0.05, (1, 2, 3), (0.4, 0, 0)), line_plan(1, 0.05, (1.2, 2.1, 3.0), (0.5, 0.1, 0))],
                 [(0, -OFF, 0), (30, OFF, 1)], (1, 2, 3))
        p2 = line_plan(2, 0.4, (0, 0, 0), (0.5, 0.25, 0.1), with_a=False)
        p2[2][0] = 0.0                                           # the exact origin with zero velocity: the filter is bypassed until the command leaves it
        sequence("two_rows_from_the_exact_origin", 80, 20.0, [p2, line_plan(2, 0.4, (0.3, 0.1, 0.0), (0.4, 0.3, 0.1))], [(0, 0.0237, 0), (50, OFF, 1)],
                 (0, 0, 0))
        sequence("six_rows_walk_and_large_update", 110, 30.0,
                 [line_plan(6, 0.05, (2, 1, 1.5), (1.0, 0.5, 0.0), with_a=False, wobble=0.02), line_plan(6, 0.05, (3.5, 1.5, 1.8), (0.8, 0.2, 0.1), wobble=0.02)],
                 [(0, OFF, 0), (40, OFF, 1)], (2, 1, 1.5))
        t0 = 40.0
        knots = np.array([(t0 + 3 * j * CALL_DT) - t0 for j in range(30)])      # exactly the trajectory times of every third call
        k30 = knots[:, None]
        exact = (knots, np.array([1.0, -1.0, 2.0]) + np.array([0.6, 0.3, -0.1]) * k30 + 0.05 * np.sin(3 * k30), np.array([0.6, 0.3, -0.1]) + 0.15 * np.cos(3 * k30) * np.ones(3),
                 -0.45 * np.sin(3 * k30) * np.ones(3))
        sequence("thirty_rows_exactly_on_the_knots", 120, t0, [exact], [(0, 0.0, 0)], (1, -1, 2))
        sequence("velocity_threshold_then_small_update", 110, 50.0,
                 [line_plan(6, 0.05, (0, 0, 2), (0.5, 0, 0)), line_plan(6, 0.05, (0.1, 0.0, 2.0), (1.9, 0.6, 0)), line_plan(6, 0.05, (0.25, 0.1, 2.0), (1.7, 0.5, 0))],
                 [(0, -OFF, 0), (20, OFF, 1), (40, OFF, 2)], (0, 0, 2))
        sequence("large_update_during_a_transition", 130, 60.0,
                 [line_plan(30, 0.02, (0, 0, 1), (0.3, 0.3, 0)), line_plan(30, 0.02, (1.5, 0, 1), (0.3, 0.0, 0)), line_plan(30, 0.02, (1.5, 2.0, 1.5), (0, 0.3, 0))],
                 [(0, -OFF, 0), (15, OFF, 1), (45, OFF, 2)], (0, 0, 1))
        sequence("transition_norm_clamps", 100, 70.0, [line_plan(6, 0.1, (0, 0, 1), (0, 0, 0)), line_plan(6, 0.1, (6, 5, 2), (1.2, 0, 0))],
                 [(0, -OFF, 0), (10, OFF, 1)], (0, 0, 1))
        sequence("per_call_clamps", 90, 80.0, [line_plan(6, 0.1, (1, 1, 1), (2.0, -1.0, 0.5), a=(3.0, 2.0, -1.0), wobble=0.3)], [(0, -OFF, 0)], (1, 1, 1))
        sequence("jerk_clamp", 90, 90.0, [line_plan(6, 0.1, (1, 1, 1), (0.5, 0.2, 0.0), a=(2.0, -1.5, 1.0), wobble=0.2)], [(0, -OFF, 0)], (1, 1, 1),
                 jerk_limit=1.0)
        sequence("timeout_after_a_plan", 260, 100.0, [line_plan(6, 0.05, (1, 0, 2), (0.2, 0.1, 0))], [(0, -OFF, 0)], (1, 0, 2), (0.6, -0.2, 0.1), moving=True)
        sequence("short_transitions", 100, 110.0,
                 [line_plan(6, 0.05, (0, 0, 1), (0.2, 0, 0)), line_plan(6, 0.05, (1, 0, 1), (0.2, 0, 0)), line_plan(2, 0.3, (1, 1.2, 1), (0, 0.2, 0)),
                  line_plan(6, 0.05, (0, 1.2, 1.6), (-0.2, 0, 0), with_v=False, with_a=False), line_plan(30, 0.01, (0.0, 0.0, 1.0), (0.1, 0.1, 0))],
                 [(0, -OFF, 0), (10, OFF, 1), (30, OFF, 2), (50, OFF, 3), (70, OFF, 4)], (0, 0, 1), transition_time=0.1)
        sequence("updates_below_both_thresholds", 80, 120.0,
                 [line_plan(2, 0.5, (1, 1, 1), (0.4, 0, 0)), line_plan(6, 0.05, (1.3, 1.25, 1.1), (1.0, 0.5, 0.3)), line_plan(2, 0.5, (1.6, 1.5, 1.2), (0.5, 0.1, 0))],
                 [(0, -OFF, 0), (25, OFF, 1), (50, OFF, 2)], (1, 1, 1))
        sequence("short_transitions_again", 70, 130.0,
                 [line_plan(6, 0.05, (0, 0, 1), (0, 0, 0)), line_plan(6, 0.05, (0.8, 0, 1), (0, 0, 0)), line_plan(6, 0.05, (0.8, 0.9, 1), (0, 0, 0))],
                 [(0, -OFF, 0), (10, OFF, 1), (35, OFF, 2)], (0, 0, 1), transition_time=0.2)

        # ------------------------------------------------------------------ B. the private methods at recorded arguments
        s = TrajectorySmoother()
        pl = line_plan(6, 0.05, (1, 2, 3), (0.7, -0.3, 0.2), a=(0.5, 0.1, -0.2), wobble=0.05)
        tq = np.concatenate([[-0.3, 0.0, 0.25, 0.6], rng.uniform(0.001, 0.249, 12)])
        out["m_plan_ts"], out["m_plan_P"], out["m_plan_V"], out["m_plan_A"] = pl
        out["m_interp_t"], out["m_interp_start"] = 500.0 + tq, np.array(500.0)
        out["m_interp_out"] = np.array([np.concatenate(s._interpolate_trajectory(float(500.0 + t), traj(pl), 500.0)) for t in tq])
        s.transition_start_pos, s.transition_start_vel = np.array([0.0, 1.0, 2.0]), np.array([0.3, 0.0, -0.1])
        s.transition_target_pos, s.transition_target_vel = np.array([1.5, 0.5, 2.5]), np.array([0.0, 0.4, 0.0])
        prog = np.concatenate([[0.0, 0.5], rng.uniform(0.01, 0.99, 10)])
        out["m_trans_record"] = record(s)
        out["m_trans_progress"] = prog
        out["m_trans_out"] = np.array([np.concatenate(s._generate_transition_state(float(p))) for p in prog])
        s.last_cloud_update = 300.0
        ft = 300.0 + np.array([2.5, 3.0, 6.9, 7.5, 20.0])
        fpos, fvel = rng.uniform(-3, 3, (5, 3)), rng.uniform(-2, 2, (5, 3))
        out["m_fail_t"], out["m_fail_pos"], out["m_fail_vel"] = ft, fpos, fvel
        out["m_fail_out"] = np.array([np.concatenate(s._get_failsafe_trajectory(float(t), mkstate(t, p, v))) for t, p, v in zip(ft, fpos, fvel)])
        s.last_filtered_vel, s.last_filtered_acc = np.array([0.2, 0.1, 0.0]), np.array([0.1, 0.0, -0.1])
        out["m_limits_record"] = record(s)
        lim_in = rng.uniform(-1, 1, (8, 9)) * np.array([3, 3, 3, 1, 1, 1, 0.2, 0.2, 0.2])
        lim_in[:3, 3:] = np.concatenate([s.last_filtered_vel, s.last_filtered_acc]) + rng.uniform(-0.01, 0.01, (3, 6))     # inside every limit
        out["m_limits_in"] = lim_in
        out["m_limits_dt"] = np.array(0.02)
        out["m_limits_out"] = np.array([np.concatenate(s._apply_trajectory_limits(r[0:3].copy(), r[3:6].copy(), r[6:9].copy(), 0.02)) for r in lim_in])
        s.last_filtered_pos = np.array([1.0, 2.0, 3.0])         # away from the origin: the filter runs; the calls chain through the filter state
        out["m_smooth_record"] = record(s)
        sm_out, sm_rec = [], []
        for r in lim_in:
            sm_out.append(np.concatenate(s._smooth_trajectory_point(r[0:3].copy(), r[3:6].copy(), r[6:9].copy(), 0.02)))
            sm_rec.append(record(s))
        out["m_smooth_out"], out["m_smooth_state"] = np.array(sm_out), np.array(sm_rec)

        # ------------------------------------------------------------------ C. closed loops at 1 kHz around three plans 100 ms apart
        T0, SIM_DT, PLAN_DT = 1000.0, 0.001, 0.01371              # the plan step shares no multiple with the simulator step inside a plan

        def closed_loop(tag, starts, vels, p0, wind=None, rows=30, with_a=True):
            sm = TrajectorySmoother()
            trk = Tracker(sm)
            ctrl = GeometricController(tuning_profile="sitl_optimized")
            sim = DroneSimulator(wind=None if wind is None else np.array(wind, float))
            st = mkstate(T0, p0, (0, 0, 0))
            log = {k: [] for k in ("pos", "vel", "att", "omega", "t", "thrust", "torque", "target", "raw", "sm_state", "update_t")}
            plans, cur, cur_start = [], None, None
            for i in range(300):
                t = st.timestamp
                if i % 100 == 0:
                    c = i // 100
                    plan = line_plan(rows, PLAN_DT, starts[c], vels[c], t_first=t, with_a=with_a)
                    plans.append(plan)
                    clock["t"] = t
                    sm.update_trajectory(traj(plan), st)
                    trk.update(t, plan)
                    cur, cur_start = plan, t
                    log["update_t"].append(t)
                tp, tv, ta = sm.get_desired_state(t, st)
                target = np.concatenate([np.array(tp, float), np.array(tv, float), np.array(ta, float)])
                trk.desired(t, st.position, st.velocity, target, record(sm))
                raw = np.array(sm._interpolate_trajectory(t, traj(cur), cur_start)[0], float)
                cmd = ctrl.compute_control(st, target[0:3].copy(), target[3:6].copy(), target[6:9].copy())
                for nm, v in (("pos", st.position), ("vel", st.velocity), ("att", st.attitude), ("omega", st.angular_velocity), ("t", t),
                              ("thrust", float(cmd.thrust)), ("torque", np.array(cmd.torque, float)), ("target", target), ("raw", raw), ("sm_state", record(sm))):
                    log[nm].append(np.array(v, float))
                st = sim.step(st, cmd, SIM_DT)
            key = f"l_{tag}_"
            for nm in ("pos", "vel", "att", "omega", "t", "thrust", "torque", "target", "update_t"):
                out[key + nm] = np.array(log[nm])
            out[key + "sm_final"] = log["sm_state"][-1]
            out[key + "final"] = np.concatenate([st.position, st.velocity, st.attitude, st.angular_velocity, [st.timestamp]])
            for pi, (ts, P, V, A) in enumerate(plans):
                out[f"{key}pl{pi}_ts"], out[f"{key}pl{pi}_P"], out[f"{key}pl{pi}_V"] = ts, P, V
                if A is not None:
                    out[f"{key}pl{pi}_A"] = A
            tg, raw = np.array(log["target"])[:, 0:3], np.array(log["raw"])
            jump = lambda x: float(np.max(np.linalg.norm(np.diff(x, axis=0), axis=1)))
            meta["loops"].append(dict(key=key, tag=tag, nsteps=300, sim_dt=SIM_DT, plan_dt=PLAN_DT, rows=rows, wind=wind, p0=list(p0),
                                      smoothed_jump=jump(tg), raw_jump=jump(raw)))

        v = (0.5, 0.2, 0.0)
        at = lambda p, k: tuple(np.array(p) + np.array(v) * 0.1 * k)
        closed_loop("steady", [at((0, 0, 1), 0), at((0, 0, 1), 1), at((0, 0, 1), 2)], [v, v, v], (0, 0, 1))
        closed_loop("switch", [at((0, 0, 1), 0), at((2, 1, 1), 1), at((2, 1, 1), 2)], [v, v, v], (0, 0, 1))
        closed_loop("velocity_switch", [at((0, 0, 1), 0), at((0, 0, 1), 1), (0.25, 0.07, 1.0)], [v, (2.0, 0.2, 0.0), (2.0, 0.2, 0.0)], (0, 0, 1))
        closed_loop("wind_six_rows", [at((1, 1, 2), 0), at((1, 1, 2), 1), at((1, 1, 2), 2)], [v, v, v], (1, 1, 2), wind=[0.5, 0.0, 0.0], rows=6, with_a=False)
        sw = [l for l in meta["loops"] if l["tag"] == "switch"][0]
        assert sw["smoothed_jump"] < 0.25 * sw["raw_jump"], sw

        meta["hits"] = {"branch": hits["branch"].tolist(), "clamps": dict(zip(so.CLAMPS, hits["clamps"].tolist()))}
        meta["margin"] = MARGIN
        assert hits["branch"].min() >= 5 and hits["clamps"].min() >= 5, meta["hits"]
        assert worst["margin"] >= MARGIN, worst
        assert worst["oracle_error"] <= 1e-10, worst
        assert len(meta["sequences"]) >= 12

        np.savez_compressed(os.path.join(OUT_DIR, "smoother_cases.npz"), **out)
        with open(os.path.join(OUT_DIR, "smoother_cases.json"), "w") as f:
            json.dump(meta, f, indent=1)
        print("wrote smoother_cases.npz / .json:", len(meta["sequences"]), "sequences,", len(meta["loops"]), "closed loops; hits", meta["hits"],
              "smallest margin %.3g" % worst["margin"], "oracle error %.3g" % worst["oracle_error"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
