#!/usr/bin/env python3
"""Golden vectors for the reference's edge loop, produced by RUNNING THE REFERENCE'S OWN CLASSES in the build container
(/root/reference/src/dart_planner: utils/pid_controller.py, control/onboard_controller.py, utils/latency_buffer.py, utils/drone_simulator.py)
with the identity-units stand-in of make_golden.py, logging disabled and the latency module's ``time.time`` pinned to the pushed state's
timestamp (push reads the wall clock when it is handed none, latency_buffer.py:65-66):

* call sequences on fresh controllers and buffers: after EVERY ``compute_control_command`` / ``get_fallback_command`` / ``push`` call the
  returned values and every member of the records (SE3MPC_ONBOARD_STATE_WORDS, SE3MPC_LATENCY_STATE_WORDS, include/se3mpc.h);
* the private methods' returns at recorded arguments (``_compute_desired_attitude_and_thrust``, ``_compute_torque``, ``plan``, ``act``);
* ``LatencyBuffer(d, 0.005).buffer_size`` for a list of delays;
* closed loops of edge/main.py's body (:80-95) at depth 0, 1, 2, 5 and 9, 300 steps at 10 ms, with a plan, without one, and with the plan
  replaced every 100 steps.

The generator compares tests/edge_oracle.py to the reference call by call, asserts that every branch (edge_oracle.BRANCHES) is met at least
5 times and that every clamp / clip decision keeps a relative margin of 1e-6 from its threshold.  Only inputs and outputs of the reference go
into the files.  Writes edge_cases.npz / .json.
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
import edge_oracle as eo  # noqa: E402

MARGIN = 1e-6
PID_NAMES = ("pos_x_pid", "pos_y_pid", "pos_z_pid", "roll_pid", "pitch_pid", "yaw_rate_pid")


def main():
    tmp = _install_standins()
    try:
        import logging
        logging.disable(logging.CRITICAL)
        import dart_planner.utils.latency_buffer as lat_mod
        from dart_planner.utils.latency_buffer import DroneStateLatencyBuffer, LatencyBuffer
        from dart_planner.utils.pid_controller import PIDController
        from dart_planner.control.onboard_controller import OnboardController
        from dart_planner.utils.drone_simulator import DroneSimulator
        from dart_planner.common.types import DroneState, Trajectory

        clock = {"t": 0.0}
        lat_mod.time.time = lambda: clock["t"]
        rng = np.random.default_rng(20261019)
        out, meta = {}, {"sequences": [], "pushes": [], "loops": []}
        hits = np.zeros(len(eo.BRANCHES), int)
        worst = {"margin": np.inf, "oracle_error": 0.0}

        def mkstate(t, x):
            x = np.asarray(x, float)
            return DroneState(timestamp=float(t), position=x[0:3].copy(), velocity=x[3:6].copy(), attitude=x[6:9].copy(), angular_velocity=x[9:12].copy())

        def x_of(s):
            return np.concatenate([np.asarray(s.position, float), np.asarray(s.velocity, float), np.asarray(s.attitude, float), np.asarray(s.angular_velocity, float)])

        def record(c):
            pids = [getattr(c, n) for n in PID_NAMES]
            return np.array([float(p.integral) for p in pids] + [float(p.last_error) for p in pids]
                            + [0.0 if c.last_time is None else float(c.last_time), 0.0 if c.last_time is None else 1.0])

        def lat_record(b):
            return np.array([len(b.buffer), b.total_samples, b.missed_samples, b.actual_delay_s, b.last_timestamp], float)

        def traj(plan):
            ts, P, V, A = plan
            return Trajectory(timestamps=np.array(ts, float), positions=np.array(P, float), velocities=None if V is None else np.array(V, float),
                              accelerations=None if A is None else np.array(A, float))

        def line_plan(N, dt, p0, v, a=(0, 0, 0), t_first=100.0, with_v=True, with_a=True, wobble=0.0):
            k = np.arange(N)[:, None] * dt
            a = np.asarray(a, float)
            P = np.asarray(p0, float) + np.asarray(v, float) * k + 0.5 * a * k * k + wobble * rng.normal(0, 1, (N, 3))
            V = np.asarray(v, float) + a * k
            A = np.broadcast_to(a, (N, 3)) + wobble * rng.normal(0, 1, (N, 3))
            return (t_first + np.arange(N) * dt, P, V if with_v else None, np.array(A) if with_a else None)

        def put_plan(key, plan):
            ts, P, V, A = plan
            out[key + "_ts"], out[key + "_P"] = np.array(ts, float), np.array(P, float)
            if V is not None:
                out[key + "_V"] = np.array(V, float)
            if A is not None:
                out[key + "_A"] = np.array(A, float)

        def oracle_params(c):
            return eo.params(mass=c.mass, g=c.g, pid=np.array([[p.Kp, p.Ki, p.Kd, p.integral_limit or 0.0] for p in (getattr(c, n) for n in PID_NAMES)]))

        def track(d, live=True):
            hits[:] += d["hits"][0]
            worst["margin"] = min(worst["margin"], float(d["margin"][0]))

        # ------------------------------------------------------------------ A. controller call sequences
        def sequence(tag, plan, calls, gains=None, mass=1.0, g=9.81):
            """calls: [(t, x12, use_plan)]; use_plan False = get_fallback_command (no plan yet)."""
            c = OnboardController(mass=mass, g=g)
            for name, (kp, ki, kd, lim) in (gains or {}).items():
                setattr(c, name, PIDController(kp, ki, kd, integral_limit=lim))
            ost = eo.onboard_reset(1)
            ev = {k: [] for k in ("t", "x", "use_plan", "thrust", "torque", "target", "record")}
            for t, x, use_plan in calls:
                s = mkstate(t, x)
                if use_plan:
                    cmd, tg = c.compute_control_command(s, traj(plan))
                    thrust, torque, tg = float(cmd.thrust), np.array(cmd.torque, float), np.array(tg, float)
                else:
                    cmd = c.get_fallback_command(s)
                    thrust, torque, tg = float(cmd.thrust), np.array(cmd.torque, float), np.array(s.position, float)
                rec = record(c)
                d = {}
                oth, otq, otg = eo.control(oracle_params(c), ost, np.array([float(t)]), x[None, 0:3], x[None, 6:9], x[None, 9:12], plan if use_plan else None, diag=d)
                track(d)
                worst["oracle_error"] = max(worst["oracle_error"], abs(oth[0] - thrust), float(np.max(np.abs(otq[0] - torque))), float(np.max(np.abs(otg[0] - tg))),
                                            float(np.max(np.abs(ost[0] - rec))))
                for nm, v in (("t", t), ("x", x), ("use_plan", int(use_plan)), ("thrust", thrust), ("torque", torque), ("target", tg), ("record", rec)):
                    ev[nm].append(np.array(v, float))
            key = f"q{len(meta['sequences']):02d}_"
            for nm, v in ev.items():
                out[key + nm] = np.array(v)
            put_plan(key + "plan", plan)
            meta["sequences"].append(dict(key=key, tag=tag, calls=len(calls), mass=mass, g=g,
                                          pid=[[p.Kp, p.Ki, p.Kd, p.integral_limit or 0.0] for p in (getattr(c, n) for n in PID_NAMES)]))

        def walk(n, t0, dt, x0, step_scale, t_jitter=None, fallback_first=0):
            """n calls every dt from t0 on a random walk of the state; t_jitter: {call index: clock offset} (a negative one steps the clock back)."""
            calls, x = [], np.array(x0, float)
            for k in range(n):
                x = x + rng.normal(0, 1, 12) * step_scale
                t = t0 + k * dt + (t_jitter or {}).get(k, 0.0)
                calls.append((t, x.copy(), k >= fallback_first))
            return calls

        x0 = np.array([0.0, 0.0, 1.0, 0, 0, 0, 0.02, -0.01, 0.3, 0, 0, 0.1])
        sc = np.array([0.02] * 3 + [0.05] * 3 + [0.01] * 3 + [0.05] * 3)
        sequence("hover_near_the_plan", line_plan(30, 0.1, (0, 0, 1), (0.3, 0.1, 0.0), a=(0.1, 0.0, 0.05), t_first=100.05), walk(60, 100.0, 0.01, x0, sc))
        sequence("far_below_target_integrals_clamp", line_plan(6, 0.05, (40, -35, 60), (0.0, 0.0, 0.0), with_a=False, t_first=99.0), walk(40, 100.0, 0.01, x0, sc))
        sequence("far_above_target_thrust_clipped", line_plan(6, 0.05, (-30, 45, -50), (0.0, 0.0, 0.0), with_v=False, with_a=False, t_first=100.1),
                 walk(40, 100.0, 0.01, x0, sc))
        sequence("clock_steps_back_and_repeats", line_plan(2, 0.2, (0.2, 0.1, 1.1), (0.5, 0.0, 0.0), t_first=100.1),
                 walk(50, 100.0, 0.01, x0, sc, t_jitter={5: -0.06, 6: -0.01, 12: -0.01, 20: -0.5, 21: -0.5, 30: -0.02, 31: -0.01, 40: -0.3}))
        sequence("one_row_plan_spinning", line_plan(1, 0.1, (0.5, -0.5, 1.5), (0, 0, 0)),
                 walk(40, 100.0, 0.01, x0 + np.array([0, 0, 0, 0, 0, 0, 0.4, -0.5, 2.0, 0.5, -0.5, 9.0]), sc))
        sequence("fallback_then_plan", line_plan(6, 0.05, (0.1, 0.0, 1.2), (0.2, 0.2, 0.0), t_first=100.0), walk(40, 100.0, 0.01, x0, sc, fallback_first=10))
        sequence("no_integral_limit_other_mass", line_plan(30, 0.02, (1, 1, 3), (0.5, -0.5, 0.2), wobble=0.01, t_first=99.9), walk(50, 100.0, 0.01, x0, sc),
                 gains={"pos_x_pid": (6.0, 2.0, 1.0, None), "roll_pid": (5.0, 1.0, 0.5, 0.05), "yaw_rate_pid": (3.0, 0.5, 0.2, 0.01)}, mass=1.4, g=9.80665)
        sequence("irregular_clock", line_plan(6, 0.07, (0, 0, 1), (1.0, 0.5, 0.0), a=(0.0, 0.2, 0.0), t_first=100.02),
                 walk(50, 100.0, 0.0137, x0, sc, t_jitter={k: float(rng.uniform(-0.004, 0.004)) for k in range(50)}))

        # ------------------------------------------------------------------ B. the private methods at recorded arguments
        c = OnboardController()
        accs, yaws = rng.uniform(-6, 6, (10, 3)) * np.array([1, 1, 2.5]), rng.uniform(-3, 3, 10)
        out["m_att_acc"], out["m_att_yaw"] = accs, yaws
        out["m_att_out"] = np.array([c._compute_desired_attitude_and_thrust(a, float(y)) for a, y in zip(accs, yaws)], float)
        xs, dts = x0 + rng.normal(0, 1, (8, 12)) * 0.3, rng.uniform(0.005, 0.02, 8)
        sets = rng.uniform(-0.5, 0.5, (8, 2))
        out["m_torque_x"], out["m_torque_dt"], out["m_torque_set"] = xs, dts, sets
        tq, recs = [], []
        for x, dt, (r, p) in zip(xs, dts, sets):
            tq.append(np.array(c._compute_torque(float(r), float(p), 0.0, mkstate(0.0, x), float(dt)), float)); recs.append(record(c))
        out["m_torque_out"], out["m_torque_record"] = np.array(tq), np.array(recs)
        c = OnboardController()
        tps, tas = xs[:, 0:3] + rng.normal(0, 0.5, (8, 3)), rng.normal(0, 1.0, (8, 3))
        out["m_plan_tp"], out["m_plan_ta"] = tps, tas
        pl, recs = [], []
        for x, dt, tp, ta in zip(xs, dts, tps, tas):
            pl.append(np.array(c.plan(mkstate(0.0, x), tp, ta, float(dt)), float)); recs.append(record(c))
        out["m_plan_out"], out["m_plan_record"] = np.array(pl), np.array(recs)
        c = OnboardController()
        act, recs = [], []
        for x, dt, (r, p), th in zip(xs, dts, sets, rng.uniform(0, 15, 8)):
            cmd = c.act(mkstate(0.0, x), float(r), float(p), float(th), float(dt))
            act.append(np.concatenate([[float(cmd.thrust)], np.array(cmd.torque, float), [th]])); recs.append(record(c))
        out["m_act_out"], out["m_act_record"] = np.array(act), np.array(recs)

        # ------------------------------------------------------------------ C. buffer sizing and push sequences
        delays_ms = [1.0, 2.0, 2.5, 7.5, 12.5, 25.0, 1000.0, 5000.1]
        meta["buffer_sizes"] = {"dt": 0.005, "delays_ms": delays_ms, "sizes": [LatencyBuffer(d / 1000.0, 0.005).buffer_size for d in delays_ms]}
        assert meta["buffer_sizes"]["sizes"][:7] == [1, 1, 1, 2, 2, 5, 200], meta["buffer_sizes"]
        assert meta["buffer_sizes"]["sizes"] == [eo.buffer_size(d / 1000.0, 0.005) for d in delays_ms]
        for depth, n, reset_at in ((1, 8, None), (2, 9, None), (5, 23, 14), (9, 31, None)):
            b = DroneStateLatencyBuffer(depth * 0.005, 0.005)
            assert b.buffer_size == depth
            obuf = eo.latency_reset(1, depth)
            ev = {k: [] for k in ("t", "x", "d_t", "d_x", "record", "reset")}
            t = 50.0
            for k in range(n):
                if k == reset_at:
                    b.reset(); obuf = eo.latency_reset(1, depth)
                t += float(rng.uniform(0.004, 0.006))
                x = rng.normal(0, 1, 12)
                clock["t"] = t
                s = b.push(mkstate(t, x))
                d = {}
                dl_t, dl_x = eo.push(obuf, np.array([t]), x[None], diag=d)
                assert dl_t[0] == s.timestamp and np.array_equal(dl_x[0], x_of(s))
                rec = lat_record(b)
                assert np.array_equal(obuf["state"][0, [0, 2, 3]], rec[[0, 1, 3]]) and rec[2] == min(rec[1], depth)
                hits[0 if d["filling"][0] else 1] += 1
                for nm, v in (("t", t), ("x", x), ("d_t", s.timestamp), ("d_x", x_of(s)), ("record", rec), ("reset", float(k == reset_at))):
                    ev[nm].append(np.array(v, float))
            key = f"p{depth}_"
            for nm, v in ev.items():
                out[key + nm] = np.array(v)
            meta["pushes"].append(dict(key=key, depth=depth, pushes=n))

        # ------------------------------------------------------------------ D. closed loops of edge/main.py:80-95, 300 steps at 10 ms
        T0, SIM_DT, NSTEPS = 100.0, 0.01, 300

        def closed_loop(tag, depth, plans, p0, every=100):
            """plans: [] (no plan: the fallback throughout) or the plans that arrive at steps 0, every, 2 * every, ... (the last one stays)."""
            ctrl, sim = OnboardController(), DroneSimulator()
            ctrl.reset()
            buf = DroneStateLatencyBuffer(depth * 0.005, 0.005) if depth > 0 else None
            assert buf is None or buf.buffer_size == depth
            st = mkstate(T0, np.concatenate([p0, np.zeros(9)]))
            ost, obuf, ot, ox = eo.onboard_reset(1), eo.latency_reset(1, depth), np.array([T0]), x_of(st)[None].copy()
            log = {k: [] for k in ("t", "x", "thrust", "torque", "target", "delayed_t", "plan")}
            trajectory, pi = None, -1
            for i in range(NSTEPS):
                if plans and i % every == 0 and i // every < len(plans):
                    pi = i // every
                    trajectory = traj(plans[pi])
                if buf is not None:
                    clock["t"] = st.timestamp
                    delayed = buf.push(st)                       # edge/main.py:81-85
                else:
                    delayed = st
                if trajectory is not None:
                    cmd, target = ctrl.compute_control_command(delayed, trajectory)     # :87-90
                else:
                    cmd, target = ctrl.get_fallback_command(delayed), delayed.position   # :91-94
                for nm, v in (("t", st.timestamp), ("x", x_of(st)), ("thrust", float(cmd.thrust)), ("torque", np.array(cmd.torque, float)),
                              ("target", np.array(target, float)), ("delayed_t", delayed.timestamp), ("plan", pi)):
                    log[nm].append(np.array(v, float))
                o = eo.edge_loop(oracle_params(ctrl), eo.sim_params(), ost, obuf, ot, ox, plans[pi] if pi >= 0 else None, 1, SIM_DT)
                hits[:] += o["hits"][0, 0]
                worst["margin"] = min(worst["margin"], np.inf if not o["near"][0, 0] else 0.0)
                worst["oracle_error"] = max(worst["oracle_error"], float(np.max(np.abs(o["cmd"][0, 0] - np.concatenate([[float(cmd.thrust)], np.array(cmd.torque, float)])))),
                                            float(np.max(np.abs(o["target"][0, 0] - np.array(target, float)))), abs(o["delayed_time"][0, 0] - delayed.timestamp))
                st = sim.step(st, cmd, SIM_DT)                   # :95
                worst["oracle_error"] = max(worst["oracle_error"], float(np.max(np.abs(ox[0] - x_of(st)))), abs(ot[0] - st.timestamp))
            key = f"l_{tag}_"
            for nm, v in log.items():
                out[key + nm] = np.array(v)
            out[key + "final"] = np.concatenate([x_of(st), [st.timestamp]])
            out[key + "onboard_final"] = record(ctrl)
            if buf is not None:
                out[key + "latency_final"] = lat_record(buf)
            for i, p in enumerate(plans):
                put_plan(f"{key}pl{i}", p)
            thrust = np.array(log["thrust"])
            zero_cmd = [int(i) for i in np.flatnonzero((thrust == 0) & np.all(np.array(log["torque"]) == 0, axis=1) & np.all(np.array(log["target"]) == 0, axis=1))]
            meta["loops"].append(dict(key=key, tag=tag, depth=depth, nsteps=NSTEPS, sim_dt=SIM_DT, plans=len(plans), every=every, p0=[float(v) for v in p0],
                                      zero_command_steps=zero_cmd, zero_thrust_steps=int(np.sum(thrust == 0))))
            if plans:
                assert zero_cmd == ([depth] if depth > 0 else []), (tag, zero_cmd)      # the stale delayed state: exactly one zero command, at step index `depth`
            else:
                assert zero_cmd == []

        p0 = np.array([0.0, 0.0, 1.0])
        main_plan = lambda: line_plan(30, 0.1, (0.05, -0.03, 1.02), (0.3, 0.1, 0.05), a=(0.05, -0.02, 0.0), t_first=100.055)
        for depth in (0, 1, 2, 5, 9):
            closed_loop(f"plan_depth{depth}", depth, [main_plan()], p0)
        closed_loop("no_plan_depth0", 0, [], p0)
        closed_loop("no_plan_depth5", 5, [], p0)
        closed_loop("replanned_depth5", 5, [line_plan(6, 0.25, (0.0, 0.0, 1.0), (0.3, 0.0, 0.0), t_first=100.0, with_a=False),
                                            line_plan(6, 0.25, (0.4, 0.1, 1.1), (0.3, 0.2, 0.0), t_first=101.0),
                                            line_plan(2, 0.5, (0.7, 0.3, 1.1), (0.0, 0.2, 0.1), t_first=102.0, with_v=False)], p0)
        closed_loop("replanned_depth2", 2, [line_plan(30, 0.04, (0.0, 0.0, 1.0), (0.2, 0.2, 0.0), t_first=100.0),
                                            line_plan(30, 0.04, (0.1, 0.3, 1.0), (0.2, -0.2, 0.1), t_first=101.0)], p0)

        meta["hits"] = dict(zip(eo.BRANCHES, hits.tolist()))
        meta["margin"] = MARGIN
        assert hits.min() >= 5, meta["hits"]
        assert worst["margin"] >= MARGIN, worst
        assert worst["oracle_error"] <= 1e-10, worst

        np.savez_compressed(os.path.join(OUT_DIR, "edge_cases.npz"), **out)
        with open(os.path.join(OUT_DIR, "edge_cases.json"), "w") as f:
            json.dump(meta, f, indent=1)
        print("wrote edge_cases.npz / .json:", len(meta["sequences"]), "sequences,", len(meta["pushes"]), "push sequences,", len(meta["loops"]),
              "closed loops; hits", meta["hits"], "smallest margin %.3g" % worst["margin"], "oracle error %.3g" % worst["oracle_error"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
