#!/usr/bin/env python3
"""Golden vectors for the MotorMixer and the motor model, produced by RUNNING THE REFERENCE'S OWN CLASSES in the build
container (/root/reference/src/dart_planner/hardware/motor_mixer.py, motor_model.py, pixhawk_interface.py) with the identity-units stand-in of
make_golden.py, an empty stand-in for the MAVLink package the Pixhawk module imports, and logging replaced by a recorder (the overrun and
all-idle tests of mix_commands are visible only as log lines):

* the mixing matrix and its "inverse" of the X factory at three arm lengths and of the plus factory (rank 3: np.linalg.solve raises and the class falls back to np.linalg.pinv);
* call sequences on fresh mixers: 40 ``mix_commands`` each, every one followed by ``get_control_allocation`` and the model's three forward
  functions on the returned PWMs; after EVERY call the record (saturation_events, last_motor_commands) and what the call did (RuntimeError,
  the two log lines, the counter's step) are stored;
* ``_convert_to_body_rate_cmd`` on 40 commands;
* closed loops of the reference's ``GeometricController``, ``MotorMixer``, the model's forward functions, B @ F and ``DroneSimulator.step`` at
  1 kHz: hover, a climb whose command reaches the controller's thrust limit, the smoother's switching scene with the smoother in front, and
  hover with motor 0 at health 0.5.

The generator asserts (through tests/mixer_oracle.py, which it also compares to the reference call by call) that every branch of
pwm_from_thrust and every flag occurs at least 5 times and that every discontinuous decision keeps a relative margin of 1e-3 from its
threshold, so that neither float32 nor a last-bit difference of a BLAS product can flip a case.  Only inputs and outputs of the reference go
into the files.  Writes mixer_cases.npz / .json.
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
import mixer_oracle as mo  # noqa: E402

MARGIN = 1e-3
CALLS = 40


class LogRecorder:
    """Stands in for the mixer module's logger: keeps the messages of one call."""
    def __init__(self):
        self.lines = []

    def warning(self, msg, *a, **k):
        self.lines.append(str(msg))

    error = warning

    def info(self, *a, **k):
        pass

    debug = info


def main():
    tmp = _install_standins()
    try:
        os.makedirs(os.path.join(tmp, "pymavlink"))
        with open(os.path.join(tmp, "pymavlink", "__init__.py"), "w") as f:
            f.write("mavutil = None\n")
        import logging
        logging.disable(logging.CRITICAL)
        import dart_planner.hardware.motor_mixer as mx_mod
        from dart_planner.hardware.motor_mixer import (MotorMixer, MotorMixingConfig, QuadrotorLayout, create_x_configuration_mixer,
                                                       create_plus_configuration_mixer)
        from dart_planner.hardware.motor_model import MotorParameters, QuadraticMotorModel
        from dart_planner.hardware.pixhawk_interface import PixhawkInterface, HardwareConfig
        import dart_planner.control.trajectory_smoother as sm_mod
        from dart_planner.control.trajectory_smoother import TrajectorySmoother
        from dart_planner.control.geometric_controller import GeometricController
        from dart_planner.utils.drone_simulator import DroneSimulator
        from dart_planner.common.types import DroneState, Trajectory

        rec_log = LogRecorder()
        mx_mod.logger = rec_log
        clock = {"t": 0.0}
        sm_mod.time.time = lambda: clock["t"]
        rng = np.random.default_rng(20261019)
        out, meta = {}, {"sequences": [], "loops": [], "matrices": []}
        hits = {"branch": np.zeros(len(mo.BRANCHES), int), "flags": np.zeros(len(mo.FLAG_NAMES), int)}
        worst = {"margin": np.inf, "oracle_error": 0.0}

        # ------------------------------------------------------------------ A. matrices
        for tag, mk in (("x_0.10", lambda: create_x_configuration_mixer(0.10)), ("x_0.15", lambda: create_x_configuration_mixer(0.15)),
                        ("x_0.25", lambda: create_x_configuration_mixer(0.25)), ("plus_0.15", lambda: create_plus_configuration_mixer(0.15))):
            m = mk()
            out[f"mat_{tag}_B"], out[f"mat_{tag}_inverse"] = np.array(m.mixing_matrix, float), np.array(m.inverse_matrix, float)
            meta["matrices"].append(dict(tag=tag, positions=m.config.motor_positions, directions=m.config.motor_directions,
                                         rank=int(np.linalg.matrix_rank(m.mixing_matrix)), cond=float(np.linalg.cond(m.mixing_matrix))))

        # ------------------------------------------------------------------ B. call sequences
        def oracle_params(mixer, **pix):
            motors = [{k: getattr(mixer.motor_model.motor_parameters[i], k) for k in mo.MOTOR_FIELDS} for i in range(4)]
            return mo.params(mixer.mixing_matrix, mixer.inverse_matrix, motors, mixer.config.pwm_min, mixer.config.pwm_max, mixer.config.pwm_idle, **pix)

        def model_of(motors):
            return QuadraticMotorModel({i: MotorParameters(motor_id=i, direction=(1, -1, 1, -1)[i], **m) for i, m in enumerate(motors)})

        def x_mixer(arm=0.15, motors=None, **cfg):
            x = arm * 0.707
            return MotorMixer(MotorMixingConfig(layout=QuadrotorLayout.X_CONFIGURATION, motor_positions=[[x, -x, 0.0], [x, x, 0.0], [-x, x, 0.0], [-x, -x, 0.0]],
                                                motor_directions=[1, -1, 1, -1], arm_length=arm, motor_model=None if motors is None else model_of(motors), **cfg))

        def one_call(mixer, p, state, thrust, torque):
            """mix_commands on the reference and on the oracle -> what the reference did, as stored."""
            rec_log.lines = []
            before = mixer.saturation_events
            raised = False
            try:
                pwm = np.array(mixer.mix_commands(float(thrust), np.array(torque, float)), float)
            except RuntimeError:
                raised, pwm = True, np.full(4, np.nan)
            flags = ((mo.NEGATIVE_THRUST if thrust < 0 else 0) | (mo.NON_FINITE if raised else 0)
                     | (mo.OVERRUN if any("110%" in l for l in rec_log.lines) else 0) | (mo.SATURATION_EVENT if mixer.saturation_events > before else 0)
                     | (mo.ALL_IDLE if any("All motors at idle" in l for l in rec_log.lines) else 0)
                     | (mo.WATCHDOG if (not raised and mixer.saturation_events > p["watchdog_threshold"]) else 0))
            d = {}
            opwm, oflags = mo.mix(p, state, np.array([thrust], float), np.array([torque], float), diag=d)
            record = np.concatenate([[mixer.saturation_events], np.array(mixer.last_motor_commands, float)])
            assert int(oflags[0]) == flags, (thrust, torque, int(oflags[0]), flags)
            assert np.array_equal(np.isnan(opwm[0]), np.isnan(pwm))
            err = 0.0 if raised else float(np.max(np.abs(opwm[0] - pwm)))
            err = max(err, float(np.max(np.abs(state[0] - record))))
            worst["oracle_error"] = max(worst["oracle_error"], err)
            worst["margin"] = min(worst["margin"], float(d["margin"][0]))
            if not raised:
                for br in d["branch"][0]:
                    hits["branch"][br] += 1
            for i in range(len(mo.FLAG_NAMES)):
                hits["flags"][i] += (flags >> i) & 1
            return pwm, flags, record, raised

        def sequence(tag, mixer, draw, **pix):
            """40 commands from draw(k) -> (thrust, torque), redrawn until the row keeps MARGIN from every threshold."""
            p = oracle_params(mixer, **pix)
            state = mo.reset(1)
            ev = {k: [] for k in ("thrust", "torque", "pwm", "flags", "state", "allocation", "motor_thrust", "motor_torque", "motor_rpm")}
            for k in range(CALLS):
                for _ in range(1000):
                    thrust, torque = draw(k)
                    if mo.margin(p, state, np.array([thrust], float), np.array([torque], float))[0] >= MARGIN:
                        break
                else:
                    raise AssertionError(f"{tag}: no command with the margin at call {k}")
                pwm, flags, record, raised = one_call(mixer, p, state, thrust, torque)
                # the model's forward functions and get_control_allocation at the PWMs the call returned (the record's after a RuntimeError)
                q = np.array(mixer.last_motor_commands, float)
                mt = np.array([mixer.motor_model.thrust_from_pwm(float(q[i]), i) for i in range(4)], float)
                mq = np.array([mixer.motor_model.torque_from_pwm(float(q[i]), i) for i in range(4)], float)
                mr = np.array([mixer.motor_model.rpm_from_pwm(float(q[i]), i) for i in range(4)], float)
                al = np.array(mixer.get_control_allocation(q), float)
                rb = mo.readback(p, q[None])
                worst["oracle_error"] = max(worst["oracle_error"], float(np.max(np.abs(rb["motor_thrust"][0] - mt))), float(np.max(np.abs(rb["motor_torque"][0] - mq))),
                                            float(np.max(np.abs(rb["motor_rpm"][0] - mr)) / 1e4), float(np.max(np.abs(rb["allocation"][0] - al))))
                for nm, v in (("thrust", thrust), ("torque", torque), ("pwm", pwm), ("flags", flags), ("state", record), ("allocation", al),
                              ("motor_thrust", mt), ("motor_torque", mq), ("motor_rpm", mr)):
                    ev[nm].append(np.array(v))
            key = f"q{len(meta['sequences']):02d}_"
            for nm, v in ev.items():
                out[key + nm] = np.array(v)
            out[key + "B"], out[key + "inverse"] = p["mixing"], p["inverse"]
            out[key + "motors"] = np.array([p[k] for k in mo.MOTOR_FIELDS])                  # (9, 4)
            meta["sequences"].append(dict(key=key, tag=tag, calls=CALLS, config_pwm_min=p["config_pwm_min"], config_pwm_max=p["config_pwm_max"],
                                          config_pwm_idle=p["config_pwm_idle"], max_thrust=p["max_thrust"], body_rate_scale=p["body_rate_scale"],
                                          watchdog_threshold=p["watchdog_threshold"], final_events=int(mixer.saturation_events)))

        U = rng.uniform
        tq = lambda s, sz=0.02: np.array([U(-s, s), U(-s, s), U(-sz, sz)])
        default = dict(mo.DEFAULT_MOTOR)
        sequence("default_hover_band", create_x_configuration_mixer(0.15), lambda k: (U(5.0, 13.0), tq(0.15)))
        sequence("default_aggressive_to_20N", create_x_configuration_mixer(0.15), lambda k: (20.0 if k % 8 == 0 else U(0.5, 22.0), tq(1.0, 0.3)))
        sequence("default_low_and_negative_thrust", create_x_configuration_mixer(0.15), lambda k: (U(-3.0, 0.6) if k % 2 else U(0.25, 0.38), tq(0.0, 0.0) if k % 4 == 0 else tq(0.01, 0.002)))
        sequence("motor_limit_above_the_config", x_mixer(motors=[dict(default, pwm_max=1.3)] * 4), lambda k: (U(8.0, 26.0), tq(0.8, 0.2)))
        sequence("discriminant_negative_asks_full_pwm", x_mixer(motors=[dict(default, thrust_c=0.5, thrust_b=0.2)] * 4), lambda k: (U(0.3, 6.0), tq(0.15, 0.05)))
        sequence("linear_motors", x_mixer(motors=[dict(default, thrust_a=0.0, thrust_b=4.0)] * 4), lambda k: (U(0.0, 18.0), tq(0.5, 0.1)))
        sequence("one_dead_one_linear_motor", x_mixer(motors=[default, dict(default, thrust_a=0.0, thrust_b=3.5, thrust_c=0.0), dict(default, thrust_a=0.0, thrust_b=0.0, thrust_c=0.0), default]),
                 lambda k: (U(1.0, 12.0), tq(0.4, 0.1)))
        sequence("model_idle_below_config_idle", x_mixer(motors=[dict(default, pwm_idle=0.05)] * 4, pwm_idle=0.12), lambda k: (U(-0.5, 4.0), tq(0.3, 0.05)))
        sequence("model_idle_above_config_idle", x_mixer(motors=[dict(default, pwm_idle=0.2, pwm_min=0.02)] * 4, pwm_idle=0.1, pwm_min=0.05), lambda k: (U(-0.5, 5.0), tq(0.3, 0.05)))
        sequence("plus_factory_with_lapack_s_inverse", create_plus_configuration_mixer(0.15), lambda k: (U(2.0, 16.0), tq(0.4, 0.1)))
        bad = [np.nan, np.inf, -np.inf]
        sequence("non_finite_commands", create_x_configuration_mixer(0.25),
                 lambda k: (bad[k % 3] if k % 5 == 0 else U(1.0, 12.0), np.array([bad[k % 3], 0.1, 0.0]) if k % 5 == 2 else tq(0.3, 0.05)))
        sequence("mixed_motors_past_the_watchdog", x_mixer(arm=0.25, motors=[dict(default, thrust_a=2.2, pwm_max=1.2), dict(default, thrust_b=1.0, thrust_c=0.3, pwm_idle=0.08),
                                                                            dict(default, thrust_a=3.0, rpm_coefficient=9000.0, rpm_offset=-200.0), dict(default, torque_coefficient=2e-7)]),
                 lambda k: (U(0.0, 20.0), tq(1.0, 0.3)))
        sequence("narrow_config_band", x_mixer(motors=[default] * 4, pwm_min=0.15, pwm_max=0.9, pwm_idle=0.1), lambda k: (U(0.0, 18.0), tq(0.6, 0.1)), watchdog_threshold=3.5)

        # ------------------------------------------------------------------ C. _convert_to_body_rate_cmd
        class Stub:
            config = HardwareConfig()
        stub = Stub()
        mixer = create_x_configuration_mixer(arm_length=0.15)                     # what pixhawk_interface.py:461 builds on first use
        stub._motor_mixer = mixer
        p = oracle_params(mixer, max_thrust=Stub.config.max_thrust, watchdog_threshold=float(Stub.config.saturation_watchdog_threshold))
        state = mo.reset(1)
        rows = {k: [] for k in ("thrust", "torque", "pwm", "out", "state")}
        for k in range(CALLS):
            while True:
                thrust, torque = (U(-2.0, 16.0), tq(0.6, 0.15))
                if mo.margin(p, state, np.array([thrust]), np.array([torque]))[0] >= MARGIN and abs(thrust - 10.0) > 1e-2:
                    break
            cmd = PixhawkInterface._convert_to_body_rate_cmd(stub, float(thrust), np.array(torque, float))
            opwm, _ = mo.mix(p, state, np.array([thrust]), np.array([torque]))
            res = np.concatenate([[float(cmd.thrust)], np.array(cmd.body_rates, float)])
            worst["oracle_error"] = max(worst["oracle_error"], float(np.max(np.abs(mo.body_rate(p, np.array([thrust]), opwm)[0] - res))))
            for nm, v in (("thrust", thrust), ("torque", torque), ("pwm", np.array(mixer.last_motor_commands, float)), ("out", res),
                          ("state", np.concatenate([[mixer.saturation_events], np.array(mixer.last_motor_commands, float)]))):
                rows[nm].append(np.array(v, float))
        for nm, v in rows.items():
            out["br_" + nm] = np.array(v)
        meta["body_rate"] = dict(max_thrust=Stub.config.max_thrust, body_rate_scale=2.0, watchdog_threshold=float(Stub.config.saturation_watchdog_threshold),
                                 tripped_after=int(np.argmax(np.array(rows["state"])[:, 0] > Stub.config.saturation_watchdog_threshold)))

        # ------------------------------------------------------------------ D. closed loops at 1 kHz
        T0, SIM_DT, PLAN_DT = 1000.0, 0.001, 0.01371

        def mkstate(t, p_, v_, a=(0, 0, 0), w=(0, 0, 0)):
            return DroneState(timestamp=float(t), position=np.array(p_, float), velocity=np.array(v_, float), attitude=np.array(a, float),
                              angular_velocity=np.array(w, float))

        def traj(plan):
            ts, P, V, A = plan
            return Trajectory(timestamps=np.array(ts, float), positions=np.array(P, float), velocities=np.array(V, float), accelerations=np.array(A, float))

        def line_plan(rows_, p0, v, t_first):
            k = np.arange(rows_)[:, None] * PLAN_DT
            return (t_first + np.arange(rows_) * PLAN_DT, np.asarray(p0, float) + np.asarray(v, float) * k, np.broadcast_to(np.asarray(v, float), (rows_, 3)).copy(),
                    np.zeros((rows_, 3)))

        def closed_loop(tag, nsteps, p0, hold=None, starts=None, vels=None, health=None, actuated=True):
            """hold: a standing target (a two-row plan of equal rows: every sampler returns it); starts / vels: the smoother's three plans."""
            mixer = create_x_configuration_mixer(0.15)
            p = oracle_params(mixer)
            state = mo.reset(1)
            ctrl = GeometricController(tuning_profile="sitl_optimized")
            sim = DroneSimulator()
            sm = TrajectorySmoother() if hold is None else None
            st = mkstate(T0, p0, (0, 0, 0))
            h = np.ones(4) if health is None else np.array(health, float)
            log = {k: [] for k in ("pos", "vel", "att", "omega", "t", "thrust", "torque", "target", "pwm", "wrench", "flags")}
            plans = []
            for i in range(nsteps):
                t = st.timestamp
                if sm is not None and i % 100 == 0:
                    plan = line_plan(30, starts[i // 100], vels[i // 100], t)
                    plans.append(plan)
                    clock["t"] = t
                    sm.update_trajectory(traj(plan), st)
                if sm is not None:
                    tp, tv, ta = sm.get_desired_state(t, st)
                    target = np.concatenate([np.array(tp, float), np.array(tv, float), np.array(ta, float)])
                else:
                    target = np.concatenate([np.array(hold, float), np.zeros(6)])
                cmd = ctrl.compute_control(st, target[0:3].copy(), target[3:6].copy(), target[6:9].copy())
                thrust, torque = float(cmd.thrust), np.array(cmd.torque, float)
                if actuated:
                    assert mo.margin(p, state, np.array([thrust]), torque[None])[0] >= MARGIN, (tag, i)
                    pwm, flags, _, raised = one_call(mixer, p, state, thrust, torque)
                    assert not raised
                    F = h * np.array([mixer.motor_model.thrust_from_pwm(float(pwm[j]), j) for j in range(4)])
                    wrench = mixer.mixing_matrix @ F
                    real = type(cmd)(thrust=float(wrench[0]), torque=np.array(wrench[1:4], float))
                else:
                    pwm, flags, wrench, real = np.full(4, np.nan), 0, np.concatenate([[thrust], torque]), cmd
                for nm, v in (("pos", st.position), ("vel", st.velocity), ("att", st.attitude), ("omega", st.angular_velocity), ("t", t), ("thrust", thrust),
                              ("torque", torque), ("target", target), ("pwm", pwm), ("wrench", wrench), ("flags", flags)):
                    log[nm].append(np.array(v, float))
                st = sim.step(st, real, SIM_DT)
            final = np.concatenate([st.position, st.velocity, st.attitude, st.angular_velocity, [st.timestamp]])
            if not actuated:
                return final
            key = f"l_{tag}_"
            for nm, v in log.items():
                out[key + nm] = np.array(v)
            out[key + "final"] = final
            out[key + "mixer_final"] = np.concatenate([[mixer.saturation_events], np.array(mixer.last_motor_commands, float)])
            for pi, (ts, P, V, A) in enumerate(plans):
                out[f"{key}pl{pi}_ts"], out[f"{key}pl{pi}_P"], out[f"{key}pl{pi}_V"], out[f"{key}pl{pi}_A"] = ts, P, V, A
            entry = dict(key=key, tag=tag, nsteps=nsteps, sim_dt=SIM_DT, p0=list(p0), hold=None if hold is None else list(hold), plans=len(plans),
                         health=None if health is None else list(health), max_command=float(np.max(log["thrust"])), max_realised=float(np.max(np.array(log["wrench"])[:, 0])),
                         events=int(mixer.saturation_events), controller_max_thrust=float(ctrl.config.max_thrust))
            meta["loops"].append(entry)
            return final

        closed_loop("hover", 300, (0.0, 0.0, 1.0), hold=(0.05, -0.03, 1.02))
        climb = closed_loop("climb", 300, (0.0, 0.0, 1.0), hold=(0.1, 0.0, 4.0))
        free = closed_loop("climb", 300, (0.0, 0.0, 1.0), hold=(0.1, 0.0, 4.0), actuated=False)
        cl = meta["loops"][-1]
        cl["final_altitude"], cl["unactuated_final_altitude"] = float(climb[2]), float(free[2])
        assert cl["max_command"] == cl["controller_max_thrust"] and cl["max_realised"] <= 15.2 + 1e-9 and cl["events"] == 0 and climb[2] < free[2], cl
        v = (0.5, 0.2, 0.0)
        at = lambda p_, k: tuple(np.array(p_) + np.array(v) * 0.1 * k)
        closed_loop("smoothed_switch", 300, (0.0, 0.0, 1.0), starts=[at((0, 0, 1), 0), at((2, 1, 1), 1), at((2, 1, 1), 2)], vels=[v, v, v])
        closed_loop("hover_motor0_half", 300, (0.0, 0.0, 1.0), hold=(0.0, 0.0, 1.0), health=(0.5, 1.0, 1.0, 1.0))

        meta["hits"] = {"branch": dict(zip(mo.BRANCHES, hits["branch"].tolist())), "flags": dict(zip(mo.FLAG_NAMES, hits["flags"].tolist()))}
        meta["margin"] = MARGIN
        assert hits["branch"].min() >= 5 and hits["flags"].min() >= 5, meta["hits"]
        assert worst["margin"] >= MARGIN, worst
        assert worst["oracle_error"] <= 1e-10, worst
        assert len(meta["sequences"]) >= 12

        np.savez_compressed(os.path.join(OUT_DIR, "mixer_cases.npz"), **out)
        with open(os.path.join(OUT_DIR, "mixer_cases.json"), "w") as f:
            json.dump(meta, f, indent=1)
        print("wrote mixer_cases.npz / .json:", len(meta["sequences"]), "sequences,", len(meta["loops"]), "closed loops; hits", meta["hits"],
              "smallest margin %.3g" % worst["margin"], "oracle error %.3g" % worst["oracle_error"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
