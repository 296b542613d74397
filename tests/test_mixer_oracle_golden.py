"""CPU: tests/mixer_oracle.py (the float64 NumPy restatement of the reference's MotorMixer, motor model and body-rate conversion) against
tests/golden/mixer_cases.npz, the vectors of the reference's own classes: every recorded call to 1e-10 (the reference's pwm**2 goes through
pow and its matrix product through BLAS, so this is not bit-exact), flags, event counts and NaN patterns exact, and every recorded row at least
the generator's margin away from each threshold."""
import numpy as np
import pytest

import mixer_checks as xc
import mixer_oracle as mo

DATA, META = xc.golden()


@pytest.mark.parametrize("seq", META["sequences"], ids=lambda s: s["tag"])
def test_sequence(seq):
    key, p = seq["key"], xc.seq_params(DATA, seq)
    state = mo.reset(1)
    for e in range(seq["calls"]):
        thrust, torque = DATA[key + "thrust"][e][None], DATA[key + "torque"][e][None]
        assert mo.margin(p, state, thrust, torque)[0] >= META["margin"], e
        pwm, flags = mo.mix(p, state, thrust, torque)
        ref = DATA[key + "state"][e]
        assert flags[0] == DATA[key + "flags"][e] and state[0, 0] == ref[0], e
        assert np.array_equal(np.isnan(pwm[0]), np.isnan(DATA[key + "pwm"][e]))
        if not flags[0] & mo.NON_FINITE:
            assert np.max(np.abs(pwm[0] - DATA[key + "pwm"][e])) <= 1e-10, e
        assert np.max(np.abs(state[0, 1:5] - ref[1:5])) <= 1e-10, e
        rb = mo.readback(p, state[:, 1:5])
        for nm, scale in (("motor_thrust", 1.0), ("motor_torque", 1e2), ("motor_rpm", 1e4), ("allocation", 1.0)):
            assert np.max(np.abs(rb[nm][0] - DATA[key + nm][e])) <= 1e-10 * scale, (nm, e)
    assert state[0, 0] == seq["final_events"]


def test_body_rate_commands():
    br = META["body_rate"]
    p = mo.default_params(max_thrust=br["max_thrust"], body_rate_scale=br["body_rate_scale"], watchdog_threshold=br["watchdog_threshold"])
    assert np.max(np.abs(p["inverse"] - DATA["mat_x_0.15_inverse"])) <= 1e-13 and np.max(np.abs(p["mixing"] - DATA["mat_x_0.15_B"])) <= 1e-15
    state = mo.reset(1)
    for e in range(DATA["br_thrust"].shape[0]):
        pwm, _ = mo.mix(p, state, DATA["br_thrust"][e][None], DATA["br_torque"][e][None])
        assert np.max(np.abs(pwm[0] - DATA["br_pwm"][e])) <= 1e-10 and np.max(np.abs(state[0] - DATA["br_state"][e])) <= 1e-10
        assert np.max(np.abs(mo.body_rate(p, DATA["br_thrust"][e][None], pwm)[0] - DATA["br_out"][e])) <= 1e-10


@pytest.mark.parametrize("loop", META["loops"], ids=lambda l: l["tag"])
def test_loop_steps(loop):
    """Every step of a recorded closed loop: the command through the oracle's mixer and motors gives the recorded PWMs and wrench."""
    key, p = loop["key"], mo.default_params()
    state = mo.reset(1)
    health = None if loop["health"] is None else np.array(loop["health"])
    for i in range(loop["nsteps"]):
        pwm, flags = mo.mix(p, state, DATA[key + "thrust"][i][None], DATA[key + "torque"][i][None])
        assert flags[0] == DATA[key + "flags"][i] and np.max(np.abs(pwm[0] - DATA[key + "pwm"][i])) <= 1e-10
        assert np.max(np.abs(mo.readback(p, pwm, health)["wrench"][0] - DATA[key + "wrench"][i])) <= 1e-10
    assert np.max(np.abs(state[0] - DATA[key + "mixer_final"])) <= 1e-10


def test_fixtures_cover_what_the_issue_lists():
    assert len(META["sequences"]) >= 12 and all(s["calls"] == 40 for s in META["sequences"]) and len(META["loops"]) == 4
    assert min(META["hits"]["branch"].values()) >= 5 and min(META["hits"]["flags"].values()) >= 5 and META["margin"] == 1e-3
    assert [m["tag"] for m in META["matrices"]] == ["x_0.10", "x_0.15", "x_0.25", "plus_0.15"] and DATA["br_thrust"].shape[0] == 40
    assert {l["tag"] for l in META["loops"]} == {"hover", "climb", "smoothed_switch", "hover_motor0_half"} and all(l["nsteps"] <= 300 for l in META["loops"])
    climb = [l for l in META["loops"] if l["tag"] == "climb"][0]
    assert climb["max_command"] == climb["controller_max_thrust"] >= 20.0 and climb["max_realised"] <= 15.2 + 1e-9 and climb["events"] == 0
    assert climb["final_altitude"] < climb["unactuated_final_altitude"]
    assert max(s["final_events"] for s in META["sequences"]) > 5                      # past the watchdog threshold
    # the quirk values the issue quotes: hover's get_control_allocation and the infeasible roll-and-pitch command
    p = mo.default_params()
    pwm, _ = mo.mix(p, None, np.array([9.81]), np.zeros((1, 3)))
    assert np.max(np.abs(mo.readback(p, pwm)["allocation"][0] - [0.936, 11.85, 0.936, -11.27])) <= 5e-3
    pwm, _ = mo.mix(p, None, np.array([9.81]), np.array([[1.0, 1.0, 0.0]]))
    assert np.max(np.abs(pwm[0] - [0.759, 1.0, 0.759, 0.1])) <= 5e-4 and np.max(np.abs(mo.readback(p, pwm)["wrench"][0] - [8.95, 0.377, 0.377, 1.635])) <= 5e-4
    s = mo.reset(2)
    mo.mix(p, s, np.array([20.0, 0.3]), np.zeros((2, 3)))
    assert s[:, 0].tolist() == [0.0, 1.0]                                                # 20 N counts no event, 0.3 N counts one


def test_float32_evaluation_of_the_oracle_keeps_every_flag():
    """The yardstick of the float32 kernels' exact flags: with parameters and commands rounded to float32 the oracle decides every recorded row
    the same way (the margin is what makes that so)."""
    for seq in META["sequences"]:
        key, p = seq["key"], xc.seq_params(DATA, seq)
        p32 = {k: (np.asarray(v).astype(np.float32).astype(float) if isinstance(v, np.ndarray) else float(np.float32(v))) for k, v in p.items()}
        p32["watchdog_threshold"] = p["watchdog_threshold"]
        s64, s32 = mo.reset(1), mo.reset(1)
        for e in range(seq["calls"]):
            th, tq = DATA[key + "thrust"][e][None], DATA[key + "torque"][e][None]
            a, fa = mo.mix(p, s64, th, tq)
            b, fb = mo.mix(p32, s32, th.astype(np.float32).astype(float), tq.astype(np.float32).astype(float))
            assert fa[0] == fb[0], (seq["tag"], e)
            assert fa[0] & mo.NON_FINITE or np.max(np.abs(a - b)) <= 1e-4
