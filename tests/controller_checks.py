"""Parity checks of the consumer-side kernels (se3mpc_control_*, se3mpc_closed_loop_*), shared by the CPU suite (product
sources compiled for the host, tests/emu) and the GPU suite: against the vectors the reference's own classes produced
(tests/golden/controller_cases.npz) and against the oracle (oracle/controller_oracle.py) on random batches.

Tolerances: f64 1e-9 on every output per call (the kernel and NumPy differ only by the last bit of sin / cos / acos / sqrt and
of three-term sums); closed loops 1e-8 over <= 100 steps.  f32: the law has hard branches (saturation, singularity, tilt limit),
so f32 is compared call by call FROM THE SAME STATE with the oracle evaluated on the f32-rounded inputs: thrust 2e-5 relative,
torque 2e-4 absolute (torques are differences of O(1) rotation entries times gains of ~20) wherever both took the same
branches, and at most 2 % of the calls may sit on another side of a branch."""
import numpy as np

from dart_planner_amd.capi import ControllerParams, SimulatorParams
from oracle import controller_oracle as co


def oracle_config(seq=None) -> co.ControllerConfig:
    cfg = co.ControllerConfig()
    if seq is not None:
        cfg.anti_windup_method = seq["anti_windup"]
        cfg.yaw_singularity_fallback_method = seq["fallback"]
        cfg.default_heading_yaw = seq["default_heading_yaw"]
    return cfg


def state_to_oracle(st_rows: np.ndarray, cfg) -> co.ControllerState:
    """device controller state (B, 12) -> oracle ControllerState"""
    B = len(st_rows)
    s = co.ControllerState(B, cfg)
    s.integral = st_rows[:, 0:3].copy(); s.last_time = st_rows[:, 3].copy(); s.last_valid_thrust = st_rows[:, 4].copy()
    s.unsaturated_thrust = st_rows[:, 5].copy(); s.unsaturated_torque = st_rows[:, 6:9].copy()
    s.failsafe_count = st_rows[:, 9].astype(np.int64); s.halvings = st_rows[:, 10].astype(np.int64)
    fl = st_rows[:, 11].astype(np.int64)
    s.failsafe_active = (fl & 1) != 0; s.thrust_saturated = (fl & 2) != 0
    s.torque_saturated = np.stack([(fl & 4) != 0, (fl & 8) != 0, (fl & 16) != 0], axis=1)
    return s


def check_defaults(h):
    """se3mpc_controller_default_params / se3mpc_simulator_default_params == the values the reference instantiates
    (golden meta: GeometricController(tuning_profile="sitl_optimized").config, DroneSimulator())."""
    import json, os
    meta = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "controller_cases.json")))
    cp, sp = h.ops.lib.controller_default_params(), h.ops.lib.simulator_default_params()
    c = meta["config"]
    for k in ("kp_pos", "ki_pos", "kd_pos", "kp_att", "kd_att", "inertia", "max_torque_xyz", "max_integral_per_axis"):
        assert list(getattr(cp, k)) == c[k], k
    for k in ("max_integral_pos", "max_tilt_angle", "mass", "gravity", "max_thrust", "min_thrust", "tracking_error_threshold",
              "velocity_error_threshold", "back_calculation_gain", "integral_decay_factor", "saturation_threshold",
              "yaw_singularity_threshold", "default_heading_yaw"):
        assert getattr(cp, k) == c[k], k
    assert (cp.anti_windup_method, cp.yaw_fallback_method) == (0, 0) and c["anti_windup_method"] == "clamping" and c["yaw_singularity_fallback_method"] == "skip_yaw"
    s = meta["simulator"]
    assert (sp.mass, sp.gravity, list(sp.inertia), sp.max_thrust, sp.max_torque) == (s["mass"], s["gravity"], s["inertia"], s["max_thrust"], s["max_torque"])
    ref = ControllerParams.from_config(co.ControllerConfig())
    assert bytes(ref) == bytes(cp)
    assert bytes(SimulatorParams.reference_defaults()) == bytes(sp)


def check_control_sequences(h, data, meta):
    """Every call sequence the reference's controller produced, call by call, through se3mpc_control_* (B = 1 per sequence: the
    configurations differ), including the controller members after each call."""
    dt_ = h.dt
    f64 = dt_ == np.float64
    mism = calls = 0
    for seq in meta["sequences"]:
        k = seq["key"]
        cfg = oracle_config(seq)
        cp = ControllerParams.from_config(cfg)
        st = h.ops.controller_state(cp, 1)
        for i in range(seq["calls"]):
            a = lambda nm: h.to_dev(np.ascontiguousarray(data[k + nm][i][None].astype(dt_)))
            t = h.to_dev(np.array([data[k + "t"][i]], dtype=np.float64))
            before = h.to_host(st).copy()
            out = h.ops.control(cp, st, t, a("pos"), a("vel"), a("att"), a("omega"), a("dpos"), a("dvel"), a("dacc"),
                                h.to_dev(np.array([data[k + "yaw"][i]], dtype=dt_)), h.to_dev(np.array([data[k + "yaw_rate"][i]], dtype=dt_)),
                                want_body_rate=seq["kind"] == "body_rate")
            after = h.to_host(st)
            calls += 1
            if f64:
                if seq["kind"] == "body_rate":
                    assert abs(float(h.to_host(out["body_thrust"])[0]) - data[k + "br_thrust"][i]) <= 1e-9, (k, i)
                    assert np.max(np.abs(h.to_host(out["body_rates"])[0] - data[k + "br_rates"][i])) <= 1e-8, (k, i)
                else:
                    assert abs(float(h.to_host(out["thrust"])[0]) - data[k + "thrust"][i]) <= 1e-9, (k, i)
                    assert np.max(np.abs(h.to_host(out["torque"])[0] - data[k + "torque"][i])) <= 1e-9, (k, i)
                assert np.max(np.abs(after[0, 0:3] - data[k + "integral"][i])) <= 1e-11, (k, i)
                fl = int(after[0, 11])
                assert bool(fl & 1) == bool(data[k + "failsafe_active"][i]) and bool(fl & 2) == bool(data[k + "thrust_saturated"][i]), (k, i)
                assert [bool(fl & 4), bool(fl & 8), bool(fl & 16)] == [bool(x) for x in data[k + "torque_saturated"][i]], (k, i)
                assert int(after[0, 9]) == int(data[k + "failsafe_count"][i]) and int(after[0, 10]) == int(data[k + "halvings"][i]), (k, i)
                assert abs(after[0, 4] - data[k + "last_valid_thrust"][i]) <= 1e-9, (k, i)
                assert after[0, 3] == data[k + "t"][i]
            else:
                # f32: the oracle from the SAME controller state on the f32-rounded inputs
                r = lambda nm: data[k + nm][i][None].astype(dt_).astype(float)
                so = state_to_oracle(before, cfg)
                th, tq, fo = co.compute_control(so, cfg, np.array([data[k + "t"][i]]), r("pos"), r("vel"), r("att"), r("omega"), r("dpos"),
                                                r("dvel"), r("dacc"), np.array([float(dt_(data[k + "yaw"][i]))]), np.array([float(dt_(data[k + "yaw_rate"][i]))]))
                fl = int(h.to_host(out["flags"])[0])
                same = (bool(fl & 1) == bool(fo["failsafe"][0]) and bool(fl & 4) == bool(fo["thrust_saturated"][0]) and bool(fl & 8) == bool(fo["singular"][0])
                        and bool(fl & 16) == bool(fo["tilt_limited"][0]) and [bool(fl & 32), bool(fl & 64), bool(fl & 128)] == [bool(x) for x in so.torque_saturated[0] & ~fo["failsafe"][0]])
                if not same:
                    mism += 1
                    # put the device state on the oracle's side so the sequence continues from a common state
                    continue
                assert abs(float(h.to_host(out["thrust"])[0]) - th[0]) <= 2e-5 * max(1.0, abs(th[0])), (k, i)
                assert np.max(np.abs(h.to_host(out["torque"])[0] - tq[0])) <= 2e-4, (k, i, h.to_host(out["torque"])[0], tq[0])
                assert np.max(np.abs(after[0, 0:3] - so.integral[0])) <= 1e-5, (k, i)
    assert mism <= 0.02 * calls, (mism, calls)
    return mism, calls


def check_fast_sequences(h, data, meta):
    """The reference's compute_control_fast / compute_control_from_fast_state sequences (alone, and interleaved with compute_control on one
    controller record) through se3mpc_control_fast_* / se3mpc_control_*, call by call, with the controller members after each call and the
    saturation counts the reference keeps (summed from the flags, as the mirror class does)."""
    dt_ = h.dt
    f64 = dt_ == np.float64
    vc = meta["vehicle_constants"]
    veh = co.VehicleConstants(mass=vc["mass"], gravity=vc["gravity"])
    mism = calls = 0
    for seq in meta["fast_sequences"]:
        k = seq["key"]
        cfg = oracle_config(seq)
        cp = ControllerParams.from_config(cfg)
        st = h.ops.controller_state(cp, 1)
        n_thrust = n_torque = 0
        for i in range(seq["calls"]):
            a = lambda nm: h.to_dev(np.ascontiguousarray(data[k + nm][i][None].astype(dt_)))
            s1 = lambda nm: h.to_dev(np.array([data[k + nm][i]], dtype=dt_))
            before = h.to_host(st).copy()
            fast = int(data[k + "path"][i]) == 1
            if fast:
                out = h.ops.control_fast(cp, st, float(data[k + "dt"][i]), a("pos"), a("vel"), a("att"), a("omega"), a("dpos"), a("dvel"), a("dacc"),
                                         s1("yaw"), s1("yaw_rate"), vehicle_mass=vc["mass"], vehicle_gravity=vc["gravity"])
                fl = int(h.to_host(out["flags"])[0])
                n_thrust += int(bool(fl & 4)); n_torque += bin((fl >> 5) & 7).count("1")
            else:
                out = h.ops.control(cp, st, h.to_dev(np.array([data[k + "t"][i]], dtype=np.float64)), a("pos"), a("vel"), a("att"), a("omega"), a("dpos"),
                                    a("dvel"), a("dacc"), s1("yaw"), s1("yaw_rate"))
                fl = int(h.to_host(out["flags"])[0])
            after = h.to_host(st)
            calls += 1
            if f64:
                assert abs(float(h.to_host(out["thrust"])[0]) - data[k + "thrust"][i]) <= 1e-9, (k, i)
                assert np.max(np.abs(h.to_host(out["torque"])[0] - data[k + "torque"][i])) <= 1e-9, (k, i)
                assert np.max(np.abs(after[0, 0:3] - data[k + "integral"][i])) <= 1e-11, (k, i)
                sf = int(after[0, 11])
                assert bool(sf & 1) == bool(data[k + "failsafe_active"][i]) and bool(sf & 2) == bool(data[k + "thrust_saturated"][i]), (k, i)
                assert [bool(sf & 4), bool(sf & 8), bool(sf & 16)] == [bool(x) for x in data[k + "torque_saturated"][i]], (k, i)
                assert int(after[0, 9]) == int(data[k + "failsafe_count"][i]) and int(after[0, 10]) == int(data[k + "halvings"][i]), (k, i)
                assert abs(after[0, 4] - data[k + "last_valid_thrust"][i]) <= 1e-9 and abs(after[0, 5] - data[k + "unsaturated_thrust"][i]) <= 1e-9, (k, i)
                assert (n_thrust, n_torque) == (int(data[k + "thrust_saturation_count"][i]), int(data[k + "torque_saturation_count"][i])), (k, i)
                if fast:
                    assert after[0, 3] == before[0, 3] or (after[0, 3] != after[0, 3] and before[0, 3] != before[0, 3]), (k, i)   # last_time untouched
                    if fl & 2:                                                        # invalid dt: nothing changes (controller.py:279-280)
                        assert np.array_equal(after, before, equal_nan=True), (k, i)
            elif fast:
                r = lambda nm: data[k + nm][i][None].astype(dt_).astype(float)
                so = state_to_oracle(before, cfg)
                th, tq, fo = co.compute_control_fast(so, cfg, veh, float(data[k + "dt"][i]), r("pos"), r("vel"), r("att"), r("omega"), r("dpos"), r("dvel"),
                                                     r("dacc"), np.array([float(dt_(data[k + "yaw"][i]))]), np.array([float(dt_(data[k + "yaw_rate"][i]))]))
                same = (bool(fl & 2) == bool(fo["bad_dt"][0]) and bool(fl & 4) == bool(fo["thrust_saturated"][0]) and bool(fl & 8) == bool(fo["singular"][0])
                        and bool(fl & 16) == bool(fo["tilt_limited"][0]) and [bool(fl & 32), bool(fl & 64), bool(fl & 128)] == [bool(x) for x in fo["torque_saturated"][0]])
                if not same:
                    mism += 1
                    continue
                assert abs(float(h.to_host(out["thrust"])[0]) - th[0]) <= 2e-5 * max(1.0, abs(th[0])), (k, i)
                assert np.max(np.abs(h.to_host(out["torque"])[0] - tq[0])) <= 2e-4, (k, i)
                assert np.max(np.abs(after[0, 0:3] - so.integral[0])) <= 1e-5, (k, i)
    assert mism <= 0.02 * calls, (mism, calls)
    return mism, calls


def check_fast_batch_vs_oracle(h, B=300, calls=6, seed=0):
    """A random batch through se3mpc_control_fast_* against the oracle, state carried over `calls` calls (f64: every output and the record;
    f32: from the same record each call)."""
    rng = np.random.default_rng(seed)
    cfg = oracle_config()
    cp = ControllerParams.from_config(cfg)
    veh = co.VehicleConstants()
    st = h.ops.controller_state(cp, B)
    so = co.ControllerState(B, cfg)
    f64 = h.dt == np.float64
    worst = 0.0
    for c in range(calls):
        r3 = lambda s: rng.normal(0, s, (B, 3)).astype(h.dt)
        pos, vel, att, om = r3(3.0), r3(1.0), r3(0.4), r3(1.0)
        dpos, dvel, dacc = pos + r3(1.0), vel + r3(1.0), r3(2.0)
        yaw, yr = rng.uniform(-3, 3, B).astype(h.dt), rng.normal(0, 0.5, B).astype(h.dt)
        dt = [0.0025, 0.001, 0.2, 0.01, 0.0025, 0.05][c % 6]
        if not f64:
            so = state_to_oracle(h.to_host(st).copy(), cfg)
        out = h.ops.control_fast(cp, st, dt, *(h.to_dev(x) for x in (pos, vel, att, om, dpos, dvel, dacc, yaw, yr)), vehicle_mass=veh.mass,
                                 vehicle_gravity=veh.gravity)
        f = lambda x: x.astype(float)
        th, tq, fo = co.compute_control_fast(so, cfg, veh, dt, f(pos), f(vel), f(att), f(om), f(dpos), f(dvel), f(dacc), f(yaw), f(yr))
        fl = h.to_host(out["flags"])
        same = (((fl & 2) != 0) == fo["bad_dt"]) & (((fl & 4) != 0) == fo["thrust_saturated"]) & (((fl & 8) != 0) == fo["singular"]) & \
               (((fl & 16) != 0) == fo["tilt_limited"]) & np.all(np.stack([(fl & 32) != 0, (fl & 64) != 0, (fl & 128) != 0], 1) == fo["torque_saturated"], axis=1)
        if f64:
            assert same.all(), (c, int((~same).sum()))
            e = max(float(np.max(np.abs(h.to_host(out["thrust"]) - th))), float(np.max(np.abs(h.to_host(out["torque"]) - tq))),
                    float(np.max(np.abs(h.to_host(st)[:, 0:3] - so.integral))))
            assert e <= 1e-9, (c, e)
            worst = max(worst, e)
        else:
            assert same.mean() >= 0.97, (c, float(same.mean()))
            e = float(np.max(np.abs(h.to_host(out["thrust"])[same] - th[same]) / np.maximum(1.0, np.abs(th[same]))))
            assert e <= 2e-5 and float(np.max(np.abs(h.to_host(out["torque"])[same] - tq[same]))) <= 3e-4, (c, e)
            worst = max(worst, e)
    return worst


def check_building_blocks(h, B=200, seed=0):
    """se3mpc_controller_integral_update / attitude_torque / desired_frame against the oracle on random batches, and the known answers the
    reference's own controller tests hold (tests/test_controller_torque_calculation.py:20-92: with zero attitude gains the torque is the
    Coriolis term w x (I w), diagonal and full inertia, rtol 1e-10; tests/control/test_geometric_controller_yaw_singularity.py:215-233:
    cos_angle is |yaw_vector . b3| exactly, singular at >= the threshold)."""
    rng = np.random.default_rng(seed)
    f64 = h.dt == np.float64
    tol = 1e-10 if f64 else 2e-5
    dev = lambda a: h.to_dev(np.ascontiguousarray(np.asarray(a, dtype=h.dt)))
    # ---- Coriolis known answers
    cfg = oracle_config()
    cfg.kp_att = np.zeros(3); cfg.kd_att = np.zeros(3); cfg.inertia = np.array([0.025, 0.03, 0.045]); cfg.max_torque_xyz = np.array([100.0, 100.0, 100.0])
    cp = ControllerParams.from_config(cfg)
    st = h.ops.controller_state(cp, 1)
    w = np.array([[0.1, 0.2, 0.3]])
    up = np.array([[0.0, 0.0, 1.0]])
    out = h.ops.controller_attitude_torque(cp, st, dev(np.zeros((1, 3))), dev(w), dev(up))
    assert np.allclose(h.to_host(out["torque"])[0], np.cross(w[0], cfg.inertia * w[0]), rtol=1e-10 if f64 else 1e-5, atol=0 if f64 else 1e-9)
    full = np.array([[0.02, 0.001, 0.002], [0.001, 0.02, 0.003], [0.002, 0.003, 0.04]])
    out = h.ops.controller_attitude_torque(cp, st, dev(np.zeros((1, 3))), dev(w), dev(up), inertia=full)
    assert np.allclose(h.to_host(out["torque"])[0], np.cross(w[0], full @ w[0]), rtol=1e-10 if f64 else 1e-5, atol=0 if f64 else 1e-9)
    out = h.ops.controller_attitude_torque(cp, st, dev(np.zeros((1, 3))), dev(np.zeros((1, 3))), dev(up))
    assert not h.to_host(out["torque"]).any()
    # ---- singularity detection known answers
    cp0 = ControllerParams.from_config(oracle_config())
    for z, sing in ((0.0, False), (0.95, True), (-0.95, True), (0.5, True), (0.1, True), (0.09, False)):
        r = h.ops.controller_desired_frame(cp0, dev([[0.0, 0.0, z]]), dev(up))
        assert float(h.to_host(r["cos_angle"])[0]) == float(h.dt(abs(z))) and bool(h.to_host(r["singular"])[0]) == sing, z
    # ---- frames against the oracle: the attitude law's own construction (method -1) and each fallback forced
    yaw = rng.uniform(-3, 3, B); cur = rng.uniform(-3, 3, B)
    b3 = rng.normal(0, 1, (B, 3)); b3[: B // 4, :2] *= 0.02; b3 /= np.linalg.norm(b3, axis=1)[:, None]
    yv = np.stack([np.cos(yaw), np.sin(yaw), np.zeros(B)], 1)
    b3r, yvr, curr = (np.asarray(a, h.dt).astype(float) for a in (b3, yv, cur))
    att = np.stack([np.zeros(B), np.zeros(B), curr], 1)
    for name, code in (("skip_yaw", 0), ("default_heading", 1), ("maintain_current", 2), ("something_else", 3)):
        c2 = oracle_config(); c2.yaw_singularity_fallback_method = name; c2.default_heading_yaw = 0.7
        cpx = ControllerParams.from_config(c2)
        # forced fallback == the oracle's frame with the threshold at 0 (everything singular)
        c3 = oracle_config(); c3.yaw_singularity_fallback_method = name; c3.default_heading_yaw = 0.7; c3.yaw_singularity_threshold = 0.0
        for method, ocfg in ((-1, c2), (code, c3)):
            r = h.ops.controller_desired_frame(cpx, dev(yv), dev(b3), dev(cur), method)
            # the oracle takes yaw angles: rebuild them from the rounded vector so both see the same input
            b1, b2, b3n, sg = co.desired_frame(ocfg, b3r, att, np.arctan2(yvr[:, 1], yvr[:, 0]))
            fr = h.to_host(r["frame"]).astype(float)
            same = (h.to_host(r["singular"]).astype(bool) == sg) if method < 0 else np.ones(B, bool)
            assert same.mean() >= (1.0 if f64 else 0.98), (name, method)
            e = max(float(np.max(np.abs(fr[same, 0:3] - b1[same]))), float(np.max(np.abs(fr[same, 3:6] - b2[same]))))
            assert e <= (1e-9 if f64 else 3e-4), (name, method, e)
    # ---- _update_integral_error against the oracle, both methods, explicit saturation arguments
    for method in ("clamping", "back_calculation", "neither"):
        c2 = oracle_config(); c2.anti_windup_method = method
        cpx = ControllerParams.from_config(c2)
        st = h.ops.controller_state(cpx, B)
        so = co.ControllerState(B, c2)
        for _ in range(4):
            ve = rng.normal(0, 30.0, (B, 3)).astype(h.dt)
            sat = rng.integers(0, 16, B).astype(np.int32)
            rows = h.to_host(st).copy()
            rows[:, 5] = rng.uniform(15, 30, B); rows[:, 6:9] = rng.normal(0, 1, (B, 3))        # unsaturated thrust / torques the back-calculation reads
            rows = rows.astype(h.dt).astype(np.float64) if not f64 else rows
            st = h.to_dev(np.ascontiguousarray(rows))
            so = state_to_oracle(rows, c2)
            so.torque_saturated = np.stack([(sat & 2) != 0, (sat & 4) != 0, (sat & 8) != 0], 1)
            co.update_integral_error(so, c2, ve.astype(float), np.full(B, 0.01), (sat & 1) != 0, np.ones(B, bool))
            h.ops.controller_integral_update(cpx, st, h.to_dev(ve), 0.01, h.to_dev(sat))
            after = h.to_host(st)
            assert np.max(np.abs(after[:, 0:3] - so.integral)) <= (1e-12 if f64 else 2e-5), method
            assert np.array_equal(after[:, 3:], rows[:, 3:], equal_nan=True)                    # nothing but the integral moves
    return True


def check_closed_loops_golden(h, data, meta):
    """The reference's closed loops (planner plan -> sampler -> controller -> simulator) in ONE launch each, per-step logs against
    the reference's own."""
    assert h.dt == np.float64
    cp = ControllerParams.from_config(co.ControllerConfig())
    worst = 0.0
    for lp in meta["loops"]:
        k = lp["key"]
        sp = SimulatorParams.reference_defaults(max_thrust=lp["max_thrust"], max_torque=lp["max_torque"])
        st = h.ops.controller_state(cp, 1)
        d = lambda a: h.to_dev(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
        time = d([meta["T0"]]); pos = d([lp["p0"]]); vel = d([lp["v0"]]); att = d(np.zeros((1, 3))); om = d(np.zeros((1, 3)))
        out = h.ops.closed_loop(cp, sp, st, time, pos, vel, att, om, d(data[k + "ts"]), d(data[k + "P"]), d(data[k + "V"]), d(data[k + "A"]),
                                nsteps=lp["nsteps"], sim_dt=lp["sim_dt"], wind=None if lp["wind"] is None else d(lp["wind"]),
                                gust=None if lp["gust"] is None else (lp["gust"][0], lp["gust"][1]), stop_at_plan_end=not lp["emergency"], log=True)
        act = data[k + "active"].astype(bool)
        assert int(h.to_host(out["steps_taken"])[0]) == int(act.sum()) == lp["steps_active"], k
        ls, lc, lt = h.to_host(out["log_state"])[:, 0], h.to_host(out["log_cmd"])[:, 0], h.to_host(out["log_time"])[:, 0]
        ref_state = np.concatenate([data[k + "pos"], data[k + "vel"], data[k + "att"], data[k + "omega"]], axis=1)
        e = float(np.max(np.abs(ls - ref_state)))
        worst = max(worst, e)
        assert e <= 1e-8, (k, e)
        assert np.max(np.abs(lt - data[k + "t"])) <= 1e-9, k
        assert np.max(np.abs(lc[act, 0] - data[k + "thrust"][act])) <= 1e-8 and np.max(np.abs(lc[act, 1:] - data[k + "torque"][act])) <= 1e-8, k
        assert np.all(np.isnan(lc[~act]))
        final = np.concatenate([h.to_host(pos)[0], h.to_host(vel)[0], h.to_host(att)[0], h.to_host(om)[0], h.to_host(time)])
        assert np.max(np.abs(final - data[k + "final"])) <= 1e-8, k
    return worst


def random_plans(rng, B, N, t0, dt):
    """Smooth random plans shaped like the planner's output: positions along a line p0 -> goal with noise, constant velocity blocks."""
    ts = t0 + np.arange(N) * dt
    a = rng.uniform(-3, 3, (B, 1, 3)); b = rng.uniform(-3, 3, (B, 1, 3))
    s = np.linspace(0, 1, N)[None, :, None]
    P = a + s * (b - a) + rng.normal(0, 0.02, (B, N, 3))
    V = np.tile(rng.uniform(-2, 2, (B, 1, 3)), (1, N, 1)) + rng.normal(0, 0.05, (B, N, 3))
    A = rng.normal(0, 0.3, (B, N, 3))
    return ts, P, V, A


def check_closed_loop_vs_oracle(h, B=96, N=12, nsteps=40, seed=0, per_drone_plans=True):
    """Random drones, plans, winds and a gust against the batched oracle; the plan ends inside the run for some drones
    (per-drone timestamps), so `stop_at_plan_end` is exercised lane by lane."""
    rng = np.random.default_rng(seed)
    cfg = co.ControllerConfig()
    cp, sp = ControllerParams.from_config(cfg), SimulatorParams.reference_defaults()
    sim = co.SimulatorConfig()
    t0 = 500.0
    ts, P, V, A = random_plans(rng, B, N, t0, 0.02)
    TS = np.tile(ts, (B, 1)) - rng.choice([0.0, 0.05, 0.3], (B, 1))                       # some plans start (and end) earlier
    pos = P[:, 0] + rng.normal(0, 0.3, (B, 3)); vel = V[:, 0] + rng.normal(0, 0.3, (B, 3))
    att = rng.normal(0, 0.1, (B, 3)); om = rng.normal(0, 0.3, (B, 3)); t = np.full(B, t0)
    wind = rng.normal(0, 1.5, (B, 3))
    gust = (nsteps // 2, [4.0, -1.0, 0.5])
    dt_ = h.dt
    r = lambda a: np.asarray(a).astype(dt_).astype(float)
    if not per_drone_plans:
        P, V, A, TS = P[0], V[0], A[0], TS[0]
    fin, log = co.closed_loop(cfg, sim, co.ControllerState(B, cfg), r(pos), r(vel), r(att), r(om), t, TS, r(P), r(V), r(A), nsteps, 0.01,
                              wind=r(wind), gust_step=gust[0], gust_wind=gust[1])
    d = lambda a, ty=dt_: h.to_dev(np.ascontiguousarray(np.asarray(a).astype(ty)))
    st = h.ops.controller_state(cp, B)
    dtime, dpos, dvel, datt, dom = d(t, np.float64), d(pos), d(vel), d(att), d(om)
    out = h.ops.closed_loop(cp, sp, st, dtime, dpos, dvel, datt, dom, d(TS, np.float64), d(P), d(V), d(A), nsteps=nsteps, sim_dt=0.01,
                            wind=d(wind), gust=gust, log=True)
    taken = h.to_host(out["steps_taken"])
    assert np.array_equal(taken, log["active"].sum(0)), "steps taken per drone"
    assert len(np.unique(taken)) >= 3 or not per_drone_plans          # plans end at different steps, lane by lane
    ls = h.to_host(out["log_state"]).astype(float)
    ref = np.concatenate([log["pos"], log["vel"], log["att"], log["omega"]], axis=2)
    if dt_ == np.float64:
        assert np.max(np.abs(ls - ref)) <= 1e-8
        assert np.max(np.abs(h.to_host(dpos) - fin["pos"])) <= 1e-8 and np.max(np.abs(h.to_host(dtime) - fin["t"])) <= 1e-9
    else:
        # f32 closed loop: drones that never sat near a branch track the f64 oracle to a few 1e-4 over 40 steps
        err = np.max(np.abs(ls - ref), axis=(0, 2))
        assert np.median(err) <= 5e-3 and np.mean(err <= 5e-2) >= 0.9, (np.median(err), np.mean(err <= 5e-2))
    return float(np.max(np.abs(ls - ref)))


def check_plan_rules(h):
    """The status every entry point with a plan operand returns for every plan argument, in the harness's precision: se3mpc_control_plan_*,
    se3mpc_closed_loop_*, se3mpc_smoother_update_* (old and new plan), se3mpc_smoother_desired_*, se3mpc_closed_loop_smoothed_*.

    Where the expectations come from.  include/se3mpc.h: a negative row count or stride and more than 4096 rows are SE3MPC_ERR_SHAPE, a NULL
    required operand is SE3MPC_ERR_NULL, V and A may be NULL, B = 0 / nsteps = 0 is a no-op that returns SE3MPC_OK, and the smoother's entry
    points accept a plan of 0 rows.  The header is silent on the rest, and there the behaviour of the library decides (characterised once,
    and pinned here): (a) the controller's two entry points need at least one row, the smoother's take none; (b) the shape of a plan is
    checked before the no-op return in both families, but its stamps and positions are looked at AFTER that return by the controller's entry
    points (an empty batch may come with NULL plans) and BEFORE it by the smoother's; (c) the OLD plan of se3mpc_smoother_update_* is never
    required (a drone without a trajectory does not read it); (d) parameter errors win over plan errors, shape errors over NULL errors.
    B = 2 drones, plans of 2 rows (one 4096-row plan for the upper end of the range); a rejected or no-op call leaves every in/out and
    output buffer, pre-filled with a byte pattern, untouched."""
    from dart_planner_amd.capi import SmootherParams
    ops, lib = h.ops, h.ops.lib
    ptr = ops.be.ptr
    suf = "f64" if h.dt == np.float64 else "f32"
    OK, NULL, SHAPE, PARAM = 0, -1, -3, -4
    B, ROWS = 2, 4096
    cp, sp, mp = lib.controller_default_params(), lib.simulator_default_params(), SmootherParams.reference_defaults()
    real = lambda a: h.to_dev(np.ascontiguousarray(np.asarray(a).astype(h.dt)))
    ts = h.to_dev(np.arange(ROWS) * 0.01)
    P, V, A = real(np.zeros((ROWS, 3))), real(np.zeros((ROWS, 3))), real(np.zeros((ROWS, 3)))
    ctrl0, smooth0 = np.array(h.to_host(ops.controller_state(cp, B))), np.array(h.to_host(ops.smoother_state(B)))
    pattern = lambda shape, ty: h.to_dev(np.frombuffer(bytearray(b"\x5a" * (int(np.prod(shape)) * np.dtype(ty).itemsize)), dtype=ty).reshape(shape))

    def plan(N=2, stamps=True, pos=True, vel=True, acc=True, strides=(0, 0, 0, 0)):
        return [N, ptr(ts) if stamps else 0, strides[0], ptr(P) if pos else 0, strides[1], ptr(V) if vel else 0, strides[2], ptr(A) if acc else 0, strides[3]]

    def buffers():
        b = dict(time=h.to_dev(np.zeros(B)), sample=h.to_dev(np.zeros(B)), state=h.to_dev(ctrl0.copy()), sm=h.to_dev(smooth0.copy()))
        for k in ("pos", "vel", "att", "om"):
            b[k] = real(np.zeros((B, 3)))
        b.update(thrust=pattern((B,), h.dt), torque=pattern((B, 3), h.dt), flags=pattern((B,), np.int32), target=pattern((B, 9), h.dt),
                 branch=pattern((B,), np.int32), taken=pattern((B,), np.int32), log_state=pattern((3, B, 12), h.dt), log_cmd=pattern((3, B, 4), h.dt),
                 log_time=pattern((3, B), np.float64), log_target=pattern((3, B, 9), h.dt))
        return b

    def control_plan(b, pl, B_=B, nsteps=None, **kw):
        return lib.loop_status("control_plan", suf, kw.get("cp", cp), B_, ptr(b["time"]), ptr(b["sample"]), ptr(b["pos"]), ptr(b["vel"]), ptr(b["att"]),
                               ptr(b["om"]), *pl, 0 if kw.get("no_state") else ptr(b["state"]), ptr(b["thrust"]), ptr(b["torque"]), 0, 0, ptr(b["flags"]),
                               ptr(b["target"]), 0)

    def closed_loop(b, pl, B_=B, nsteps=3, **kw):
        return lib.loop_status("closed_loop", suf, cp, sp, B_, nsteps, kw.get("sim_dt", 0.01), *pl, ptr(b["time"]), ptr(b["pos"]), ptr(b["vel"]), ptr(b["att"]),
                               ptr(b["om"]), 0 if kw.get("no_state") else ptr(b["state"]), 0, kw.get("wind_stride", 0), -1, None, 0, ptr(b["log_state"]),
                               ptr(b["log_cmd"]), ptr(b["log_time"]), ptr(b["taken"]), 0)

    def update_new(b, pl, B_=B, nsteps=None, old=None, **kw):
        return lib.loop_status("smoother_update", suf, mp, B_, ptr(b["time"]), *(plan() if old is None else old), *pl, 0 if kw.get("no_state") else ptr(b["sm"]), 0)

    def update_old(b, pl, B_=B, nsteps=None, **kw):
        return update_new(b, plan(), B_, old=pl, **kw)

    def desired(b, pl, B_=B, nsteps=None, **kw):
        return lib.loop_status("smoother_desired", suf, mp, B_, ptr(b["time"]), ptr(b["pos"]), ptr(b["vel"]), *pl, 0 if kw.get("no_state") else ptr(b["sm"]),
                               ptr(b["target"]), ptr(b["branch"]), 0)

    def smoothed(b, pl, B_=B, nsteps=3, **kw):
        return lib.loop_status("closed_loop_smoothed", suf, mp, cp, sp, B_, nsteps, kw.get("sim_dt", 0.01), *pl, ptr(b["time"]), ptr(b["pos"]), ptr(b["vel"]),
                               ptr(b["att"]), ptr(b["om"]), 0 if kw.get("no_state") else ptr(b["state"]), ptr(b["sm"]), 0, kw.get("wind_stride", 0), -1, None,
                               ptr(b["log_state"]), ptr(b["log_cmd"]), ptr(b["log_time"]), ptr(b["log_target"]), 0)

    def call(fn, pl, **kw):
        """-> the status; a call that is rejected or has nothing to do must not have written a byte"""
        b = buffers()
        before = {k: np.array(h.to_host(v)).tobytes() for k, v in b.items()}
        rc = fn(b, pl, **kw)
        if rc != OK or kw.get("B_", B) == 0 or kw.get("nsteps", 1) == 0:
            for k, v in b.items():
                assert np.array(h.to_host(v)).tobytes() == before[k], (fn.__name__, pl, kw, k)
        return rc

    def expected(min_rows, presence, empty, N=2, stamps=True, pos=True, vel=True, acc=True, strides=(0, 0, 0, 0)):
        """min_rows: 1 controller family, 0 smoother family; presence: "after" (the no-op return), "before" it, or None (never required)"""
        if N < min_rows or N > 4096 or min(strides) < 0:
            return SHAPE
        missing = N > 0 and not (stamps and pos)
        if presence == "before" and missing:
            return NULL
        if empty:
            return OK
        return NULL if presence == "after" and missing else OK

    cases = [dict(N=n) for n in (-1, 0, 1, 4096, 4097)]
    cases += [dict(strides=tuple(-1 if i == j else 0 for i in range(4))) for j in range(4)]
    cases += [dict(stamps=False), dict(pos=False), dict(vel=False), dict(acc=False), dict(vel=False, acc=False)]
    cases += [dict(N=0, stamps=False, pos=False), dict(N=-1, stamps=False), dict(N=4097, pos=False), dict(stamps=False, strides=(0, 0, -1, 0))]   # two errors at once
    entries = [(control_plan, 1, "after", False), (closed_loop, 1, "after", True), (update_old, 0, None, False), (update_new, 0, "before", False),
               (desired, 0, "before", False), (smoothed, 0, "before", True)]
    checked = 0
    for fn, min_rows, presence, has_nsteps in entries:
        for case in cases:
            for kw in [dict(), dict(B_=0)] + ([dict(nsteps=0)] if has_nsteps else []):
                want = expected(min_rows, presence, bool(kw), **case)
                got = call(fn, plan(**case), **kw)
                assert got == want, (fn.__name__, suf, case, kw, got, want)
                checked += 1
    assert checked == 18 * (4 * 2 + 2 * 3)
    # the two traps, literally
    assert call(closed_loop, plan(stamps=False, pos=False), B_=0) == OK and call(control_plan, plan(stamps=False, pos=False), B_=0) == OK
    assert call(closed_loop, plan(N=0)) == SHAPE and call(control_plan, plan(N=0)) == SHAPE
    assert call(smoothed, plan(stamps=False), B_=0) == NULL and call(smoothed, plan(pos=False), nsteps=0) == NULL and call(desired, plan(pos=False), B_=0) == NULL
    assert "plan" in lib.last_error()
    assert call(update_new, plan(stamps=False), B_=0) == NULL and call(update_old, plan(stamps=False, pos=False)) == OK
    assert call(smoothed, plan(N=0)) == OK and call(desired, plan(N=0, stamps=False, pos=False)) == OK and call(update_new, plan(N=0)) == OK
    # which of two errors wins
    for fn in (closed_loop, smoothed):
        assert call(fn, plan(N=-1), sim_dt=float("nan")) == PARAM                   # parameters before the plan
        assert call(fn, plan(stamps=False), wind_stride=-1) == SHAPE               # any shape error before any NULL
        assert call(fn, plan(N=4097), B_=-1) == SHAPE and call(fn, plan(stamps=False), B_=-1) == SHAPE
    for fn in (control_plan, closed_loop, update_new, desired, smoothed):
        assert call(fn, plan(N=-1), no_state=True) == SHAPE and call(fn, plan(pos=False), no_state=True) == NULL
    assert call(update_new, plan(pos=False), old=plan(N=-1)) == SHAPE and call(update_new, plan(N=4097), old=plan(stamps=False)) == SHAPE
    bad = lib.controller_default_params(); bad.mass = 0.0
    assert call(control_plan, plan(N=0), cp=bad) == PARAM


def record_launch_sequences(ops, monkeypatch):
    """The library calls of every public method of ClosedLoopMonteCarlo at B = 2, N = 6, 3 cycles x 2 substeps, 8 samples x 1 iteration, as
    {method: [one line per call]}: the entry point, then its arguments -- scalars as they are, a parameter struct by its class name, a
    non-NULL address as P (NULL stays 0).  Host logic only: the calls are recorded, not made (8 samples is below what se3mpc_mppi_* runs), on
    zero-filled buffers (so the overflow counter run_fused reads is 0).  Also asserted here, on the recorded addresses: run() hands every
    cycle the same plan tensors, a smoothed run alternates two sets and names the previous cycle's set as the old plan."""
    import ctypes as C
    import torch
    from dart_planner_amd.capi import Params, SmootherParams
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    calls = []
    word = lambda a: (type(a).__name__ if isinstance(a, C.Structure) else tuple(a) if isinstance(a, C.Array) else "P" if isinstance(a, int) and a >= 4096 else a)
    rec = lambda name, args: calls.append((name, [word(a) for a in args], list(args)))
    monkeypatch.setattr(ops.lib, "call", lambda base, suf, *args, params=None: rec(f"{base}_{suf}", (params,) + args))
    monkeypatch.setattr(ops.lib, "loop_call", lambda base, suf, *args: rec(f"{base}_{suf}", args))
    monkeypatch.setattr(ops.lib, "controller_reset", lambda *args: rec("controller_reset", args))
    monkeypatch.setattr(ops.lib, "smoother_reset", lambda *args: rec("smoother_reset", args))
    monkeypatch.setattr(ops.be, "empty", lambda shape, kind: torch.zeros(shape, dtype=ops.be._dt[kind]))
    B, N, cycles, substeps, sim_dt = 2, 6, 3, 2, 0.01
    mc = ClosedLoopMonteCarlo(ops, Params.reference_defaults(horizon=N), ControllerParams.from_config(co.ControllerConfig()), SimulatorParams.reference_defaults())
    mp = SmootherParams.reference_defaults()
    p0, v0, goal = torch.zeros(B, 3, dtype=torch.float64), torch.zeros(B, 3, dtype=torch.float64), torch.ones(B, 3, dtype=torch.float64)
    wind = torch.ones(B, 3, dtype=torch.float64)
    mppi = dict(n_samples=8, iters=1, sigma=1.0, temperature=5.0, seed=3)
    runs = dict(run=lambda: mc.run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind),
                run_smoothed=lambda: mc.run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind, smoother=mp),
                run_fused=lambda: mc.run_fused(p0, v0, goal, cycles, substeps, sim_dt, wind=wind),
                run_mppi=lambda: mc.run_mppi(p0, v0, goal, cycles, substeps, sim_dt, wind=wind, **mppi),
                run_mppi_smoothed=lambda: mc.run_mppi(p0, v0, goal, cycles, substeps, sim_dt, wind=wind, smoother=mp, **mppi),
                run_mppi_fused=lambda: mc.run_mppi_fused(p0, v0, goal, cycles, substeps, sim_dt, wind=wind, **mppi))
    out, raw = {}, {}
    for name, fn in runs.items():
        del calls[:]
        keep = fn()                                                           # (alive while the addresses are compared)
        out[name] = [" ".join([c[0]] + [str(w) for w in c[1]]) for c in calls]
        raw[name] = [(c[0], c[2]) for c in calls]
        del keep
    plan_of = lambda args, at: tuple(args[at + i] for i in (1, 3, 5, 7))      # the four addresses of a nine-argument plan group
    loops = [plan_of(a, 5)[1:] for n, a in raw["run"] if n == "closed_loop_f64"]
    assert len(loops) == cycles and len(set(loops)) == 1, "run() re-uses one set of plan tensors"
    for name in ("run_smoothed", "run_mppi_smoothed"):
        upd = [(plan_of(a, 3)[1:], plan_of(a, 12)[1:]) for n, a in raw[name] if n == "smoother_update_f64"]
        flown = [plan_of(a, 6)[1:] for n, a in raw[name] if n == "closed_loop_smoothed_f64"]
        assert len(upd) == len(flown) == cycles and upd[0][0] == (0, 0, 0)
        for c in range(cycles):
            assert flown[c] == upd[c][1] and (c == 0 or upd[c][0] == upd[c - 1][1]), (name, c)
        if name == "run_smoothed":
            assert upd[0][1] == upd[2][1] != upd[1][1], "a smoothed run alternates two sets of plan tensors"
    return out


# what record_launch_sequences gives for the six methods (written from a run of the commit before ClosedLoopMonteCarlo got its one _start / _actor)
LAUNCH_SEQUENCES = {'run': ['controller_reset ControllerParams 2 P 0',
         'solve_f64 Params 2 P P P 0 P P P 0 0 0 0',
         'closed_loop_f64 ControllerParams SimulatorParams 2 2 0.01 6 P 0 P 54 P 54 P 18 P P P P P P P 3 -1 None 0 0 0 0 P 0',
         'solve_f64 Params 2 P P P 0 P P P 0 0 0 0',
         'closed_loop_f64 ControllerParams SimulatorParams 2 2 0.01 6 P 0 P 54 P 54 P 18 P P P P P P P 3 -1 None 0 0 0 0 P 0',
         'solve_f64 Params 2 P P P 0 P P P 0 0 0 0',
         'closed_loop_f64 ControllerParams SimulatorParams 2 2 0.01 6 P 0 P 54 P 54 P 18 P P P P P P P 3 -1 None 0 0 0 0 P 0'],
 'run_smoothed': ['controller_reset ControllerParams 2 P 0',
                  'smoother_reset 2 P 0',
                  'solve_f64 Params 2 P P P 0 P P P 0 0 0 0',
                  'smoother_update_f64 SmootherParams 2 P 0 0 0 0 0 0 0 0 0 6 P 0 P 54 P 54 P 18 P 0',
                  'closed_loop_smoothed_f64 SmootherParams ControllerParams SimulatorParams 2 2 0.01 6 P 0 P 54 P 54 P 18 P P P P P P P P 3 -1 None 0 0 0 0 0',
                  'solve_f64 Params 2 P P P 0 P P P 0 0 0 0',
                  'smoother_update_f64 SmootherParams 2 P 6 P 0 P 54 P 54 P 18 6 P 0 P 54 P 54 P 18 P 0',
                  'closed_loop_smoothed_f64 SmootherParams ControllerParams SimulatorParams 2 2 0.01 6 P 0 P 54 P 54 P 18 P P P P P P P P 3 -1 None 0 0 0 0 0',
                  'solve_f64 Params 2 P P P 0 P P P 0 0 0 0',
                  'smoother_update_f64 SmootherParams 2 P 6 P 0 P 54 P 54 P 18 6 P 0 P 54 P 54 P 18 P 0',
                  'closed_loop_smoothed_f64 SmootherParams ControllerParams SimulatorParams 2 2 0.01 6 P 0 P 54 P 54 P 18 P P P P P P P P 3 -1 None 0 0 0 0 0'],
 'run_fused': ['controller_reset ControllerParams 2 P 0', 'monte_carlo_f64 Params ControllerParams SimulatorParams 2 3 2 0.01 P P 3 P P P P P P 0 0 0 P 0'],
 'run_mppi': ['controller_reset ControllerParams 2 P 0',
              'mppi_closed_loop_f64 Params ControllerParams SimulatorParams 2 1 2 0.01 0 6 8 1 1.0 5.0 3 0 0 P 0 0 0.0 P 3 P P P P P P P P P 0 0 0',
              'mppi_closed_loop_f64 Params ControllerParams SimulatorParams 2 1 2 0.01 1 6 8 1 1.0 5.0 3 0 0 P 0 0 0.0 P 3 P P P P P P P P P 0 0 0',
              'mppi_closed_loop_f64 Params ControllerParams SimulatorParams 2 1 2 0.01 2 6 8 1 1.0 5.0 3 0 0 P 0 0 0.0 P 3 P P P P P P P P P 0 0 0'],
 'run_mppi_smoothed': ['controller_reset ControllerParams 2 P 0',
                       'smoother_reset 2 P 0',
                       'mppi_closed_loop_f64 Params ControllerParams SimulatorParams 2 1 0 0.01 0 6 8 1 1.0 5.0 3 0 0 P 0 0 0.0 P 3 P P P P P P P P P P 0 0',
                       'smoother_update_f64 SmootherParams 2 P 0 0 0 0 0 0 0 0 0 6 P 0 P 54 P 54 P 54 P 0',
                       'closed_loop_smoothed_f64 SmootherParams ControllerParams SimulatorParams 2 2 0.01 6 P 0 P 54 P 54 P 54 P P P P P P P P 3 -1 None 0 0 0 0 0',
                       'mppi_closed_loop_f64 Params ControllerParams SimulatorParams 2 1 0 0.01 1 6 8 1 1.0 5.0 3 0 0 P 0 0 0.0 P 3 P P P P P P P P P P 0 0',
                       'smoother_update_f64 SmootherParams 2 P 6 P 0 P 54 P 54 P 54 6 P 0 P 54 P 54 P 54 P 0',
                       'closed_loop_smoothed_f64 SmootherParams ControllerParams SimulatorParams 2 2 0.01 6 P 0 P 54 P 54 P 54 P P P P P P P P 3 -1 None 0 0 0 0 0',
                       'mppi_closed_loop_f64 Params ControllerParams SimulatorParams 2 1 0 0.01 2 6 8 1 1.0 5.0 3 0 0 P 0 0 0.0 P 3 P P P P P P P P P P 0 0',
                       'smoother_update_f64 SmootherParams 2 P 6 P 0 P 54 P 54 P 54 6 P 0 P 54 P 54 P 54 P 0',
                       'closed_loop_smoothed_f64 SmootherParams ControllerParams SimulatorParams 2 2 0.01 6 P 0 P 54 P 54 P 54 P P P P P P P P 3 -1 None 0 0 0 0 0'],
 'run_mppi_fused': ['controller_reset ControllerParams 2 P 0', 'mppi_closed_loop_f64 Params ControllerParams SimulatorParams 2 3 2 0.01 0 6 8 1 1.0 5.0 3 0 0 P 0 0 0.0 P 3 P P P P P P P P P 0 0 0']}


def check_launch_sequences(ops, monkeypatch):
    got = record_launch_sequences(ops, monkeypatch)
    assert sorted(got) == sorted(LAUNCH_SEQUENCES)
    for name, want in LAUNCH_SEQUENCES.items():
        assert got[name] == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(got[name], want)) if g != w], len(got[name]), len(want))


def check_operand_rules(h, monkeypatch):
    """Ops.closed_loop, control_plan, simulator_step, control, controller_attitude_torque and controller_desired_frame refuse, with a
    ValueError and before any launch, a clock, controller record, wind, thrust or yaw operand of the wrong row count, the wrong dtype or
    (clocks and records) the wrong width, and leave the in/out tensors bit for bit as they were.  B = 3 drones, a plan of N = 2 rows.
    A wrongly sized buffer must only ever be rejected: the library's call is replaced by a failure for the length of this check, so a
    missing rule shows as a failed test and never as a kernel striding over a short buffer."""
    import pytest
    ops = h.ops
    B, N = 3, 2
    dt_, other = h.dt, (np.float32 if h.dt == np.float64 else np.float64)
    cp, sp = ops.lib.controller_default_params(), ops.lib.simulator_default_params()
    state = ops.controller_state(cp, B)                                        # (the one launch of this check: a fresh record)

    def no_launch(base, suf, *args):
        raise AssertionError(f"se3mpc_{base}_{suf} was called with an operand that should have been refused")
    monkeypatch.setattr(ops.lib, "loop_call", no_launch)
    d = lambda a, ty=dt_: h.to_dev(np.ascontiguousarray(np.asarray(a).astype(ty)))
    good = dict(state=state, time=d(np.zeros(B), np.float64), sample_time=d(np.zeros(B), np.float64), pos=d(np.zeros((B, 3))), vel=d(np.zeros((B, 3))),
                att=d(np.zeros((B, 3))), omega=d(np.zeros((B, 3))), thrust=d(np.full(B, 9.0)), torque=d(np.zeros((B, 3))), wind=d(np.ones((B, 3))),
                yaw=d(np.zeros(B)), yaw_rate=d(np.zeros(B)), current_yaw=d(np.zeros(B)), dpos=d(np.ones((B, 3))), dvel=d(np.zeros((B, 3))),
                b3_des=d(np.tile([0.0, 0.0, 1.0], (B, 1))), yaw_vector=d(np.tile([1.0, 0.0, 0.0], (B, 1))))
    ts, P = d(np.arange(N) * 0.1, np.float64), d(np.zeros((N, 3)))
    clock_bad = lambda: [d(np.zeros(B + 1), np.float64), d(np.zeros(B), np.float32), d(np.zeros((B, 2)), np.float64)]          # rows, dtype, width
    record_bad = lambda: [d(np.zeros((B + 1, 12)), np.float64), d(np.zeros((B, 12)), np.float32), d(np.zeros((B, 13)), np.float64)]
    per_drone_bad = lambda: [d(np.zeros(B + 1)), d(np.zeros(B), other)]                                                         # rows, dtype
    wind_bad = lambda: [d(np.ones((B + 1, 3))), d(np.ones((B, 3)), other), d(np.ones(3), other)]
    calls = dict(
        closed_loop=(lambda g: ops.closed_loop(cp, sp, g["state"], g["time"], g["pos"], g["vel"], g["att"], g["omega"], ts, P, nsteps=2, wind=g["wind"]),
                     dict(time=clock_bad, state=record_bad, wind=wind_bad)),
        control_plan=(lambda g: ops.control_plan(cp, g["state"], g["time"], g["sample_time"], g["pos"], g["vel"], g["att"], g["omega"], ts, P),
                      dict(time=clock_bad, sample_time=clock_bad, state=record_bad)),
        simulator_step=(lambda g: ops.simulator_step(sp, g["time"], g["pos"], g["vel"], g["att"], g["omega"], g["thrust"], g["torque"], 0.01, wind=g["wind"]),
                        dict(time=clock_bad, thrust=per_drone_bad, wind=wind_bad)),
        control=(lambda g: ops.control(cp, g["state"], g["time"], g["pos"], g["vel"], g["att"], g["omega"], g["dpos"], g["dvel"], None, g["yaw"], g["yaw_rate"]),
                 dict(yaw=per_drone_bad, yaw_rate=per_drone_bad, time=clock_bad)),
        controller_attitude_torque=(lambda g: ops.controller_attitude_torque(cp, g["state"], g["att"], g["omega"], g["b3_des"], g["yaw"], g["yaw_rate"]),
                                    dict(yaw=per_drone_bad, yaw_rate=per_drone_bad)),
        controller_desired_frame=(lambda g: ops.controller_desired_frame(cp, g["yaw_vector"], g["b3_des"], g["current_yaw"]), dict(current_yaw=per_drone_bad)))
    before = {k: np.array(h.to_host(v)).tobytes() for k, v in good.items()}
    cases = 0
    for name, (fn, operands) in calls.items():
        for operand, bad in operands.items():
            for wrong in bad():
                with pytest.raises(ValueError):
                    fn(dict(good, **{operand: wrong}))
                cases += 1
    assert cases == 3 * 3 + 3 * 3 + (3 + 2 + 3) + (2 + 2 + 3) + 4 + 2
    for k, v in good.items():
        assert np.array(h.to_host(v)).tobytes() == before[k], k
