"""GPU suite, consumer side of the contract: se3mpc_control_*, se3mpc_control_plan_*,
se3mpc_simulator_step_*, se3mpc_closed_loop_* on a real MI355X through the C ABI, against the vectors the reference's own
controller / simulator / plan sampler produced and against the oracle; then the receding-horizon Monte-Carlo of BASELINE.json
config 5's named test shape (tests/test_monte_carlo_sim.py: 33 planning cycles of 0.15 s), entirely on the device."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import controller_checks as cc  # noqa: E402
import parity_checks as pc  # noqa: E402
from oracle import controller_oracle as co  # noqa: E402
from oracle import se3mpc_oracle as orc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gpu_ops():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend("cuda:0"))
    assert os.path.basename(ops.lib.path) == "libse3mpc.so"
    return ops


@pytest.fixture(scope="module")
def golden_controller():
    return np.load(os.path.join(GOLDEN, "controller_cases.npz")), json.load(open(os.path.join(GOLDEN, "controller_cases.json")))


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"), lambda a: a.detach().cpu().numpy(), dt)


def test_controller_defaults(gpu_ops):
    cc.check_defaults(harness(gpu_ops, np.float64))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_control_reproduces_reference_sequences(gpu_ops, golden_controller, dt):
    data, meta = golden_controller
    mism, calls = cc.check_control_sequences(harness(gpu_ops, dt), data, meta)
    print(f"{np.dtype(dt).name}: {calls} controller calls, {mism} on another side of a branch")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_control_fast_reproduces_reference_sequences(gpu_ops, golden_controller, dt):
    """compute_control_fast / compute_control_from_fast_state (the reference's 400 Hz hardware loop path), alone and interleaved with
    compute_control on one controller record, against the reference's own returns; then a 4096-drone batch against the oracle."""
    data, meta = golden_controller
    mism, calls = cc.check_fast_sequences(harness(gpu_ops, dt), data, meta)
    worst = cc.check_fast_batch_vs_oracle(harness(gpu_ops, dt), B=4096, calls=6, seed=6)
    print(f"{np.dtype(dt).name}: {calls} fast-path calls, {mism} on another side of a branch; 4096-drone batch worst {worst:.2e}")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_controller_building_blocks(gpu_ops, dt):
    """_update_integral_error, _geometric_attitude_control / _fast_geometric_attitude_control, _detect_yaw_singularity / _handle_yaw_singularity
    as device entry points: the oracle on random batches and the known answers of the reference's own controller tests."""
    cc.check_building_blocks(harness(gpu_ops, dt), B=2048, seed=8)


def test_controller_mirror_fast_path(gpu_ops, golden_controller):
    """The mirror class's compute_control_fast / compute_control_from_fast_state and the members the reference's own controller tests read
    (integral_vel_error, last_thrust_saturated, unsaturated_thrust, the saturation counts of get_performance_metrics)."""
    from dart_planner_amd.control.geometric_controller import GeometricController, GeometricControllerConfig
    from dart_planner_amd.common.types import FastDroneState
    data, meta = golden_controller
    seq = next(s for s in meta["fast_sequences"] if s["kind"] == "fast_state")
    k = seq["key"]
    ctrl = GeometricController(config=GeometricControllerConfig(), tuning_profile="sitl_optimized")
    ctrl._ops = gpu_ops
    for i in range(seq["calls"]):
        fs = FastDroneState(timestamp=float(data[k + "t"][i]), position=data[k + "pos"][i], velocity=data[k + "vel"][i], attitude=data[k + "att"][i],
                            angular_velocity=data[k + "omega"][i])
        thrust, torque = ctrl.compute_control_from_fast_state(fs, data[k + "dpos"][i], data[k + "dvel"][i], data[k + "dacc"][i], float(data[k + "yaw"][i]),
                                                              float(data[k + "yaw_rate"][i]), float(data[k + "dt"][i]))
        assert abs(thrust - data[k + "thrust"][i]) <= 1e-9 and np.max(np.abs(torque - data[k + "torque"][i])) <= 1e-9, i
        assert np.max(np.abs(ctrl.integral_vel_error - data[k + "integral"][i])) <= 1e-11
        assert abs(ctrl.unsaturated_thrust - data[k + "unsaturated_thrust"][i]) <= 1e-9 and ctrl.last_thrust_saturated == bool(data[k + "thrust_saturated"][i])
    m = ctrl.get_performance_metrics()
    assert m["thrust_saturation_count"] == int(data[k + "thrust_saturation_count"][-1]) and m["torque_saturation_count"] == int(data[k + "torque_saturation_count"][-1])
    assert ctrl.last_time is None                      # the fast path never stamps the controller (controller.py:253-346)
    # an invalid dt: the vehicle's hover thrust, zero torque (controller.py:279-280)
    th, tq = ctrl.compute_control_fast(np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3), np.ones(3), np.zeros(3), np.zeros(3), dt=0.2)
    assert th == 1.0 * 9.80665 and not tq.any()


def test_controller_mirror_private_steps(gpu_ops):
    """The mirror's private steps on the device, with the situations and known answers of the reference's own controller tests
    (tests/test_controller_torque_calculation.py:20-92, :157-176; tests/control/test_geometric_controller_anti_windup.py:44-75, :96-130, :199-214;
    tests/control/test_geometric_controller_yaw_singularity.py:32-66, :79-96, :215-233) -- those files themselves run in place on the CPU box."""
    from dart_planner_amd.control.geometric_controller import GeometricController, GeometricControllerConfig
    from dart_planner_amd.common.types import DroneState

    def make(**kw):
        cfg = GeometricControllerConfig()
        for k, v in kw.items():
            setattr(cfg, k, v)
        c = GeometricController(config=cfg, tuning_profile="")
        c._ops = gpu_ops
        return c
    # torque = w x (I w) with zero attitude gains: diagonal inertia, then a full matrix assigned to _fast_inertia
    c = make(inertia=np.array([0.025, 0.03, 0.045]), max_torque_xyz=np.array([100.0, 100.0, 100.0]), kp_att=np.zeros(3), kd_att=np.zeros(3))
    w = np.array([0.1, 0.2, 0.3])
    tq = c._fast_geometric_attitude_control(att=np.zeros(3), ang_vel=w, b3_des=np.array([0, 0, 1]), yaw_des=0.0, yaw_rate_des=0.0)
    np.testing.assert_allclose(tq, np.cross(w, np.array([0.0025, 0.006, 0.0135])), rtol=1e-10)
    full = np.array([[0.02, 0.001, 0.002], [0.001, 0.02, 0.003], [0.002, 0.003, 0.04]])
    c._fast_inertia = full
    tq = c._fast_geometric_attitude_control(np.zeros(3), w, np.array([0, 0, 1]), 0.0, 0.0)
    np.testing.assert_allclose(tq, np.cross(w, full @ w), rtol=1e-10)
    # the two attitude laws agree on a diagonal inertia; torque limits are applied and counted
    c = make(inertia=np.array([0.025, 0.03, 0.045]))
    st = DroneState(timestamp=0.0, position=np.zeros(3), velocity=np.zeros(3), attitude=np.zeros(3), angular_velocity=np.array([1.0, 2.0, 3.0]))
    _, t_full = c._geometric_attitude_control(st, np.array([0, 0, 1]), 0.0, 0.0, 10.0, 0.01)
    t_fast = c._fast_geometric_attitude_control(np.zeros(3), np.array([1.0, 2.0, 3.0]), np.array([0, 0, 1]), 0.0, 0.0)
    np.testing.assert_allclose(t_full, t_fast, rtol=1e-10)
    c = make(max_torque_xyz=np.array([1.0, 1.0, 2.0]))
    tq = c._fast_geometric_attitude_control(np.zeros(3), np.array([10.0, 10.0, 10.0]), np.array([0, 0, 1]), 0.0, 0.0)
    assert np.all(np.abs(tq) <= np.array([1.0, 1.0, 2.0])) and c._torque_saturation_count == int(np.sum(np.abs(c.unsaturated_torque) > np.array([1.0, 1.0, 2.0])))
    # per-axis integral clamp, clamping and back-calculation anti-windup with assigned members
    aw = dict(kp_pos=np.array([10.0, 10.0, 12.0]), ki_pos=np.array([0.5, 0.5, 1.0]), kd_pos=np.array([6.0, 6.0, 8.0]), max_thrust=20.0, min_thrust=0.5,
              max_integral_pos=5.0, max_integral_per_axis=np.array([2.0, 2.0, 3.0]), back_calculation_gain=0.1, integral_decay_factor=0.99, saturation_threshold=0.95)
    c = make(**aw)
    for _ in range(100):
        c._update_integral_error(np.array([10.0, 10.0, 10.0]), 0.01)
    assert np.all(np.abs(c.integral_vel_error) <= np.array([2.0, 2.0, 3.0]) + 1e-12)
    c = make(**aw)
    c._update_integral_error(np.array([1.0, 1.0, 1.0]), 0.01)
    free = c.integral_vel_error.copy()
    c.integral_vel_error = np.zeros(3)
    c._update_integral_error(np.array([1.0, 1.0, 1.0]), 0.01, thrust_saturated=True)
    np.testing.assert_allclose(c.integral_vel_error, 0.1 * free, rtol=1e-12)              # clamping: the update shrinks tenfold (controller.py:590-591)
    c = make(anti_windup_method="back_calculation", **aw)
    c.unsaturated_thrust = 25.0
    c.unsaturated_torque = np.array([6.0, 3.0, 3.0])
    c._update_integral_error(np.array([1.0, 1.0, 1.0]), 0.01, thrust_saturated=True, torque_saturated=np.array([True, False, False]))
    mt = np.asarray(c.config.max_torque_xyz, float)
    exp = np.array([0.01, 0.01, 0.01]) - (25.0 - 20.0) * 0.1 * np.array([0.33, 0.33, 0.34]) - np.array([(6.0 - mt[0]) * 0.1 * 0.5, 0.0, 0.0])
    np.testing.assert_allclose(c.integral_vel_error, exp, rtol=1e-12, atol=1e-15)
    assert abs(c.unsaturated_thrust - 25.0) == 0.0 and not c.last_thrust_saturated
    c.last_thrust_saturated = True; c.last_torque_saturated = np.array([True, False, True])
    assert c.last_thrust_saturated and c.last_torque_saturated.tolist() == [True, False, True]
    # yaw singularity: detection values and the fallbacks' orthonormal frames
    c = make()
    up = np.array([0.0, 0.0, 1.0])
    for z, sing in ((0.0, False), (0.95, True), (-0.95, True), (0.5, True), (0.1, True), (0.09, False)):
        s_, ca, method = c._detect_yaw_singularity(np.array([0.0, 0.0, z]), up)
        assert (s_, ca, method) == (sing, abs(z), "skip_yaw")
    c.config.default_heading_yaw = np.pi / 2
    for method, b3 in (("skip_yaw", np.array([0.1, 0.1, 0.99])), ("default_heading", up), ("maintain_current", np.array([0.1, 0.0, 0.995])), ("unknown_method", up)):
        b3 = b3 / np.linalg.norm(b3)
        b1, b2, b3o = c._handle_yaw_singularity(np.array([1.0, 0.0, 0.0]), b3, np.pi / 4, method)
        Rm = np.stack([b1, b2, b3o], 1)
        assert np.allclose(b3o, b3) and np.allclose(Rm.T @ Rm, np.eye(3), atol=1e-12), method


def test_controller_mirror_quaternion_states_reproduce_the_reference(gpu_ops, golden_controller):
    """Quaternion attitudes through the mirror against the commands the REFERENCE's controller returned for the same states
    (make_golden_controller.py block F: lengths 1, 3, 0.25, 1e-3 and, below the 1e-6 threshold, 1e-9 -> identity), float64 to 1e-9."""
    from dart_planner_amd.control.geometric_controller import GeometricController
    from dart_planner_amd.common.types import DroneState
    g, _ = golden_controller
    for i in range(len(g["quat_thrust"])):
        c = GeometricController(tuning_profile="sitl_optimized", precision="f64"); c._ops = gpu_ops
        st = DroneState(timestamp=5.0, position=g["quat_pos"][i], velocity=g["quat_vel"][i], attitude=g["quat_quat"][i], angular_velocity=g["quat_omega"][i])
        cmd = c.compute_control(st, g["quat_dpos"][i], g["quat_dvel"][i], g["quat_dacc"][i], float(g["quat_yaw"][i]), float(g["quat_yaw_rate"][i]))
        assert abs(cmd.thrust - g["quat_thrust"][i]) <= 1e-9 * abs(g["quat_thrust"][i]), i
        assert np.max(np.abs(np.asarray(cmd.torque) - g["quat_torque"][i])) <= 1e-9, i


def test_controller_mirror_reset_and_quaternion_states(gpu_ops):
    """(1) reset() after a failsafe: the reference's reset (controller.py:853-869) clears the integral, the clock and the failsafe flags but
    NOT the gains its failsafe halved in place on self.config (:817-821) -- the mirror's halving count (word 10 of the device record)
    survives.  (2) A quaternion attitude (controller.py:785-803: normalised; identity below 1e-6) gives the command of the same attitude
    in Euler angles, whatever the quaternion's length."""
    from dart_planner_amd.control.geometric_controller import GeometricController
    from dart_planner_amd.common.types import DroneState
    c = GeometricController(tuning_profile="sitl_optimized"); c._ops = gpu_ops
    st = DroneState(timestamp=1.0, position=np.array([0.0, 0.0, 1.0]), velocity=np.zeros(3), attitude=np.zeros(3), angular_velocity=np.zeros(3))
    c.compute_control(st, np.array([0.5, 0.0, 1.0]), np.zeros(3), np.zeros(3))
    c._set_words(10, [2.0])                                      # two failsafe halvings happened
    c._set_words(0, [0.3, -0.2, 0.1]); c._set_flag_bits(1, 1)
    c.reset()
    assert c._word(10) == 2.0 and np.all(c.integral_vel_error == 0) and np.isnan(c._word(3)) and not (int(c._word(11)) & 1)
    fresh = GeometricController(tuning_profile="sitl_optimized"); fresh._ops = gpu_ops
    fresh._set_words(10, [2.0])
    a = c.compute_control(st, np.array([0.5, 0.0, 1.0]), np.zeros(3), np.zeros(3))
    b = fresh.compute_control(st, np.array([0.5, 0.0, 1.0]), np.zeros(3), np.zeros(3))
    assert a.thrust == b.thrust and np.array_equal(np.asarray(a.torque), np.asarray(b.torque))
    # quaternion attitudes
    roll, pitch, yaw = 0.2, -0.1, 0.7
    cr, sr, cp_, sp_, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    quat = np.array([cr * cp_ * cy + sr * sp_ * sy, sr * cp_ * cy - cr * sp_ * sy, cr * sp_ * cy + sr * cp_ * sy, cr * cp_ * sy - sr * sp_ * cy])
    out = []
    for att in (np.array([roll, pitch, yaw]), quat, 3.0 * quat, 1e-9 * quat):
        g = GeometricController(tuning_profile="sitl_optimized"); g._ops = gpu_ops
        s2 = DroneState(timestamp=1.0, position=np.array([0.0, 0.0, 1.0]), velocity=np.array([0.1, 0.0, 0.0]), attitude=att, angular_velocity=np.array([0.01, 0.02, 0.03]))
        cmd = g.compute_control(s2, np.array([0.5, 0.2, 1.2]), np.zeros(3), np.zeros(3))
        out.append(np.concatenate([[cmd.thrust], np.asarray(cmd.torque, float)]))
    np.testing.assert_allclose(out[1], out[0], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(out[2], out[0], rtol=1e-12, atol=1e-14)          # the length of the quaternion does not matter
    ident = GeometricController(tuning_profile="sitl_optimized"); ident._ops = gpu_ops
    s3 = DroneState(timestamp=1.0, position=np.array([0.0, 0.0, 1.0]), velocity=np.array([0.1, 0.0, 0.0]), attitude=np.zeros(3), angular_velocity=np.array([0.01, 0.02, 0.03]))
    cmd = ident.compute_control(s3, np.array([0.5, 0.2, 1.2]), np.zeros(3), np.zeros(3))
    np.testing.assert_allclose(out[3], np.concatenate([[cmd.thrust], np.asarray(cmd.torque, float)]), rtol=1e-12, atol=1e-14)   # |q| < 1e-6: identity


def test_closed_loop_reproduces_reference_loops(gpu_ops, golden_controller):
    data, meta = golden_controller
    worst = cc.check_closed_loops_golden(harness(gpu_ops, np.float64), data, meta)
    print(f"closed loops vs the reference: worst state error {worst:.2e}")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_closed_loop_random_batch_vs_oracle(gpu_ops, dt):
    worst = cc.check_closed_loop_vs_oracle(harness(gpu_ops, dt), B=4096, N=12, nsteps=40, seed=3)
    print(f"4096 drones x 40 steps, {np.dtype(dt).name}: worst state error vs the oracle {worst:.2e}")
    if dt == np.float64:
        cc.check_closed_loop_vs_oracle(harness(gpu_ops, dt), B=130, N=12, nsteps=40, seed=4, per_drone_plans=False)


def test_simulator_step_matches_reference(gpu_ops, golden_controller):
    import torch
    from dart_planner_amd.capi import SimulatorParams
    data, _ = golden_controller
    d = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to("cuda:0")
    for i in range(len(data["s_thrust"])):
        sp = SimulatorParams.reference_defaults(max_thrust=float(data["s_max"][i, 0]), max_torque=float(data["s_max"][i, 1]))
        t, pos, vel, att, om = d([3.0 + i]), d(data["s_pos"][i][None]), d(data["s_vel"][i][None]), d(data["s_att"][i][None]), d(data["s_omega"][i][None])
        gpu_ops.simulator_step(sp, t, pos, vel, att, om, d([data["s_thrust"][i]]), d(data["s_torque"][i][None]), float(data["s_dt"][i]), wind=d(data["s_wind"][i]))
        got = np.concatenate([a.cpu().numpy().ravel() for a in (pos, vel, att, om, t)])
        assert np.max(np.abs(got - data["s_out"][i])) <= 1e-13, i


def test_plan_sampler_matches_reference(gpu_ops, golden_controller):
    """se3mpc_control_plan_*'s target output == OnboardController._interpolate_trajectory on the reference's own query times
    (knots, mid-points, before / after the plan, 1e-12 past a knot)."""
    import torch
    from dart_planner_amd.capi import ControllerParams
    data, _ = golden_controller
    d = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to("cuda:0")
    cp = ControllerParams.from_config(co.ControllerConfig())
    tq = data["i_tq"]
    B = len(tq)
    z = d(np.zeros((B, 3)))
    out = gpu_ops.control_plan(cp, gpu_ops.controller_state(cp, B), d(tq), d(tq), z, z, z, z, d(data["i_ts"]), d(data["i_P"]), d(data["i_V"]), d(data["i_A"]),
                               want_target=True)
    tg = out["target"].cpu().numpy()
    assert np.array_equal(tg[:, 0:3], data["i_pos"]) and np.array_equal(tg[:, 3:6], data["i_vel"]) and np.array_equal(tg[:, 6:9], data["i_acc"])
    out = gpu_ops.control_plan(cp, gpu_ops.controller_state(cp, 8), d(tq[:8]), d(tq[:8]), z[:8], z[:8], z[:8], z[:8], d(data["i_ts"]), d(data["i_P"]), want_target=True)
    tg = out["target"].cpu().numpy()
    assert np.array_equal(tg[:, 0:3], data["i_pos_only"]) and not tg[:, 3:].any()


def monte_carlo(ops, prm, cp, sp, p0, v0, goal, cycles, substeps, sim_dt, wind, dtype, log=False):
    """The product's receding-horizon Monte-Carlo (dart_planner_amd/control/closed_loop.py): per cycle ONE se3mpc_solve_* launch and ONE
    se3mpc_closed_loop_* launch, plans read in place from the solver's outputs."""
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    r = ClosedLoopMonteCarlo(ops, prm, cp, sp).run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind, log=log)
    return r["pos"], r["vel"], r["att"], r["omega"], r["time"], r["controller_state"], r["logs"]


def test_monte_carlo_closed_loop_on_device(gpu_ops):
    """BASELINE.json config 5's named test shape (reference tests/test_monte_carlo_sim.py: SIM_DURATION 5 s, DT 0.15 s -> 33
    planning cycles from p = (0,0,2) towards (8,0,5), random wind per run), with the contract's controller in the loop at 100 Hz
    (15 control + simulator steps per cycle) for 4096 runs at once.  A 48-run sample is replayed cycle by cycle with the oracle
    (SciPy solve + NumPy controller / simulator) from the device's own states; the full batch is checked through invariants."""
    import torch
    from dart_planner_amd.capi import ControllerParams, Params, SimulatorParams
    ops = gpu_ops
    dev = ops.be.device
    S, cycles, substeps, sim_dt = 4096, 33, 15, 0.01
    prm = Params.reference_defaults()                                 # the DI planner: horizon 6, dt 1/400
    cfg = co.ControllerConfig()
    cp, sp = ControllerParams.from_config(cfg), SimulatorParams.reference_defaults()
    g = torch.Generator(device=dev); g.manual_seed(5)
    dtype = torch.float64
    p0 = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev).repeat(S, 1) + 0.2 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    v0 = 0.3 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    goal = torch.tensor([8.0, 0.0, 5.0], dtype=dtype, device=dev).repeat(S, 1).contiguous()
    wind = (torch.rand(S, 1, dtype=dtype, device=dev, generator=g) * 1.5) * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)   # wind_std ~ U(0, 1.5)
    wind = wind.contiguous()
    pos, vel, att, om, time, st, logs = monte_carlo(ops, prm, cp, sp, p0, v0, goal, cycles, substeps, sim_dt, wind, dtype, log=True)
    torch.cuda.synchronize()
    # invariants on all 4096 runs
    assert float((time - cycles * substeps * sim_dt).abs().max()) <= 1e-9
    assert torch.isfinite(pos).all() and torch.isfinite(vel).all()
    taken = torch.stack([o["steps_taken"] for _, o in logs])
    assert int(taken.min()) == substeps == int(taken.max())
    # the simulator's translation ignores attitude (simulator.py:59): x / y only move with the wind
    drift = (pos[:, :2] - p0[:, :2] - v0[:, :2] * 4.95).abs().max()
    expect = (wind[:, :2].abs().max() / 1.5) * 0.5 * 4.95 ** 2
    assert float(drift) <= float(expect) * 1.05 + 1e-6
    # 48 runs replayed with the oracle, cycle by cycle, each cycle FROM THE DEVICE'S OWN state (so the comparison is per cycle: one
    # SciPy solve and 15 NumPy control / simulator steps against one solve launch and one closed-loop launch)
    pick = np.arange(0, S, S // 48)[:48]
    ocfg = orc.OracleConfig()
    sim = co.SimulatorConfig()
    k = np.arange(6)
    worst_plan = worst_state = 0.0
    h = lambda a: a.cpu().numpy()
    for c in range(cycles):
        sol, out = logs[c]
        ls, lt = h(out["log_state"])[:, pick], h(out["log_time"])[:, pick]
        X = h(sol["x"])[pick]; info = ops.info_to_host(sol["info"])[pick]
        start = ls[0]
        acc = []
        for j in range(len(pick)):
            xr, ir = orc.solve(start[j, 0:3], start[j, 3:6], h(goal)[0], ocfg)
            assert (int(info["nit"][j]), int(info["nfev"][j]), int(info["status"][j])) == (ir["nit"], ir["nfev"], ir["status"]), (c, j)
            worst_plan = max(worst_plan, float(np.max(np.abs(X[j, :18] - xr[:18]))))
            acc.append(orc.extract_solution(xr, ocfg)["accelerations"])
        assert worst_plan <= 1e-9
    # one full replay of the first 3 cycles' control / simulator steps from the logged controller members would need the members
    # per cycle; instead the closed-loop launch itself is checked against the oracle in test_closed_loop_random_batch_vs_oracle and
    # here through the end state of cycle 0 (fresh controller): plan of cycle 0 -> 15 steps
    sol, out = logs[0]
    X = h(sol["x"])[pick]
    P, V, A = X[:, :18].reshape(-1, 6, 3), X[:, 18:36].reshape(-1, 6, 3), h(sol["accelerations"])[pick]
    ts = 0.0 + k * prm.dt
    fin, log = co.closed_loop(cfg, sim, co.ControllerState(len(pick), cfg), h(p0)[pick], h(v0)[pick], np.zeros((len(pick), 3)), np.zeros((len(pick), 3)),
                              np.zeros(len(pick)), ts, P, V, A, substeps, sim_dt, wind=h(wind)[pick], stop_at_plan_end=False)
    ref = np.concatenate([log["pos"], log["vel"], log["att"], log["omega"]], axis=2)
    worst_state = float(np.max(np.abs(h(out["log_state"])[:, pick] - ref)))
    assert worst_state <= 1e-8
    dist = (pos - goal).norm(dim=1)
    print(f"Monte-Carlo 4096 x 33 cycles x 15 steps on device: plans vs SciPy {worst_plan:.2e} m, first-cycle states vs oracle {worst_state:.2e}; "
          f"final distance to goal: median {float(dist.median()):.2f} m (the reference's simulator has no lateral authority)")


def test_monte_carlo_f32_tracks_f64(gpu_ops):
    """The same Monte-Carlo in float32 (production precision): median end-state deviation from the f64 run stays small; runs near a
    controller branch may part ways (reported, bounded)."""
    import torch
    from dart_planner_amd.capi import ControllerParams, Params, SimulatorParams
    ops = gpu_ops
    dev = ops.be.device
    S, cycles, substeps, sim_dt = 1024, 33, 15, 0.01
    prm = Params.reference_defaults()
    cp, sp = ControllerParams.from_config(co.ControllerConfig()), SimulatorParams.reference_defaults()
    g = torch.Generator(device=dev); g.manual_seed(6)
    p0 = torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64, device=dev).repeat(S, 1) + 0.2 * torch.randn(S, 3, dtype=torch.float64, device=dev, generator=g)
    v0 = 0.3 * torch.randn(S, 3, dtype=torch.float64, device=dev, generator=g)
    goal = torch.tensor([8.0, 0.0, 5.0], dtype=torch.float64, device=dev).repeat(S, 1).contiguous()
    wind = torch.randn(S, 3, dtype=torch.float64, device=dev, generator=g).contiguous()
    r64 = monte_carlo(ops, prm, cp, sp, p0, v0, goal, cycles, substeps, sim_dt, wind, torch.float64)
    f = lambda a: a.float().contiguous()
    r32 = monte_carlo(ops, prm, cp, sp, f(p0), f(v0), f(goal), cycles, substeps, sim_dt, f(wind), torch.float32)
    err = (r32[0].double() - r64[0]).abs().max(dim=1).values
    print(f"f32 vs f64 Monte-Carlo end positions: median {float(err.median()):.2e} m, 95 % {float(err.quantile(0.95)):.2e} m, max {float(err.max()):.2e} m")
    assert float(err.median()) <= 5e-3 and float(err.quantile(0.95)) <= 0.25


# ------------------------------------------------------------------ f-3: a device-solved plan on the wire
def _reference_envelope_verify(raw: bytes, secret: str):
    """The receiving side of the reference's envelope, restated from its rules
    (/root/reference/src/dart_planner/communication/secure_serializer.py:92-167): the message is JSON with exactly the fields
    (data, signature, timestamp, message_id); the signature is HMAC-SHA256(secret, f"{json.dumps(data)}:{timestamp}:{message_id}")
    as lowercase hex, where `data` is re-dumped from the PARSED message with json's default separators.  Returns data."""
    import hashlib
    import hmac
    msg = json.loads(raw.decode("utf-8"))
    assert set(msg) == {"data", "signature", "timestamp", "message_id"}
    expect = hmac.new(secret.encode("utf-8"), f"{json.dumps(msg['data'])}:{msg['timestamp']}:{msg['message_id']}".encode("utf-8"),
                      hashlib.sha256).hexdigest()
    assert hmac.compare_digest(msg["signature"], expect), "signature"
    return msg["data"]


def test_device_plan_travels_in_the_reference_envelope(gpu_ops):
    """Plan on the MI355X, put the Trajectory on the wire with this package's SecureSerializer, and check the bytes with a verifier
    written from the reference's envelope rules -- a verifier that is first proven on messages the reference's own serializer signed
    (tests/golden/wire_messages.json) and on tampered copies of them."""
    from dart_planner_amd.common.types import DroneState
    from dart_planner_amd.communication.secure_serializer import SecureSerializer, trajectory_from_wire
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCPlanner
    g = json.load(open(os.path.join(GOLDEN, "wire_messages.json")))
    for m in g["messages"]:                                   # the verifier accepts what the reference signed ...
        raw = m["raw"].encode("utf-8")
        _reference_envelope_verify(raw, g["secret"])
        bad = raw.replace(b'"timestamp": ', b'"timestamp": 1', 1)
        with pytest.raises(AssertionError):                   # ... and rejects a tampered copy and a wrong key
            _reference_envelope_verify(bad, g["secret"])
        with pytest.raises(AssertionError):
            _reference_envelope_verify(raw, g["secret"] + "x")
    pl = SE3MPCPlanner(precision="f64")
    tr = pl.plan_trajectory(DroneState(timestamp=0.0, position=np.array([0.0, 0.0, 1.0]), velocity=np.zeros(3)), np.array([5.0, 3.0, 2.0]))
    assert pl._get_ops().lib.path.endswith("libse3mpc.so") and pl.last_result["nfev"] == 3
    ser = SecureSerializer(secret_key=g["secret"], message_ttl=300)
    raw = ser.serialize({"status": "ok", "trajectory": tr})                      # the cloud handler's reply (cloud/main_improved.py:87)
    data = _reference_envelope_verify(raw, g["secret"])
    back = trajectory_from_wire(data["trajectory"])
    for f in ("timestamps", "positions", "velocities", "accelerations", "attitudes", "body_rates", "thrusts", "yaws", "yaw_rates"):
        assert np.array_equal(np.asarray(getattr(back, f)), np.asarray(getattr(tr, f))), f     # repr round trip of float64: exact
    assert np.max(np.abs(back.positions[0] - [2.1897985430479023, 2.1897985430479023, 3.1679005576174233])) <= 1e-9
    # and this package's own receiving side agrees
    assert np.array_equal(trajectory_from_wire(ser.deserialize(raw)["trajectory"]).positions, tr.positions)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_monte_carlo_in_one_launch_equals_the_two_launch_form(gpu_ops, prec):
    """se3mpc_monte_carlo_*: every planning cycle of every drone inside ONE kernel (each drone pays only for its own slow solves) ==
    alternating se3mpc_solve_* and se3mpc_closed_loop_* (ClosedLoopMonteCarlo.run), BIT FOR BIT -- it is the same code: BASELINE config 5's
    named shape (4096 runs x 33 cycles x 15 steps), ragged batches at other horizons (33: the smallest with 64 lanes per drone), shared /
    no wind."""
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    dtype = torch.float32 if prec == "f32" else torch.float64
    dev = gpu_ops.be.device
    for N, B, cycles, substeps in ((6, 4096, 33, 15), (13, 77, 6, 7), (30, 131, 5, 4), (33, 2, 2, 3)):
        mc = ClosedLoopMonteCarlo(gpu_ops, Params.reference_defaults(horizon=N))
        g = torch.Generator(device=dev); g.manual_seed(5)
        p0 = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev).repeat(B, 1) + 0.2 * torch.randn(B, 3, dtype=dtype, device=dev, generator=g)
        v0 = 0.3 * torch.randn(B, 3, dtype=dtype, device=dev, generator=g)
        goal = torch.tensor([8.0, 0.0, 5.0], dtype=dtype, device=dev).repeat(B, 1).contiguous()
        wind = torch.randn(B, 3, dtype=dtype, device=dev, generator=g).contiguous()
        for w in (wind, None, wind[0].contiguous()):
            a = mc.run(p0, v0, goal, cycles, substeps, 0.01, wind=w)
            b = mc.run_fused(p0, v0, goal, cycles, substeps, 0.01, wind=w, want_last_plan=True)
            for key in ("pos", "vel", "att", "omega", "time", "controller_state"):
                assert torch.equal(a[key], b[key]), (N, B, key)
            assert torch.isfinite(b["pos"]).all() and float((b["pos"] - p0).abs().max()) > 1e-3
        info = gpu_ops.info_to_host(b["last_plan"]["info"])
        assert set(np.unique(info["status"])) <= {0, 1, 2} and info["nit"].min() >= 1


def test_monte_carlo_hipgraph_replay_equals_eager(gpu_ops):
    """The library never allocates or synchronises, so the whole receding-horizon Monte-Carlo (66 launches) captures into one hipGraph;
    a replay with new initial conditions equals the eager run bit for bit."""
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    ops = gpu_ops
    dev = ops.be.device
    S, cycles, substeps, sim_dt = 512, 8, 15, 0.01
    mc = ClosedLoopMonteCarlo(ops, Params.reference_defaults())
    replay = mc.capture(S, torch.float32, cycles, substeps, sim_dt)
    g = torch.Generator(device=dev); g.manual_seed(11)
    for trial in range(2):
        p0 = torch.tensor([0.0, 0.0, 2.0], device=dev).repeat(S, 1) + 0.3 * torch.randn(S, 3, device=dev, generator=g)
        v0 = 0.3 * torch.randn(S, 3, device=dev, generator=g)
        goal = (torch.tensor([8.0, 0.0, 5.0], device=dev) + torch.randn(S, 3, device=dev, generator=g)).contiguous()
        wind = torch.randn(S, 3, device=dev, generator=g)
        eager = mc.run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind)
        out = replay(p0, v0, goal, wind)
        torch.cuda.synchronize()
        for k in ("pos", "vel", "att", "omega", "time", "controller_state"):
            assert torch.equal(out[k], eager[k]), (trial, k)


def test_closed_loop_refuses_strides_that_leave_the_storage(gpu_ops):
    """Explicit plan strides read past the views' shapes; a stride that would run off the tensor's storage is refused on the host, before any
    launch (an out-of-bounds read on the device can take the whole node down)."""
    import torch
    from dart_planner_amd.capi import ControllerParams, SimulatorParams
    ops = gpu_ops
    dev = ops.be.device
    cp, sp = ControllerParams.from_config(co.ControllerConfig()), SimulatorParams.reference_defaults()
    B, N = 8, 6
    X = torch.zeros(B, 9 * N, dtype=torch.float64, device=dev)
    acc = torch.zeros(B, N, 3, dtype=torch.float64, device=dev)
    z = torch.zeros(B, 3, dtype=torch.float64, device=dev)
    t = torch.zeros(B, dtype=torch.float64, device=dev)
    ts = torch.arange(N, dtype=torch.float64, device=dev) / 400
    st = ops.controller_state(cp, B)
    ops.closed_loop(cp, sp, st, t, z.clone(), z.clone(), z.clone(), z.clone(), ts, X, X[:, 3 * N:], acc, nsteps=2, strides=(9 * N, 9 * N, 3 * N))   # legal
    with pytest.raises(ValueError, match="storage"):
        ops.closed_loop(cp, sp, st, t, z.clone(), z.clone(), z.clone(), z.clone(), ts, X, X[:, 3 * N:], acc, nsteps=2, strides=(9 * N, 9 * N, 9 * N))  # acc is 3N wide
    with pytest.raises(ValueError, match="storage"):
        ops.closed_loop(cp, sp, st, t, z.clone(), z.clone(), z.clone(), z.clone(), ts, X[:4], X[:, 3 * N:], acc, nsteps=2, strides=(19 * N, 9 * N, 3 * N))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_plan_operand_rules_of_every_entry_point(gpu_ops, dt):
    cc.check_plan_rules(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_front_ends_refuse_wrong_operands_before_any_launch(gpu_ops, dt, monkeypatch):
    cc.check_operand_rules(harness(gpu_ops, dt), monkeypatch)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_monte_carlo_in_one_launch_equals_the_two_launch_form_with_a_different_constant_in_every_block(gpu_ops, prec):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import torch
    import param_sets as ps
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    dtype = torch.float32 if prec == "f32" else torch.float64
    dev = gpu_ops.be.device
    L = ps.LOOP_SHAPE
    b = ps.loop_blocks(L["N"])
    mc = ClosedLoopMonteCarlo(gpu_ops, b["prm"], b["cp"], b["sp"])
    g = torch.Generator(device=dev); g.manual_seed(5)
    B = L["B"]
    p0 = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev).repeat(B, 1) + 0.2 * torch.randn(B, 3, dtype=dtype, device=dev, generator=g)
    v0 = 0.3 * torch.randn(B, 3, dtype=dtype, device=dev, generator=g)
    goal = torch.tensor([8.0, 0.0, 5.0], dtype=dtype, device=dev).repeat(B, 1).contiguous()
    wind = torch.randn(B, 3, dtype=dtype, device=dev, generator=g).contiguous()
    a = mc.run(p0, v0, goal, L["cycles"], L["substeps"], 0.01, wind=wind)
    f = mc.run_fused(p0, v0, goal, L["cycles"], L["substeps"], 0.01, wind=wind, want_last_plan=True)
    for key in ("pos", "vel", "att", "omega", "time", "controller_state"):
        assert torch.equal(a[key], f[key]), key
    assert torch.isfinite(f["pos"]).all() and float((f["pos"] - p0).abs().max()) > 1e-3
