"""Checks of the MotorMixer / motor model kernels (dart_planner_amd/csrc/mixer.hip) that take a harness (tests/parity_checks.Harness): run by
tests/test_emu_mixer.py on the host emulation and by tests/test_gpu_mixer.py on the device.

References: tests/golden/mixer_cases.npz (the reference's own classes, tests/golden/make_golden_mixer.py) and tests/mixer_oracle.py (pinned to
those vectors by tests/test_mixer_oracle_golden.py).

Bounds.  float64: 1e-9 per call and per loop step; flags, event counts and which record is written exact.  float32 per call: PWMs, motor
thrusts, allocations and wrenches 1e-4 absolute (tests/parity_checks.py's float32 bound), rpm and motor torque 5e-6 relative (values up to
1e4 and 1e2: a few float32 roundings of a three-operation chain), flags exact -- every recorded or drawn row keeps a relative margin of 1e-3
from each threshold (mixer_oracle.margin), four orders above float32's rounding.  float32 closed loops: the bound of
controller_checks.check_closed_loop_vs_oracle (median over the loops of the largest state error <= 5e-3, at least 90 % of them <= 5e-2)."""
import json
import os

import numpy as np

import mixer_oracle as mo
from dart_planner_amd.capi import MIXER_STATE_WORDS, MixerParams, SmootherParams
from smoother_checks import Dev, _loop_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 1e-3
READBACK = ("motor_thrust", "motor_torque", "motor_rpm", "allocation", "wrench")
_cache = {}


def golden():
    """The fixtures, loaded once and shared (read-only)."""
    if "g" not in _cache:
        z = np.load(os.path.join(GOLDEN, "mixer_cases.npz"))
        data = {k: z[k] for k in z.files}
        for v in data.values():
            v.setflags(write=False)
        _cache["g"] = (data, json.load(open(os.path.join(GOLDEN, "mixer_cases.json"))))
    return _cache["g"]


def tol(h):
    return 1e-9 if h.dt == np.float64 else 1e-4


def rel_tol(h):
    return 1e-12 if h.dt == np.float64 else 5e-6


def capi_params(p) -> MixerParams:
    """The oracle's parameter dict as se3mpc_mixer_params."""
    motors = [{k: p[k][i] for k in mo.MOTOR_FIELDS} for i in range(4)]
    return MixerParams.from_matrices(p["mixing"], p["inverse"], motors, p["config_pwm_min"], p["config_pwm_max"], p["config_pwm_idle"], p["max_thrust"],
                                     p["body_rate_scale"], p["watchdog_threshold"])


def seq_params(data, seq):
    """The oracle parameters of a golden sequence (the kernel is given the GOLDEN inverse matrix)."""
    motors = [dict(zip(mo.MOTOR_FIELDS, data[seq["key"] + "motors"][:, i])) for i in range(4)]
    return mo.params(data[seq["key"] + "B"], data[seq["key"] + "inverse"], motors, seq["config_pwm_min"], seq["config_pwm_max"], seq["config_pwm_idle"],
                     seq["max_thrust"], seq["body_rate_scale"], seq["watchdog_threshold"])


def host(h, a):
    return np.array(h.to_host(a))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def close(got, ref, h, rel=False):
    """Largest error of got against ref: absolute, or relative to max(|ref|, 1)."""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    e = np.abs(got - ref) / (np.maximum(np.abs(ref), 1.0) if rel else 1.0)
    return float(np.nanmax(e)) if e.size and not np.all(np.isnan(e)) else 0.0


# ---------------------------------------------------------------------------------------------- golden sequences through the C ABI
def check_golden_sequences(h, only=None):
    """Every recorded mix_commands call of the reference: PWMs, flags, the record, then the forward model and get_control_allocation."""
    data, meta = golden()
    dv, ops, worst = Dev(h), h.ops, {}
    for seq in meta["sequences"]:
        if only is not None and seq["tag"] not in only:
            continue
        key = seq["key"]
        mp = capi_params(seq_params(data, seq))
        st = ops.mixer_state(1)
        err = rerr = 0.0
        for e in range(seq["calls"]):
            out = ops.mixer_mix(mp, dv.r(data[key + "thrust"][e][None]), dv.r(data[key + "torque"][e][None]), st)
            pwm, fl, rec = host(h, out["pwm"]).astype(float)[0], int(host(h, out["flags"])[0]), host(h, st).astype(float)[0]
            ref = data[key + "state"][e]
            assert fl == int(data[key + "flags"][e]), (seq["tag"], e, fl, int(data[key + "flags"][e]))
            assert rec[0] == ref[0], (seq["tag"], e, rec[0], ref[0])                              # saturation_events: exact
            if fl & mo.NON_FINITE:
                assert np.all(np.isnan(pwm))
            else:
                assert np.array_equal(rec[1:5], pwm)                                                # last_motor_commands IS what the call returned
            err = max(err, close(pwm, data[key + "pwm"][e], h), close(rec[1:5], ref[1:5], h))
            rb = ops.mixer_readback(mp, dv.r(rec[None, 1:5]))
            for nm in ("motor_thrust", "allocation"):
                err = max(err, close(host(h, rb[nm])[0], data[key + nm][e], h))
            for nm in ("motor_torque", "motor_rpm"):
                rerr = max(rerr, close(host(h, rb[nm])[0], data[key + nm][e], h, rel=True))
        assert int(host(h, st)[0, 0]) == seq["final_events"]
        worst[seq["tag"]] = (err, rerr)
    print("mixer golden sequences, largest (absolute, relative) error per sequence:", {k: (float("%.3g" % a), float("%.3g" % r)) for k, (a, r) in worst.items()})
    bad = {k: v for k, v in worst.items() if not (v[0] <= tol(h) and v[1] <= max(rel_tol(h), 1e-9))}
    assert not bad, bad
    return worst


def check_golden_matrices_and_defaults(h):
    """se3mpc_mixer_default_params against the reference's X factory at arm length 0.15 (1e-12 relative on both matrices, the other fields
    exact), the Python defaults against the library's, and the golden matrices' own consistency."""
    data, meta = golden()
    lib = h.ops.lib
    d = lib.mixer_default_params()
    B, inv = np.array(d.mixing).reshape(4, 4), np.array(d.inverse).reshape(4, 4)
    for got, ref in ((B, data["mat_x_0.15_B"]), (inv, data["mat_x_0.15_inverse"])):
        assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)) <= 1e-12, (got, ref)
    for k in mo.MOTOR_FIELDS:
        assert list(getattr(d, k)) == [mo.DEFAULT_MOTOR[k]] * 4, k
    assert (d.config_pwm_min, d.config_pwm_max, d.config_pwm_idle, d.max_thrust, d.body_rate_scale, d.watchdog_threshold) == (0.0, 1.0, 0.1, 10.0, 2.0, 5.0)
    py = MixerParams.reference_defaults()
    assert bytes(py)[256:] == bytes(d)[256:] and np.max(np.abs(np.array(py.inverse) - np.array(d.inverse))) <= 1e-12 and list(py.mixing) == list(d.mixing)
    ranks = {m["tag"]: m["rank"] for m in meta["matrices"]}
    assert ranks == {"x_0.10": 4, "x_0.15": 4, "x_0.25": 4, "plus_0.15": 3}, ranks
    p = mo.default_params()
    for m in meta["matrices"][:3]:
        arm = float(m["tag"][2:])
        assert np.allclose(mo.mixing_matrix(p, mo.x_positions(arm), [1, -1, 1, -1]), data[f"mat_{m['tag']}_B"], rtol=1e-13, atol=0)


def check_golden_body_rate(h):
    """_convert_to_body_rate_cmd on the recorded commands, the watchdog bit where the reference's loop would trip."""
    data, meta = golden()
    dv, ops, br = Dev(h), h.ops, meta["body_rate"]
    p = mo.default_params(max_thrust=br["max_thrust"], body_rate_scale=br["body_rate_scale"], watchdog_threshold=br["watchdog_threshold"])
    p["inverse"] = data["mat_x_0.15_inverse"]
    mp, st = capi_params(p), ops.mixer_state(1)
    err, first = 0.0, None
    for e in range(data["br_thrust"].shape[0]):
        out = ops.mixer_mix(mp, dv.r(data["br_thrust"][e][None]), dv.r(data["br_torque"][e][None]), st, want_body_rate=True)
        err = max(err, close(host(h, out["body_rate"])[0], data["br_out"][e], h), close(host(h, out["pwm"])[0], data["br_pwm"][e], h))
        assert host(h, st)[0, 0] == data["br_state"][e, 0]
        tripped = bool(int(host(h, out["flags"])[0]) & mo.WATCHDOG)
        assert tripped == (data["br_state"][e, 0] > br["watchdog_threshold"])
        first = e if tripped and first is None else first
    print("mixer body-rate commands, largest error %.3g, watchdog from call %s" % (err, first))
    assert err <= tol(h) and first == br["tripped_after"]


def run_golden_loop(h, loop):
    """One recorded closed loop through closed_loop_actuated (the smoothed one: three plans, 100 steps each) -> logs."""
    data, _ = golden()
    dv, ops, key = Dev(h), h.ops, loop["key"]
    cp, sp, sp_mp = ops.lib.controller_default_params(), ops.lib.simulator_default_params(), SmootherParams.reference_defaults()
    p = mo.default_params()
    p["inverse"] = data["mat_x_0.15_inverse"]
    mp = capi_params(p)
    st, mx = ops.controller_state(cp, 1), ops.mixer_state(1)
    time, pos, vel = dv.d([data[key + "t"][0]]), dv.r(data[key + "pos"][0][None]), dv.r(data[key + "vel"][0][None])
    att, om = dv.r(data[key + "att"][0][None]), dv.r(data[key + "omega"][0][None])
    health = None if loop["health"] is None else dv.r(loop["health"])
    logs = []
    if loop["plans"] == 0:                       # a standing target: two equal rows, which every sampler returns as they are
        t0 = float(data[key + "t"][0])
        plan = (dv.d([t0, t0 + 1000.0]), dv.r(np.array([loop["hold"], loop["hold"]])), dv.r(np.zeros((2, 3))), dv.r(np.zeros((2, 3))))
        logs.append(ops.closed_loop_actuated(mp, cp, sp, st, mx, time, pos, vel, att, om, *plan, nsteps=loop["nsteps"], sim_dt=loop["sim_dt"], motor_health=health,
                                             log=True))
    else:
        sm, old = ops.smoother_state(1), None
        for c in range(loop["plans"]):
            new = dv.plan(tuple(data[f"{key}pl{c}_{x}"] for x in ("ts", "P", "V", "A")))
            ops.smoother_update(sp_mp, sm, time, *new, old=old)
            logs.append(ops.closed_loop_actuated(mp, cp, sp, st, mx, time, pos, vel, att, om, *new, nsteps=100, sim_dt=loop["sim_dt"], smoother=sp_mp,
                                                 smoother_state=sm, motor_health=health, log=True))
            old = new
    cat = lambda nm: np.concatenate([host(h, l[nm]).astype(float)[:, 0] for l in logs])
    final = np.concatenate([host(h, a).astype(float)[0] for a in (pos, vel, att, om)] + [host(h, time)])
    return dict(state=cat("log_state"), cmd=cat("log_cmd"), time=cat("log_time"), target=cat("log_target"), pwm=cat("log_pwm"), wrench=cat("log_wrench"),
                mixer=host(h, mx).astype(float)[0], final=final)


def check_golden_loops(h):
    data, meta = golden()
    errs = []
    for loop in meta["loops"]:
        key = loop["key"]
        got = run_golden_loop(h, loop)
        ref_state = np.concatenate([data[key + "pos"], data[key + "vel"], data[key + "att"], data[key + "omega"]], axis=1)
        ref_cmd = np.concatenate([data[key + "thrust"][:, None], data[key + "torque"]], axis=1)
        e = dict(state=np.max(np.abs(got["state"] - ref_state)), cmd=np.max(np.abs(got["cmd"] - ref_cmd)), target=np.max(np.abs(got["target"] - data[key + "target"])),
                 time=np.max(np.abs(got["time"] - data[key + "t"])), pwm=np.max(np.abs(got["pwm"] - data[key + "pwm"])),
                 wrench=np.max(np.abs(got["wrench"] - data[key + "wrench"])), final=np.max(np.abs(got["final"] - data[key + "final"])),
                 record=np.max(np.abs(got["mixer"] - data[key + "mixer_final"])))
        print("mixer golden loop", loop["tag"], {k: float("%.3g" % v) for k, v in e.items()})
        errs.append(e)
        assert e["time"] <= 1e-9 and got["mixer"][0] == data[key + "mixer_final"][0]
        if h.dt == np.float64:
            assert max(e.values()) <= 1e-9, (loop["tag"], e)
    if h.dt == np.float32:
        worst = np.array([e["state"] for e in errs])
        assert np.median(worst) <= 5e-3 and np.mean(worst <= 5e-2) >= 0.9, worst
    return errs


# ---------------------------------------------------------------------------------------------- random batches against the oracle
MODELS = ("default", "linear", "dead_and_linear", "disc_negative", "high_motor_limit", "mixed")


def random_model(rng, kind):
    """Oracle parameters of one of the branch classes of pwm_from_thrust, with an X layout of a random arm."""
    base = dict(mo.DEFAULT_MOTOR)
    jit = lambda m: dict(m, thrust_a=m["thrust_a"] * rng.uniform(0.8, 1.2) if m["thrust_a"] else 0.0, rpm_coefficient=m["rpm_coefficient"] * rng.uniform(0.9, 1.1),
                         rpm_offset=rng.uniform(-300, 600), torque_coefficient=m["torque_coefficient"] * rng.uniform(0.5, 2.0))
    lin, dead = dict(base, thrust_a=0.0, thrust_b=rng.uniform(3.0, 5.0)), dict(base, thrust_a=0.0, thrust_b=0.0, thrust_c=0.0)
    motors = {"default": [base] * 4, "linear": [lin] * 4, "dead_and_linear": [base, lin, dead, base],
              "disc_negative": [dict(base, thrust_c=0.5, thrust_b=0.2)] * 4, "high_motor_limit": [dict(base, pwm_max=1.3)] * 4,
              "mixed": [dict(base, pwm_max=1.2, pwm_idle=0.05), dict(base, thrust_c=0.4, thrust_b=0.3), lin, dict(base, pwm_min=0.03, pwm_idle=0.2)]}[kind]
    cfg = dict(config_pwm_min=0.0, config_pwm_max=1.0, config_pwm_idle=0.1) if kind != "mixed" else dict(config_pwm_min=0.04, config_pwm_max=0.95, config_pwm_idle=0.12)
    p = mo.params(np.eye(4), np.eye(4), [jit(m) for m in motors], max_thrust=rng.uniform(8, 20), body_rate_scale=rng.uniform(1, 3), watchdog_threshold=1.5, **cfg)
    p["mixing"] = mo.mixing_matrix(p, mo.x_positions(rng.uniform(0.1, 0.3)), [1, -1, 1, -1])
    p["inverse"] = np.linalg.solve(p["mixing"], np.eye(4))
    return p


def draw_commands(rng, p, state, B, dt):
    """B commands of the kernel's precision, each redrawn until it keeps MARGIN from every threshold: no row is excluded afterwards."""
    thrust, torque = np.empty(B), np.empty((B, 3))
    todo = np.arange(B)
    for _ in range(200):
        kind = rng.integers(0, 4, todo.size)
        t = np.where(kind == 0, rng.uniform(-2.0, 0.5, todo.size), np.where(kind == 1, rng.uniform(0.0, 3.0, todo.size), rng.uniform(2.0, 24.0, todo.size)))
        q = rng.uniform(-1, 1, (todo.size, 3)) * np.array([0.8, 0.8, 0.2]) * rng.choice([0.0, 0.1, 1.0], (todo.size, 1))
        thrust[todo], torque[todo] = t.astype(dt).astype(float), q.astype(dt).astype(float)
        m = mo.margin(p, None if state is None else state[todo], thrust[todo], torque[todo])
        todo = todo[m < MARGIN]
        if todo.size == 0:
            return thrust, torque
    raise AssertionError("no command with the margin")


def check_random_batch(h, B, model, health_mode, outputs, seed=0):
    """Three chained calls on B drones against the oracle.  health_mode: None, "shared", "per_drone"; outputs: "all" (flags, body rates, the
    record and every read-back), "pwm_only" (state, flags, body_rate NULL; wrench alone read back) or "no_state"."""
    rng = np.random.default_rng([seed, B, MODELS.index(model)])
    dv, ops = Dev(h), h.ops
    p = random_model(rng, model)
    pk = {k: (np.asarray(v).astype(h.dt).astype(float) if isinstance(v, np.ndarray) else float(h.dt(v))) for k, v in p.items()}     # the parameters as the kernel holds them
    mp = capi_params(p)
    with_state = outputs != "no_state" and outputs != "pwm_only"
    st, ost = (ops.mixer_state(B), mo.reset(B)) if with_state else (None, None)
    health = None if health_mode is None else rng.uniform(0.3, 1.0, (4,) if health_mode == "shared" else (B, 4)).astype(h.dt).astype(float)
    worst = dict(abs=0.0, rel=0.0)
    flag_hits = 0
    for call in range(3):
        thrust, torque = draw_commands(rng, pk, ost, B, h.dt)
        out = ops.mixer_mix(mp, dv.r(thrust), dv.r(torque), st, want_flags=outputs != "pwm_only", want_body_rate=outputs == "all")
        opwm, oflags = mo.mix(pk, ost, thrust, torque)
        pwm = host(h, out["pwm"]).astype(float)
        worst["abs"] = max(worst["abs"], close(pwm, opwm, h))
        if "flags" in out:
            got = host(h, out["flags"])
            assert np.array_equal(got, oflags), (call, np.nonzero(got != oflags)[0][:5], got[got != oflags][:5], oflags[got != oflags][:5])
            flag_hits += int(np.count_nonzero(oflags))
        if "body_rate" in out:
            worst["abs"] = max(worst["abs"], close(host(h, out["body_rate"]), mo.body_rate(pk, thrust, opwm), h))
        if with_state:
            rec = host(h, st).astype(float)
            assert np.array_equal(rec[:, 0], ost[:, 0])
            worst["abs"] = max(worst["abs"], close(rec[:, 1:5], ost[:, 1:5], h))
        want = READBACK if outputs == "all" else ("wrench",)
        rb = ops.mixer_readback(mp, out["pwm"], motor_health=None if health is None else dv.r(health), want=want)
        assert sorted(rb) == sorted(want)
        orb = mo.readback(pk, pwm, health)
        for nm in want:
            k = "rel" if nm in ("motor_torque", "motor_rpm") else "abs"
            worst[k] = max(worst[k], close(host(h, rb[nm]), orb[nm], h, rel=k == "rel"))
    print(f"mixer random batch B={B} {model} health={health_mode} outputs={outputs}: {worst}, {flag_hits} flagged rows")
    assert worst["abs"] <= tol(h) and worst["rel"] <= max(rel_tol(h), 1e-9), worst
    assert outputs == "pwm_only" or B < 60 or flag_hits > 0


# ---------------------------------------------------------------------------------------------- bit for bit
def _chain_step(h, ops, cp, sp, mp, smp, s, plan, sim_dt, health, wind):
    """One step by separate launches -> (target, command, pwm, wrench) as host arrays."""
    dv = Dev(h)
    if smp is not None:
        tg = ops.smoother_desired(smp, s["sm"], s["time"], s["pos"], s["vel"], *plan)["target"]
        tgh = host(h, tg)
        cmd = ops.control(cp, s["st"], s["time"], s["pos"], s["vel"], s["att"], s["om"], dv.r(tgh[:, 0:3]), dv.r(tgh[:, 3:6]), dv.r(tgh[:, 6:9]))
    else:
        cmd = ops.control_plan(cp, s["st"], s["time"], s["time"], s["pos"], s["vel"], s["att"], s["om"], *plan, want_target=True)
        tgh = host(h, cmd["target"])
    mix = ops.mixer_mix(mp, cmd["thrust"], cmd["torque"], s["mx"])
    w = host(h, ops.mixer_readback(mp, mix["pwm"], motor_health=health, want=("wrench",))["wrench"])
    ops.simulator_step(sp, s["time"], s["pos"], s["vel"], s["att"], s["om"], h.to_dev(np.ascontiguousarray(w[:, 0])), h.to_dev(np.ascontiguousarray(w[:, 1:4])),
                       sim_dt, wind=wind)
    return tgh, np.concatenate([host(h, cmd["thrust"])[:, None], host(h, cmd["torque"])], axis=1), host(h, mix["pwm"]), w


def check_bit_for_bit(h, B=65, N=6, n=20, smoothed=True):
    """closed_loop_actuated(nsteps = n) == n x (control_plan -- or smoother_desired + control --, mixer_mix, mixer_readback, simulator_step) ==
    two calls of n / 2: states, clocks, every record and the logs, bit for bit; motor_health NULL == all ones."""
    rng = np.random.default_rng(5)
    ts, P, V, A, P2, pos, vel, att, om, wind = _loop_inputs(rng, B, N)
    dv, ops = Dev(h), h.ops
    cp, sp, mp = ops.lib.controller_default_params(), ops.lib.simulator_default_params(), ops.lib.mixer_default_params()
    smp = SmootherParams.reference_defaults(transition_time=0.012) if smoothed else None
    sim_dt = 0.001
    plan1, plan2 = (dv.d(ts), dv.r(P), dv.r(V), dv.r(A)), (dv.d(ts), dv.r(P2), dv.r(V), dv.r(A))
    hv = rng.uniform(0.5, 1.0, (B, 4))
    hv[::3] = 1.0
    keys = ("st", "mx", "time", "pos", "vel", "att", "om") + (("sm",) if smoothed else ())
    wd = dv.r(wind)

    def start():
        s = dict(st=ops.controller_state(cp, B), mx=ops.mixer_state(B), time=dv.d(np.full(B, 7.0)), pos=dv.r(pos), vel=dv.r(vel), att=dv.r(att), om=dv.r(om), sm=None)
        if smoothed:
            s["sm"] = ops.smoother_state(B)
            ops.smoother_update(smp, s["sm"], s["time"], *plan1)
            ops.smoother_update(smp, s["sm"], dv.d(np.full(B, 7.0)), *plan2, old=plan1)
        return s

    def loop(s, steps, health):
        return ops.closed_loop_actuated(mp, cp, sp, s["st"], s["mx"], s["time"], s["pos"], s["vel"], s["att"], s["om"], *plan2, nsteps=steps, sim_dt=sim_dt,
                                        smoother=smp, smoother_state=s["sm"], motor_health=health, wind=wd, log=True)

    snap = lambda s: [host(h, s[k]) for k in keys]
    names = ("log_state", "log_cmd", "log_time", "log_target", "log_pwm", "log_wrench")
    for health in (dv.r(hv), None):
        one = start()
        log_one = loop(one, n, health)
        two = start()
        la, lb = loop(two, n // 2, health), loop(two, n - n // 2, health)
        for a, b in zip(snap(one), snap(two)):
            assert same(a, b), "two calls of n / 2 steps differ from one of n"
        for nm in names:
            assert same(host(h, log_one[nm]), np.concatenate([host(h, la[nm]), host(h, lb[nm])])), nm
        ch = start()
        for step in range(n):
            t_before, state_before = host(h, ch["time"]).copy(), np.concatenate([host(h, ch[k]) for k in ("pos", "vel", "att", "om")], axis=1)
            tg, cmd, pwm, w = _chain_step(h, ops, cp, sp, mp, smp, ch, plan2, sim_dt, health, wd)
            for nm, ref in (("log_target", tg), ("log_time", t_before), ("log_state", state_before), ("log_cmd", cmd), ("log_pwm", pwm), ("log_wrench", w)):
                assert same(host(h, log_one[nm])[step], ref), (nm, step)
        for a, b in zip(snap(one), snap(ch)):
            assert same(a, b), "the chained launches differ from the one launch"
        if health is None:
            ones = start()
            log_ones = loop(ones, n, dv.r(np.ones((B, 4))))
            for a, b in zip(snap(one), snap(ones)):
                assert same(a, b), "motor_health NULL differs from all ones"
            assert same(host(h, log_one["log_wrench"]), host(h, log_ones["log_wrench"]))
    cmds, wr = host(h, log_one["log_cmd"]).astype(float), host(h, log_one["log_wrench"]).astype(float)
    assert np.max(np.abs(cmds - wr)) > 1e-3          # the scene saturates: the realised wrench is not the command


def check_transparent_mixer_equals_plain_loop(h, B=65, n=60):
    """With a mixer whose realised wrench equals the command at every step, the state trajectory is se3mpc_closed_loop_*'s to 1e-12 (float64).

    The loop: a hover within 1 cm of a standing target with the default controller and STRONGER motors than the reference's default ones (thrust =
    30 pwm^2, no offset, no idle floor, limits [0, 1]): commands stay between 8 and 13 N and every PWM between 0.05 and 0.5 (asserted below), inside
    all limits, where pwm_from_thrust and thrust_from_pwm are inverses and B @ inverse = I up to rounding."""
    rng = np.random.default_rng(9)
    dv, ops = Dev(h), h.ops
    cp, sp = ops.lib.controller_default_params(), ops.lib.simulator_default_params()
    motor = dict(mo.DEFAULT_MOTOR, thrust_a=30.0, thrust_b=0.0, thrust_c=0.0, pwm_idle=0.0)
    p = mo.params(np.eye(4), np.eye(4), [motor] * 4, config_pwm_idle=0.0)
    p["mixing"] = mo.mixing_matrix(p, mo.x_positions(0.15), [1, -1, 1, -1])
    p["inverse"] = np.linalg.solve(p["mixing"], np.eye(4))
    mp = capi_params(p)
    pos = rng.uniform(-1, 1, (B, 3)) + [0, 0, 2]
    hold = pos + rng.uniform(-0.01, 0.01, (B, 3))
    plan = (dv.d([0.0, 100.0]), dv.r(np.stack([hold, hold], axis=1)), None, None)
    runs = []
    for actuated in (False, True):
        st, time = ops.controller_state(cp, B), dv.d(np.zeros(B))
        s = [dv.r(pos), dv.r(np.zeros((B, 3))), dv.r(np.zeros((B, 3))), dv.r(np.zeros((B, 3)))]
        if actuated:
            mx = ops.mixer_state(B)
            log = ops.closed_loop_actuated(mp, cp, sp, st, mx, time, *s, *plan, nsteps=n, sim_dt=0.001, log=True)
            assert np.all(host(h, mx)[:, 0] == 0)
        else:
            log = ops.closed_loop(cp, sp, st, time, *s, *plan, nsteps=n, sim_dt=0.001, stop_at_plan_end=False, log=True)
        runs.append((host(h, log["log_state"]).astype(float), host(h, log["log_cmd"]).astype(float), log))
    cmd = runs[1][1]
    wr, pwm = host(h, runs[1][2]["log_wrench"]).astype(float), host(h, runs[1][2]["log_pwm"]).astype(float)
    assert 8.0 < cmd[..., 0].min() and cmd[..., 0].max() < 13.0 and 0.05 < pwm.min() and pwm.max() < 0.5, (cmd[..., 0].min(), cmd[..., 0].max(), pwm.min(), pwm.max())
    e = dict(wrench=float(np.max(np.abs(wr - cmd))), state=float(np.max(np.abs(runs[0][0] - runs[1][0]))))
    print("transparent mixer against the plain loop:", e)
    bound = 1e-12 if h.dt == np.float64 else 1e-4
    assert e["wrench"] <= bound * 10 and e["state"] <= bound, e


# ---------------------------------------------------------------------------------------------- behaviour
def check_behaviour(h):
    """The climb under the default motors; the infeasible roll-and-pitch command; a motor at half health."""
    data, meta = golden()
    dv, ops = Dev(h), h.ops
    climb = [l for l in meta["loops"] if l["tag"] == "climb"][0]
    got = run_golden_loop(h, climb)
    assert np.max(got["cmd"][:, 0]) == climb["controller_max_thrust"] > 15.2           # the controller asks for more than the motors have
    assert np.max(got["wrench"][:, 0]) <= 15.2 + (1e-9 if h.dt == np.float64 else 1e-5)
    assert got["final"][2] < climb["unactuated_final_altitude"] - 0.05                   # ... and the vehicle climbs less than under the commanded wrench
    assert got["mixer"][0] == 0                                                          # the allclose quirk: the model's own clip hides the saturation
    # the un-actuated loop on the same scene, through se3mpc_closed_loop_*
    cp, sp = ops.lib.controller_default_params(), ops.lib.simulator_default_params()
    key = climb["key"]
    t0 = float(data[key + "t"][0])
    st, time = ops.controller_state(cp, 1), dv.d([t0])
    s = [dv.r(data[key + n_][0][None]) for n_ in ("pos", "vel", "att", "omega")]
    ops.closed_loop(cp, sp, st, time, *s, dv.d([t0, t0 + 1000.0]), dv.r(np.array([climb["hold"], climb["hold"]])), nsteps=climb["nsteps"], sim_dt=climb["sim_dt"],
                    stop_at_plan_end=False)
    free = float(host(h, s[0])[0, 2])
    assert abs(free - climb["unactuated_final_altitude"]) <= (1e-9 if h.dt == np.float64 else 5e-3) and got["final"][2] < free
    # (9.81, [1, 1, 0]): an X frame cannot give 1 N m of roll and of pitch at hover
    mp = ops.lib.mixer_default_params()
    out = ops.mixer_mix(mp, dv.r([9.81]), dv.r([[1.0, 1.0, 0.0]]))
    pwm = host(h, out["pwm"]).astype(float)[0]
    w = host(h, ops.mixer_readback(mp, out["pwm"], want=("wrench",))["wrench"]).astype(float)[0]
    bound = 1e-6 if h.dt == np.float64 else 1e-4
    assert np.max(np.abs(pwm - [0.759299753, 1.0, 0.759299753, 0.1])) <= bound, pwm
    ref = mo.default_params()
    rpwm, _ = mo.mix(ref, None, np.array([9.81]), np.array([[1.0, 1.0, 0.0]]))
    assert np.max(np.abs(w - mo.readback(ref, rpwm)["wrench"][0])) <= bound, w                   # the oracle's figure (pinned to the reference to 1e-14)
    assert np.max(np.abs(w - [8.95, 0.377, 0.377, 1.635])) <= 1e-3, w                            # ... which is the one the reference gives, to the digits quoted
    # hover with motor 0 at half health realises the oracle's wrench
    half = [l for l in meta["loops"] if l["tag"] == "hover_motor0_half"][0]
    g = run_golden_loop(h, half)
    want = mo.readback(mo.default_params(), g["pwm"], np.array(half["health"]))["wrench"]
    assert np.max(np.abs(g["wrench"] - want)) <= tol(h)
    assert np.all(g["wrench"][:, 1] > 0) and np.all(g["wrench"][:, 2] < 0)              # the weak front-right motor rolls and pitches the vehicle


# ---------------------------------------------------------------------------------------------- ClosedLoopMonteCarlo
def check_monte_carlo_option(h, B=5, N=8, cycles=3, substeps=10):
    """run / run_mppi with mixer= equal the hand-chained launches bit for bit (with and without the smoother); mixer=None is today's path; the
    fused forms and capture refuse the option; motor_health needs a mixer."""
    import pytest
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    rng = np.random.default_rng(11)
    dv, ops = Dev(h), h.ops
    prm = Params.reference_defaults(horizon=N)
    mc = ClosedLoopMonteCarlo(ops, prm)
    p0, v0, goal = dv.r(rng.uniform(-1, 1, (B, 3)) + [0, 0, 2]), dv.r(rng.normal(0, 0.2, (B, 3))), dv.r(rng.uniform(-3, 3, (B, 3)) + [0, 0, 2])
    sim_dt = 0.0025
    mp, smp = ops.lib.mixer_default_params(), SmootherParams.reference_defaults()
    health = dv.r(rng.uniform(0.6, 1.0, (B, 4)))
    eq = lambda a, b: np.array_equal(host(h, a).view(np.uint8), host(h, b).view(np.uint8))
    a, b = mc.run(p0, v0, goal, cycles, substeps, sim_dt), mc.run(p0, v0, goal, cycles, substeps, sim_dt, mixer=None)
    assert all(eq(a[k], b[k]) for k in ("pos", "vel", "att", "omega", "time", "controller_state")) and "mixer_state" not in b
    for sm_p in (None, smp):
        for hl in (None, health):
            s = mc.run(p0, v0, goal, cycles, substeps, sim_dt, smoother=sm_p, mixer=mp, motor_health=hl)
            pos, vel, att, om = p0.clone(), v0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
            time = dv.d(np.zeros(B))
            st, mx, sm, old = ops.controller_state(mc.controller, B), ops.mixer_state(B), (ops.smoother_state(B) if sm_p is not None else None), None
            for c in range(cycles):
                sol = ops.solve(prm, pos, vel, goal)
                new = (dv.d((c * substeps * sim_dt) + np.arange(N) * prm.dt), sol["x"][:, :3 * N].reshape(B, N, 3).contiguous(),
                       sol["x"][:, 3 * N:6 * N].reshape(B, N, 3).contiguous(), sol["accelerations"].reshape(B, N, 3).contiguous())
                if sm_p is not None:
                    ops.smoother_update(sm_p, sm, time, *new, old=old)
                ops.closed_loop_actuated(mp, mc.controller, mc.simulator, st, mx, time, pos, vel, att, om, *new, nsteps=substeps, sim_dt=sim_dt, smoother=sm_p,
                                         smoother_state=sm, motor_health=hl)
                old = new
            for got, want in ((s["pos"], pos), (s["vel"], vel), (s["att"], att), (s["omega"], om), (s["time"], time), (s["controller_state"], st), (s["mixer_state"], mx)):
                assert eq(got, want)
            assert ("smoother_state" in s) == (sm_p is not None) and (sm_p is None or eq(s["smoother_state"], sm))
            assert tuple(s["mixer_state"].shape) == (B, MIXER_STATE_WORDS)
    assert not eq(a["pos"], s["pos"])
    for fn, args in ((mc.run_fused, (p0, v0, goal, cycles, substeps, sim_dt)), (mc.run_mppi_fused, (p0, v0, goal, cycles, substeps, sim_dt, 64, 1, 1.0, 1.0)),
                     (mc.capture, (B, torch.float64, cycles, substeps, sim_dt))):
        with pytest.raises(ValueError, match="mixer"):
            fn(*args, mixer=mp)
        with pytest.raises(ValueError, match="mixer"):
            fn(*args, motor_health=health)
    with pytest.raises(ValueError, match="mixer"):
        mc.run(p0, v0, goal, cycles, substeps, sim_dt, motor_health=health)
    with pytest.raises(ValueError, match="mixer"):
        mc.run_mppi(p0, v0, goal, 2, substeps, sim_dt, 64, 2, 1.0, 1.0, motor_health=health)
    # MPPI as the planner
    m0 = mc.run_mppi(p0, v0, goal, 2, substeps, sim_dt, 64, 2, 1.0, 1.0, seed=3)
    m1 = mc.run_mppi(p0, v0, goal, 2, substeps, sim_dt, 64, 2, 1.0, 1.0, seed=3, mixer=None)
    assert eq(m0["pos"], m1["pos"]) and "mixer_state" not in m1
    for sm_p in (None, smp):
        m2 = mc.run_mppi(p0, v0, goal, 2, substeps, sim_dt, 64, 2, 1.0, 1.0, seed=3, smoother=sm_p, mixer=mp, motor_health=health)
        assert np.all(np.isfinite(host(h, m2["pos"]))) and np.allclose(host(h, m2["time"]), 2 * substeps * sim_dt) and m2["clearance"] is None
        st, sm, (time, pos, vel, att, om) = mc._start(p0, v0, sm_p)
        mx = ops.mixer_state(B)
        U = mc._mppi_start(p0, None)
        sh = mc.resolve_shift(substeps, sim_dt, None)
        old = None
        for c in range(2):
            out = ops.mppi_closed_loop(prm, mc.controller, mc.simulator, st, time, pos, vel, att, om, goal, U, 1, 0, sim_dt, 64, 2, 1.0, 1.0, seed=3, cycle_base=c,
                                       shift=sh, want_plan=True, want_clearance=False)
            pl = out["plan_last"]
            new = (dv.d((c * substeps * sim_dt) + np.arange(N) * prm.dt), pl[:, 0].contiguous(), pl[:, 1].contiguous(), pl[:, 2].contiguous())
            if sm_p is not None:
                ops.smoother_update(sm_p, sm, time, *new, old=old)
            ops.closed_loop_actuated(mp, mc.controller, mc.simulator, st, mx, time, pos, vel, att, om, *new, nsteps=substeps, sim_dt=sim_dt, smoother=sm_p,
                                     smoother_state=sm, motor_health=health)
            old = new
        for got, want in ((m2["pos"], pos), (m2["vel"], vel), (m2["att"], att), (m2["omega"], om), (m2["time"], time), (m2["controller_state"], st),
                          (m2["mixer_state"], mx), (m2["U"], U)):
            assert eq(got, want)


# ---------------------------------------------------------------------------------------------- the mirror classes
def check_mirror(h, monkeypatch):
    """The golden sequences through dart_planner_amd.hardware.motor_mixer.MotorMixer and the model's scalar methods, call by call, with the
    reference's exceptions and the quirk values of get_control_allocation; the factories' matrices; the import shims."""
    import importlib
    import sys
    import pytest
    import dart_planner_amd.hardware.motor_mixer as mm
    import dart_planner_amd.hardware.motor_model as mdl
    data, meta = golden()
    prec = "f64" if h.dt == np.float64 else "f32"
    monkeypatch.setattr(mm.MotorMixer, "_get_ops", lambda self: h.ops)
    monkeypatch.setattr(mdl.QuadraticMotorModel, "_get_ops", lambda self: h.ops)
    # the factories: B through the kernels' two model values, the inverse by the reference's own NumPy call
    mtol = 1e-12 if h.dt == np.float64 else 1e-6
    for m in meta["matrices"]:
        mk = mm.create_plus_configuration_mixer if m["tag"].startswith("plus") else mm.create_x_configuration_mixer
        mixer = mk(float(m["tag"].split("_")[1]), precision=prec)
        assert np.max(np.abs(mixer.mixing_matrix - data[f"mat_{m['tag']}_B"])) <= mtol * 2
        if m["rank"] == 4:
            assert np.max(np.abs(mixer.inverse_matrix - data[f"mat_{m['tag']}_inverse"])) <= mtol * 20
            assert mixer.validate_configuration() == []
        else:
            assert mixer.inverse_matrix.shape == (4, 4) and any("rank-deficient" in s for s in mixer.validate_configuration())
            if h.dt == np.float64:                # the same NumPy calls on the same matrix (solve raises, pinv answers): the same matrix
                assert np.array_equal(mixer.mixing_matrix, data[f"mat_{m['tag']}_B"]) and np.array_equal(mixer.inverse_matrix, data[f"mat_{m['tag']}_inverse"])
        assert mixer.get_motor_layout_info()["matrix_rank"] == m["rank"] and mixer.saturation_events == 0 and np.array_equal(mixer.last_motor_commands, np.zeros(4))
    # the sequences, with the golden matrices assigned (as code written against the reference may)
    for seq in meta["sequences"]:
        key = seq["key"]
        motors = {i: mdl.MotorParameters(motor_id=i, direction=(1, -1, 1, -1)[i], **dict(zip(mo.MOTOR_FIELDS, (float(x) for x in data[key + "motors"][:, i]))))
                  for i in range(4)}
        model = mdl.QuadraticMotorModel(motors, precision=prec)
        cfg = mm.MotorMixingConfig(layout=mm.QuadrotorLayout.CUSTOM, motor_model=model, pwm_min=seq["config_pwm_min"], pwm_max=seq["config_pwm_max"],
                                   pwm_idle=seq["config_pwm_idle"])
        mixer = mm.MotorMixer(cfg, precision=prec)
        mixer.mixing_matrix, mixer.inverse_matrix = np.array(data[key + "B"]), np.array(data[key + "inverse"])
        for e in range(seq["calls"]):
            thrust, torque = float(data[key + "thrust"][e]), np.array(data[key + "torque"][e])
            if int(data[key + "flags"][e]) & mo.NON_FINITE:
                with pytest.raises(RuntimeError, match="Non-finite"):
                    mixer.mix_commands(thrust, torque)
            else:
                assert np.max(np.abs(mixer.mix_commands(thrust, torque) - data[key + "pwm"][e])) <= tol(h), (seq["tag"], e)
            ref = data[key + "state"][e]
            assert mixer.saturation_events == ref[0] and np.max(np.abs(mixer.last_motor_commands - ref[1:5])) <= tol(h)
            if e % 8 == 0:
                q = mixer.last_motor_commands
                assert np.max(np.abs(mixer.get_control_allocation(q) - data[key + "allocation"][e])) <= tol(h)
                assert np.max(np.abs(mixer._pwm_to_thrust(q) - data[key + "motor_thrust"][e])) <= tol(h)
                for i in range(4):
                    assert abs(model.thrust_from_pwm(float(q[i]), i) - data[key + "motor_thrust"][e][i]) <= tol(h)
                    assert abs(model.torque_from_pwm(float(q[i]), i) - data[key + "motor_torque"][e][i]) <= max(rel_tol(h), 1e-9) * 100
                    assert abs(model.rpm_from_pwm(float(q[i]), i) - data[key + "motor_rpm"][e][i]) <= max(rel_tol(h), 1e-9) * 1e4
                    f = float(data[key + "motor_thrust"][e][i])
                    if motors[i].pwm_min < q[i] < motors[i].pwm_max and abs(motors[i].thrust_a) > 1e-9 and f > 1e-3:
                        assert abs(model.pwm_from_thrust(f, i) - q[i]) <= (1e-9 if h.dt == np.float64 else 1e-4)      # inverse of the forward model inside the limits
        mixer.reset_saturation_counter()
        assert mixer.saturation_events == 0 and np.max(np.abs(mixer.last_motor_commands - ref[1:5])) <= tol(h)
    # exceptions and the quirks by name
    mixer = mm.create_x_configuration_mixer(0.15, precision=prec)
    with pytest.raises(ValueError, match="3-element"):
        mixer.mix_commands(9.81, np.zeros(4))
    hover = mixer.mix_commands(9.81, np.zeros(3))
    assert np.max(np.abs(mixer.get_control_allocation(hover) - [0.93559905, 11.85359296, 0.93559905, -11.27229106])) <= 1e-4 * (1 if h.dt == np.float32 else 1e-3)
    assert np.max(np.abs(mixer.get_realised_wrench(hover) - [9.81, 0, 0, 0])) <= 1e-4
    mixer.mix_commands(20.0, np.zeros(3))
    assert mixer.saturation_events == 0                      # the model clipped to the motor's limit first: np.allclose sees no change
    mixer.mix_commands(0.3, np.zeros(3))
    assert mixer.saturation_events == 1                      # the idle floor moved a PWM
    assert np.array_equal(mixer._saturate_pwm(np.array([1.2, -0.3, 0.05, 0.5])), np.array([1.0, 0.1, 0.1, 0.5]).astype(h.dt).astype(float))
    assert np.max(np.abs(mixer._thrust_to_pwm(np.array([3.8, -1.0, 0.0, 50.0])) - [1.0, 0.1, 0.1, 1.0])) <= tol(h)
    model = mixer.motor_model
    assert model.thrust_from_pwm(float("nan"), 0) == 0.0 and model.thrust_from_pwm(7.0, 0) == model.thrust_from_pwm(1.0, 0)      # max(0.0, nan); the clip
    assert model.pwm_from_thrust(-1.0, 2) == np.float64(h.dt(0.1)) and model.validate_pwm(1.5, 0) is False and model.validate_pwm(0.5, 9) is False
    low = mdl.QuadraticMotorModel({0: mdl.MotorParameters(motor_id=0, thrust_a=2.5, thrust_b=0.2, thrust_c=0.5, rpm_coefficient=8000)}, precision=prec)
    assert low.pwm_from_thrust(0.3, 0) == 1.0                # below the curve's minimum: disc < 0 asks for full PWM
    for bad in (lambda: model.thrust_from_pwm(0.5, 7), lambda: model.pwm_from_thrust(1.0, 7), lambda: model.get_motor_parameters(7),
                lambda: mdl.MotorParameters(motor_id=0, thrust_a=-1.0, rpm_coefficient=1.0), lambda: mdl.MotorParameters(motor_id=0, rpm_coefficient=0.0),
                lambda: mdl.MotorParameters(motor_id=0, rpm_coefficient=1.0, pwm_min=1.0), lambda: mdl.MotorParameters(motor_id=0, rpm_coefficient=1.0, direction=0),
                lambda: mdl.QuadraticMotorModel({1: mdl.MotorParameters(motor_id=0, rpm_coefficient=1.0)}),
                lambda: mdl.fit_quadratic_motor_model(mdl.BenchTestData(motor_id=0, pwm_values=[0.1, 0.2], thrust_measurements=[1, 2], rpm_measurements=[1, 2]))):
        with pytest.raises(ValueError):
            bad()

    class Foreign(mdl.MotorModel):
        """A MotorModel written outside the package, as the reference's own unit tests have one: thrust = 8 pwm, torque = 0.2 pwm."""
        thrust_from_pwm = lambda self, pwm, motor_id: 8.0 * pwm
        torque_from_pwm = lambda self, pwm, motor_id: 0.2 * pwm
        pwm_from_thrust = lambda self, thrust, motor_id: min(max(thrust / 8.0, 0.0), 1.0)
        rpm_from_pwm = lambda self, pwm, motor_id: 1000.0 * pwm
        get_motor_parameters = lambda self, motor_id: None
        validate_pwm = lambda self, pwm, motor_id: True
    with pytest.raises(TypeError, match="MotorModel"):
        mm.MotorMixer(mm.MotorMixingConfig(motor_model=object()))
    fm = mm.MotorMixer(mm.MotorMixingConfig(motor_model=Foreign()), precision=prec)      # the mixer's own arithmetic stays on the device, the model's on the host
    Bf = np.stack([np.ones(4), [-0.15, 0.15, 0.15, -0.15], [0.15, 0.15, -0.15, -0.15], np.array([1, -1, 1, -1]) * 0.025])
    assert np.max(np.abs(fm.mixing_matrix - Bf)) <= 1e-15 and np.max(np.abs(fm.inverse_matrix - np.linalg.solve(Bf, np.eye(4)))) <= 1e-12
    events = 0
    for thrust, torque in ((12.0, [0.1, -0.05, 0.01]), (40.0, [0.0, 0.0, 0.0]), (1.0, [0.3, 0.0, 0.0]), (-2.0, [0.0, 0.0, 0.0]), (20.0, [0.5, 0.5, 0.02])):
        raw = np.clip(np.maximum(fm.inverse_matrix @ np.array([max(thrust, 0.0), *torque]), 0.0) / 8.0, 0.0, 1.0)
        want = np.maximum(raw, 0.1)
        events += int(not np.allclose(raw, want, rtol=1e-6))
        got = fm.mix_commands(thrust, np.array(torque))
        assert np.max(np.abs(got - want)) <= tol(h) and fm.saturation_events == events and np.array_equal(fm.last_motor_commands, got), (thrust, got, want)
        assert np.max(np.abs(fm.get_control_allocation(got) - fm.inverse_matrix @ (8.0 * got))) <= tol(h) * 100
        assert np.max(np.abs(fm.get_realised_wrench(got) - Bf @ (8.0 * got))) <= tol(h) * 10 and np.array_equal(fm._pwm_to_thrust(got), 8.0 * got)
    assert events >= 2 and np.max(np.abs(fm._thrust_to_pwm(np.array([4.0, -1.0, 16.0, 0.0])) - [0.5, 0.0, 1.0, 0.0])) <= tol(h)
    with pytest.raises(RuntimeError, match="Non-finite"):
        fm.mix_commands(float("nan"), np.zeros(3))
    assert fm.saturation_events == events
    pw = np.linspace(0.1, 1.0, 10)
    fit = mdl.fit_quadratic_motor_model(mdl.BenchTestData(motor_id=2, pwm_values=list(pw), thrust_measurements=list(2.5 * pw**2 + 1.2 * pw + 0.1),
                                                          rpm_measurements=list(8000 * pw + 500)))
    assert abs(fit.thrust_a - 2.5) < 1e-9 and abs(fit.rpm_coefficient - 8000) < 1e-6 and fit.pwm_idle == pw[0] + 0.1 * (pw[-1] - pw[0]) and fit.motor_id == 2
    assert mm.MotorMixingConfig().mixing_matrix.tolist()[0] == [1.0, -0.15, 0.15, 1.0]
    # import shims
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dart_planner_amd", "compat")
    monkeypatch.syspath_prepend(compat)
    for m in [m for m in sys.modules if m == "dart_planner" or m.startswith("dart_planner.")]:
        monkeypatch.delitem(sys.modules, m)
    assert importlib.import_module("dart_planner.hardware.motor_mixer").MotorMixer is mm.MotorMixer
    assert importlib.import_module("dart_planner.hardware.motor_model").QuadraticMotorModel is mdl.QuadraticMotorModel


# ---------------------------------------------------------------------------------------------- arguments, B = 0, dirty buffers, NaN drone
def check_invalid_arguments(h):
    dv, ops, lib = Dev(h), h.ops, h.ops.lib
    suf = "f64" if h.dt == np.float64 else "f32"
    B, N = 3, 4
    mp, cp, sp, smp = lib.mixer_default_params(), lib.controller_default_params(), lib.simulator_default_params(), SmootherParams.reference_defaults()
    ptr = ops.be.ptr
    now, pos, vel, att, om = dv.d(np.full(B, 1.0)), dv.r(np.zeros((B, 3))), dv.r(np.zeros((B, 3))), dv.r(np.zeros((B, 3))), dv.r(np.zeros((B, 3)))
    ts, P = dv.d(np.arange(N) * 0.1), dv.r(np.ones((N, 3)))
    sm, st, mx = ops.smoother_state(B), ops.controller_state(cp, B), ops.mixer_state(B)
    th, tq, pwm, fl = dv.r(np.full(B, 9.0)), dv.r(np.zeros((B, 3))), dv.r(np.full((B, 4), 7.0)), h.to_dev(np.full(B, 7, dtype=np.int32))
    out4 = dv.r(np.full((B, 4), 7.0))
    before = [np.array(h.to_host(a)).copy() for a in (sm, st, mx, pos, pwm, out4)]
    plan = lambda n=N, t=ts, p=P, s=(0, 0, 0, 0): [n, ptr(t), s[0], ptr(p), s[1], 0, s[2], 0, s[3]]

    def mix(mp_=mp, B_=B, th_=th, tq_=tq, st_=mx, pwm_=pwm):
        return lib.loop_status("mixer_mix", suf, mp_, B_, ptr(th_), ptr(tq_), ptr(st_), ptr(pwm_), ptr(fl), 0, 0)

    def readback(mp_=mp, B_=B, pwm_=pwm, stride=0):
        return lib.loop_status("mixer_readback", suf, mp_, B_, ptr(pwm_), 0, stride, ptr(out4), 0, 0, 0, 0, 0)

    def loop(smp_=smp, cp_=cp, sp_=sp, mp_=mp, B_=B, nsteps=2, sim_dt=0.01, pl=None, time_=now, pos_=pos, st_=st, sm_=sm, mx_=mx, health_stride=0, wind_stride=0,
             gust_step=-1):
        return lib.loop_status("closed_loop_actuated", suf, smp_, cp_, sp_, mp_, B_, nsteps, sim_dt, *(plan() if pl is None else pl), ptr(time_), ptr(pos_), ptr(vel),
                               ptr(att), ptr(om), ptr(st_), ptr(sm_), ptr(mx_), 0, health_stride, 0, wind_stride, gust_step, None, 0, 0, 0, 0, 0, 0, 0)

    NULL, SHAPE, PARAM = -1, -3, -4
    bad_params = [mp.copy(thrust_a=[float("nan")] * 4), mp.copy(pwm_max=[1.0, float("inf"), 1.0, 1.0]), mp.copy(config_pwm_idle=float("nan")),
                  mp.copy(max_thrust=float("inf")), mp.copy(body_rate_scale=float("nan")), mp.copy(watchdog_threshold=float("nan"))]
    for bp in bad_params:
        assert mix(mp_=bp) == PARAM and readback(mp_=bp) == PARAM and loop(mp_=bp) == PARAM
        assert "mixer parameters" in lib.last_error()
    assert mix(mp_=None) == NULL and readback(mp_=None) == NULL and loop(mp_=None) == NULL and loop(cp_=None) == NULL and loop(sp_=None) == NULL
    assert mix(B_=-1) == SHAPE and readback(B_=-1) == SHAPE and loop(B_=-1) == SHAPE
    assert mix(th_=None) == NULL and mix(tq_=None) == NULL and mix(pwm_=None) == NULL and readback(pwm_=None) == NULL and readback(stride=-1) == SHAPE
    assert loop(smp_=None) == NULL and loop(sm_=None) == NULL and "come together" in lib.last_error()       # one of the smoother pair alone
    assert loop(smp_=smp.copy(update_dt=0.0)) == PARAM
    assert loop(nsteps=-1) == SHAPE and loop(wind_stride=-1) == SHAPE and loop(health_stride=-1) == SHAPE and loop(pl=plan(n=-2)) == SHAPE and loop(pl=plan(n=4097)) == SHAPE
    assert loop(smp_=None, sm_=None, pl=plan(n=0)) == SHAPE                      # the raw sampler needs a row (the smoother samples zeros: below)
    assert loop(sim_dt=float("nan")) == PARAM and loop(sim_dt=float("inf")) == PARAM
    assert loop(time_=None) == NULL and loop(pos_=None) == NULL and loop(st_=None) == NULL and loop(mx_=None) == NULL and loop(pl=plan(t=None)) == NULL
    assert loop(gust_step=0) == NULL
    assert lib._dll.se3mpc_mixer_reset(-1, ptr(mx), 0) == SHAPE and lib._dll.se3mpc_mixer_reset(B, None, 0) == NULL and lib._dll.se3mpc_mixer_default_params(None) == NULL
    # no-ops: B = 0 and nsteps = 0 (with every pointer NULL)
    none = [0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert lib.loop_status("mixer_mix", suf, mp, 0, 0, 0, 0, 0, 0, 0, 0) == 0 and lib.loop_status("mixer_readback", suf, mp, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0
    assert lib.loop_status("closed_loop_actuated", suf, smp, cp, sp, mp, 0, 5, 0.01, *none, 0, 0, 0, 0, 0, 0, ptr(sm), 0, 0, 0, 0, 0, -1, None, 0, 0, 0, 0, 0, 0, 0) == 0
    assert loop(nsteps=0) == 0 and lib._dll.se3mpc_mixer_reset(0, None, 0) == 0
    # every rejected call launched nothing (the records are fresh: the one accepted call above was a NaN batch, which leaves them alone)
    for now_, then in zip((sm, st, mx, pos, pwm, out4), before):
        assert np.array_equal(np.array(h.to_host(now_)).view(np.uint8), then.view(np.uint8))
    assert np.all(host(h, fl) == 7)
    # accepted: an empty plan behind the smoother, and matrices of a singular layout (reported per drone, the records left alone)
    assert loop(pl=plan(n=0)) == 0
    singular, flown = mp.copy(inverse=np.full((4, 4), np.nan)), host(h, mx).copy()
    assert mix(mp_=singular) == 0 and np.all(host(h, fl) == mo.NON_FINITE) and np.all(np.isnan(host(h, pwm))) and same(host(h, mx), flown)
    import pytest
    with pytest.raises(ValueError):
        ops.mixer_mix(mp, th, dv.r(np.zeros((B, 4))))
    with pytest.raises(ValueError):
        ops.mixer_mix(mp, th, tq, dv.d(np.zeros((B, 4))))
    with pytest.raises(ValueError):
        ops.mixer_readback(mp, pwm, motor_health=dv.r(np.ones((B + 1, 4))))
    with pytest.raises(ValueError):
        ops.mixer_readback(mp, pwm, want=("thrust",))
    with pytest.raises(ValueError):
        ops.closed_loop_actuated(mp, cp, sp, st, mx, now, pos, vel, att, om, ts, P, smoother=smp)
    with pytest.raises(AttributeError):
        MixerParams.reference_defaults(no_such_field=1.0)


def check_dirty_buffers_and_nan_drone(h, B=66, N=6):
    """Outputs are fully written whatever they held; a drone whose command, state and plan are NaN leaves its neighbours' bits alone, and in
    the single call its own record too.

    Every buffer an entry point writes without reading (the record se3mpc_mixer_reset fills, pwm, flags, body_rate, the five read-backs and
    the six logs) is the caller's here, handed to the C ABI filled with one byte pattern: 0xFF (a NaN in both float formats, -1 as int32) in
    one run, 0x7B in the next.  An element the kernels leave unwritten keeps its pattern and so differs between the two runs."""
    rng = np.random.default_rng(21)
    ts, P, V, A, P2, pos, vel, att, om, wind = _loop_inputs(rng, B, N)
    dv, ops, lib = Dev(h), h.ops, h.ops.lib
    ptr, suf, nsteps = ops.be.ptr, "f64" if h.dt == np.float64 else "f32", 8
    cp, sp, mp = lib.controller_default_params(), lib.simulator_default_params(), lib.mixer_default_params()
    thrust, torque = rng.uniform(0.0, 20.0, B), rng.uniform(-0.5, 0.5, (B, 3))
    health = rng.uniform(0.5, 1.0, (B, 4))

    def run(poison, byte):
        def dirty(shape, dtype):
            a = np.empty(shape, dtype=dtype)
            a.view(np.uint8)[...] = byte
            return h.to_dev(a)

        p_, v_, P_, th_ = pos.copy(), vel.copy(), P2.copy(), thrust.copy()
        if poison is not None:
            p_[poison] = v_[poison] = np.nan; P_[poison] = np.nan; th_[poison] = np.nan
        mx = dirty((B, MIXER_STATE_WORDS), np.float64)
        lib.mixer_reset(B, ptr(mx), ops.be.stream())
        pwm, fl, br = dirty((B, 4), h.dt), dirty((B,), np.int32), dirty((B, 4), h.dt)
        dth, dtq, dh, dw = dv.r(th_), dv.r(torque), dv.r(health), dv.r(wind)         # (named: a temporary's memory would be handed to the next one)
        lib.loop_call("mixer_mix", suf, mp, B, ptr(dth), ptr(dtq), ptr(mx), ptr(pwm), ptr(fl), ptr(br), ops.be.stream())
        mx_single = np.array(h.to_host(mx))
        rb = [dirty((B, 4), h.dt) for _ in range(5)]
        lib.loop_call("mixer_readback", suf, mp, B, ptr(pwm), ptr(dh), 4, *[ptr(a) for a in rb], ops.be.stream())
        st, time = ops.controller_state(cp, B), dv.d(np.full(B, 7.0))
        dp, dvl, da, do = dv.r(p_), dv.r(v_), dv.r(att), dv.r(om)
        pl = (dv.d(ts), dv.r(P_), dv.r(V), dv.r(A))
        plan = ops._plan_ptrs(B, suf, *pl, None)
        logs = [dirty((nsteps, B, 12), h.dt), dirty((nsteps, B, 4), h.dt), dirty((nsteps, B), np.float64), dirty((nsteps, B, 9), h.dt), dirty((nsteps, B, 4), h.dt),
                dirty((nsteps, B, 4), h.dt)]
        lib.loop_call("closed_loop_actuated", suf, None, cp, sp, mp, B, nsteps, 0.002, *plan, ptr(time), ptr(dp), ptr(dvl), ptr(da), ptr(do), ptr(st), 0, ptr(mx),
                      ptr(dh), 4, ptr(dw), 3, -1, None, *[ptr(a) for a in logs], ops.be.stream())
        return [np.array(h.to_host(o)) for o in [pwm, fl, br] + rb + logs + [mx, st, dp, time]] + [mx_single]

    clean, again, sick = run(None, 0xFF), run(None, 0x7B), run(17, 0xFF)
    for i, (a, b) in enumerate(zip(clean, again)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), i     # nothing kept the bytes it was handed
    for a in clean[:14]:
        assert a.dtype == np.int32 or np.all(np.isfinite(a))                 # (0xFF.. is a NaN)
    assert np.all((clean[1] >= 0) & (clean[1] < 64))
    others = np.arange(B) != 17
    for a, c in zip(clean, sick):
        ax = 0 if a.shape[0] == B else 1
        assert np.array_equal(np.compress(others, a, axis=ax).view(np.uint8), np.compress(others, c, axis=ax).view(np.uint8))
    assert np.all(np.isnan(sick[0][17])) and sick[1][17] == mo.NON_FINITE and np.all(sick[-1][17] == 0)       # NaN PWMs, the flag, the record untouched
    assert np.all(np.isnan(sick[12][:, 17]))                                 # the loop logs NaN PWMs for that drone
