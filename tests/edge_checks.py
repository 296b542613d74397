"""Checks of the edge-loop kernels (dart_planner_amd/csrc/edge_loop.hip: latency buffer, OnboardController, the loop) that take a harness
(tests/parity_checks.Harness): run by tests/test_emu_edge.py on the host emulation and by tests/test_gpu_edge.py on the device.

References: tests/golden/edge_cases.npz (the reference's own classes, tests/golden/make_golden_edge.py) and tests/edge_oracle.py (pinned to
the reference call by call by that generator).

Bounds.  Single calls in float64: 1e-9, absolute, on every returned value and record word (smoother_checks.tol); clock words, counters and
everything a push returns exact.  Single calls in float32: the project's 1e-4 does not hold for this control law in any sequence, the hover one
included -- each derivative stage multiplies a float32 rounding error by Kd / dt (up to 600), twice in cascade (position PID -> desired roll ->
attitude PID), and the first call's derivative kick commands torques of 1e3 - 5e5 N m -- so the bound is derived as for the loops: per golden
sequence, 4 x the largest difference between the oracle in float64 and the oracle with every stored value rounded to float32 over that sequence's
calls (F32_CALL_TOL; measured by measure_f32_call_difference, which tests/test_emu_edge.py runs and compares with the constants).  The mirror's
private methods are held to the absolute 1e-4 in float32 and 1e-9 in float64.  Loops in
float64: 1e-9 per logged value.  Loops in float32 run a derivative term (error difference / 10 ms, gains up to 6) through up to 300 steps;
their bound is F32_LOOP_TOL = 4 x the largest difference between the oracle in float64 and the oracle with every stored value rounded to
float32 over this file's own loops (the golden loops and the random batches; measured by measure_f32_loop_difference, which
tests/test_emu_edge.py runs and compares with the constant)."""
import json
import os

import numpy as np

import edge_oracle as eo
from dart_planner_amd.capi import LATENCY_STATE_WORDS, ONBOARD_STATE_WORDS, OnboardParams
from smoother_checks import Dev, rounded, tol

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 1e-6
MAX_DISCARDED = 0.05
# The measured float64 / float32 oracle difference over this file's loops (measure_f32_loop_difference, rounded up in the third digit): states
# (positions, velocities, attitudes, body rates) 4.15e-3, commands (thrust in newtons, torques) and controller records 1.27e-2, targets 8.43e-6.
# The bound is 4 x that: the device's rounding order (and its sin / cos) differ from NumPy's.
F32_LOOP_MEASURED = dict(state=4.15e-3, cmd=1.27e-2, target=8.43e-6)
F32_LOOP_TOL = {k: 4.0 * v for k, v in F32_LOOP_MEASURED.items()}
# The same measurement over the calls of each golden sequence (measure_f32_call_difference, rounded up in the third digit): the largest absolute
# float64 / float32 oracle difference of any returned value or record word.  The bound of a float32 single call is 4 x its sequence's figure.
F32_CALL_MEASURED = dict(hover_near_the_plan=5.55e-4, far_below_target_integrals_clamp=5.95e-2, far_above_target_thrust_clipped=7.08e-2,
                         clock_steps_back_and_repeats=5.90e-4, one_row_plan_spinning=1.54e-3, fallback_then_plan=5.99e-4, no_integral_limit_other_mass=7.23e-4,
                         irregular_clock=5.66e-4)
F32_CALL_TOL = {k: 4.0 * v for k, v in F32_CALL_MEASURED.items()}
_cache = {}

# (B, depth, N, shared plan, V present, A present, nsteps): every B crosses or touches a wavefront boundary, every depth wraps its ring
BATCHES = [(1, 1, 0, False, True, True, 40), (63, 2, 2, False, True, False, 40), (64, 5, 6, True, True, True, 60), (65, 9, 30, False, False, False, 300),
           (130, 5, 6, False, False, True, 60), (65, 1, 2, True, False, True, 40), (130, 2, 30, True, True, True, 40), (64, 9, 0, False, True, True, 40)]


def golden():
    """The fixtures, loaded once and shared (read-only)."""
    if "g" not in _cache:
        z = np.load(os.path.join(GOLDEN, "edge_cases.npz"))
        data = {k: z[k] for k in z.files}
        for v in data.values():
            v.setflags(write=False)
        _cache["g"] = (data, json.load(open(os.path.join(GOLDEN, "edge_cases.json"))))
    return _cache["g"]


def golden_plan(data, key):
    return (data[key + "_ts"], data[key + "_P"], data.get(key + "_V"), data.get(key + "_A"))


def call_tol(h, tag):
    """The bound of one call of golden sequence `tag`: every returned value and record word, absolute."""
    return 1e-9 if h.dt == np.float64 else F32_CALL_TOL[tag]


def measure_f32_call_difference():
    """CPU only: per golden sequence, the oracle in float64 against the oracle with every stored value rounded to float32, call by call (each
    run chains through its own record, as a kernel of that precision does) -> {tag: largest absolute difference of any output or record word}."""
    data, meta = golden()
    worst = {}
    for seq in meta["sequences"]:
        key, plan = seq["key"], golden_plan(data, seq["key"] + "plan")
        prm = eo.params(mass=seq["mass"], g=seq["g"], pid=np.array(seq["pid"]))
        runs = []
        for dtype in (np.float64, np.float32):
            st, rows = eo.onboard_reset(1), []
            for e in range(seq["calls"]):
                x = data[key + "x"][e].astype(dtype).astype(float)
                th, tq, tg = eo.control(prm, st, np.array([data[key + "t"][e]]), x[None, 0:3], x[None, 6:9], x[None, 9:12],
                                        rounded(plan, dtype) if data[key + "use_plan"][e] else None, dtype)
                rows.append(np.concatenate([th, tq[0], tg[0], st[0, :12]]).astype(float))
            runs.append(np.array(rows))
        worst[seq["tag"]] = float(np.max(np.abs(runs[0] - runs[1])))
    return worst


def onboard_params(pid=None, mass=1.0, g=9.81) -> OnboardParams:
    rows = {} if pid is None else {name: tuple(pid[i]) for i, name in enumerate(OnboardParams.PID_ROWS)}
    return OnboardParams.reference_defaults(mass=mass, g=g, **rows)


def host(h, a):
    return np.array(h.to_host(a))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Fleet:
    """B drones on the backend: clocks, the four state arrays, the controller records and a latency buffer."""

    def __init__(self, h, t, x, depth):
        dv, ops = Dev(h), h.ops
        x = np.asarray(x, float)
        B = x.shape[0]
        self.h, self.B = h, B
        self.time = dv.d(np.broadcast_to(np.asarray(t, float), (B,)))
        self.pos, self.vel, self.att, self.om = (dv.r(x[:, 3 * i:3 * i + 3]) for i in range(4))
        self.st = ops.onboard_state(B)
        self.buf = ops.latency_buffer(B, depth, "f64" if h.dt == np.float64 else "f32")

    def state(self):
        return (self.time, self.pos, self.vel, self.att, self.om)

    def snapshot(self):
        h = self.h
        arrs = [self.st, self.time, self.pos, self.vel, self.att, self.om]
        if self.buf["depth"] > 0:
            arrs += [self.buf["state"], self.buf["ring_time"], self.buf["ring"]]
        return [host(h, a).copy() for a in arrs]


# ---------------------------------------------------------------------------------------------- golden sequences through the C ABI
def check_golden_sequences(h):
    """Every recorded call of the reference's OnboardController: thrust, torque, target and the whole record; every recorded push of its
    DroneStateLatencyBuffer: the returned state, bit for bit, and the record."""
    data, meta = golden()
    dv, ops, worst = Dev(h), h.ops, {}
    for seq in meta["sequences"]:
        key = seq["key"]
        op = onboard_params(seq["pid"], seq["mass"], seq["g"])
        plan = dv.plan(golden_plan(data, key + "plan"))
        st = ops.onboard_state(1)
        err = 0.0
        for e in range(seq["calls"]):
            x = data[key + "x"][e]
            before = host(h, st).copy()
            args = (op, st, dv.d([data[key + "t"][e]]), dv.r(x[None, 0:3]), dv.r(x[None, 6:9]), dv.r(x[None, 9:12]))
            out = ops.onboard_control(*args, *plan) if data[key + "use_plan"][e] else ops.onboard_control(*args)
            got = np.concatenate([host(h, out["thrust"]).astype(float), host(h, out["torque"]).astype(float)[0], host(h, out["target_pos"]).astype(float)[0]])
            ref = np.concatenate([[data[key + "thrust"][e]], data[key + "torque"][e], data[key + "target"][e]])
            rec, rref = host(h, st).astype(float)[0], data[key + "record"][e]
            assert np.array_equal(rec[12:14], rref[12:14]), (seq["tag"], e)                 # last_time and "is not None": exact
            if not data[key + "use_plan"][e]:
                assert same(host(h, st), before), (seq["tag"], e)                           # the fallback leaves the record alone
            err = max(err, float(np.max(np.abs(got - ref))), float(np.max(np.abs(rec[:12] - rref[:12]))))
        worst[seq["tag"]] = err
    print("edge golden sequences, largest absolute error per sequence:", {k: float("%.3g" % v) for k, v in worst.items()})
    bad = {k: (v, call_tol(h, k)) for k, v in worst.items() if not v <= call_tol(h, k)}
    assert not bad, bad
    for ps in meta["pushes"]:
        key, depth = ps["key"], ps["depth"]
        buf = ops.latency_buffer(1, depth, "f64" if h.dt == np.float64 else "f32")
        for e in range(ps["pushes"]):
            if data[key + "reset"][e]:
                buf = ops.latency_buffer(1, depth, "f64" if h.dt == np.float64 else "f32")
            x = data[key + "x"][e]
            out = ops.latency_push(buf, dv.d([data[key + "t"][e]]), *(dv.r(x[None, 3 * i:3 * i + 3]) for i in range(4)))
            got = np.concatenate([host(h, out[k])[0] for k in ("pos", "vel", "att", "omega")])
            assert np.array_equal(got, data[key + "d_x"][e].astype(h.dt)) and host(h, out["time"])[0] == data[key + "d_t"][e], (depth, e)
            rec, ref = host(h, buf["state"])[0], data[key + "record"][e]                   # ref: len, total_samples, missed_samples, actual_delay_s, last_timestamp
            assert np.array_equal(rec[[0, 2, 3]], ref[[0, 1, 3]]) and min(rec[2], depth) == ref[2], (depth, e, rec, ref)
    return worst


def run_golden_loop(h, loop):
    """One recorded closed loop through edge_loop: one launch per plan segment -> the concatenated logs and the final records."""
    data, _ = golden()
    dv, ops, key = Dev(h), h.ops, loop["key"]
    op, sp = OnboardParams.reference_defaults(), ops.lib.simulator_default_params()
    f = Fleet(h, data[key + "t"][0], data[key + "x"][0][None], loop["depth"])
    zeros = h.to_dev(np.zeros(1, dtype=np.int32))
    n, every = loop["nsteps"], loop["every"]
    cuts = sorted(set([0, n] + [i * every for i in range(loop["plans"])]))
    logs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        plan = dv.plan(golden_plan(data, f"{key}pl{a // every}")) if loop["plans"] else ()
        logs.append(ops.edge_loop(op, sp, f.st, f.buf, *f.state(), *plan, nsteps=b - a, sim_dt=loop["sim_dt"], log=True, zero_thrust_steps=zeros))
    cat = lambda nm: np.concatenate([host(h, l[nm]).astype(float)[:, 0] for l in logs])
    return dict(state=cat("log_state"), cmd=cat("log_cmd"), time=cat("log_time"), target=cat("log_target"), delayed_time=cat("log_delayed_time"),
                onboard=host(h, f.st).astype(float)[0], latency=None if loop["depth"] == 0 else host(h, f.buf["state"])[0], zeros=int(host(h, zeros)[0]),
                final=np.concatenate([host(h, a).astype(float)[0] for a in (f.pos, f.vel, f.att, f.om)] + [host(h, f.time)]))


def check_golden_loops(h):
    data, meta = golden()
    for loop in meta["loops"]:
        key = loop["key"]
        got = run_golden_loop(h, loop)
        ref_cmd = np.concatenate([data[key + "thrust"][:, None], data[key + "torque"]], axis=1)
        e = dict(state=np.max(np.abs(got["state"] - data[key + "x"])), cmd=np.max(np.abs(got["cmd"] - ref_cmd)), target=np.max(np.abs(got["target"] - data[key + "target"])),
                 final=np.max(np.abs(got["final"] - data[key + "final"])), record=np.max(np.abs(got["onboard"][:12] - data[key + "onboard_final"][:12])))
        print("edge golden loop", loop["tag"], {k: float("%.3g" % v) for k, v in e.items()}, "zero-thrust steps", got["zeros"])
        assert np.array_equal(got["time"], data[key + "t"]) and np.array_equal(got["delayed_time"], data[key + "delayed_t"])      # double clock arithmetic: exact
        assert np.array_equal(got["onboard"][12:14], data[key + "onboard_final"][12:14])
        if loop["depth"] > 0:
            ref = data[key + "latency_final"]
            assert np.array_equal(got["latency"][[0, 2, 3]], ref[[0, 1, 3]]), (got["latency"], ref)
        # the stale delayed state: ONE zero command (thrust 0, torque 0, target (0, 0, 0)), at step index `depth`; none without a buffer or a plan
        zero_cmd = np.flatnonzero(np.all(got["cmd"] == 0, axis=1) & np.all(got["target"] == 0, axis=1)).tolist()
        assert zero_cmd == loop["zero_command_steps"], (loop["tag"], zero_cmd)
        assert zero_cmd == ([loop["depth"]] if loop["depth"] > 0 and loop["plans"] else [])
        assert got["zeros"] == loop["zero_thrust_steps"], (got["zeros"], loop["zero_thrust_steps"])
        if h.dt == np.float64:
            assert max(e.values()) <= 1e-9, (loop["tag"], e)
        else:
            assert e["state"] <= F32_LOOP_TOL["state"] and e["final"] <= F32_LOOP_TOL["state"] and e["cmd"] <= F32_LOOP_TOL["cmd"] and e["record"] <= F32_LOOP_TOL["cmd"] \
                and e["target"] <= F32_LOOP_TOL["target"], (loop["tag"], e)


# ---------------------------------------------------------------------------------------------- random batches against the oracle
def random_scene(B, depth, N, shared, with_v, with_a, seed=0):
    """Drones hovering within a few centimetres of their plan's first row, plans that move at walking pace and start 55 ms after the drones'
    clocks (so the sampler is met before, inside and -- the short plans -- behind the plan): the regime of the golden loops, in which the loop
    stays bounded at every depth up to 9 and a clamp decision rarely comes within 1e-6 of its threshold."""
    rng = np.random.default_rng(1000 * seed + 7 * B + 31 * depth + N)
    t0 = 100.0 + rng.uniform(0, 1, B)
    Bp = 1 if shared else B
    x = np.zeros((B, 12))
    plan = None
    if N > 0:
        step = rng.uniform(0.031, 0.097, (Bp, 1))
        k = np.arange(N)[None, :] * step
        v, a = rng.uniform(-0.4, 0.4, (Bp, 1, 3)), rng.uniform(-0.1, 0.1, (Bp, 1, 3))
        base = rng.uniform(-2, 2, (Bp, 1, 3)) + np.array([0, 0, 2.0])
        P = base + v * k[:, :, None] + 0.5 * a * (k * k)[:, :, None]
        V, A = v + a * k[:, :, None], np.broadcast_to(a, (Bp, N, 3)).copy()
        ts = (100.0 if shared else t0[:, None]) + 0.055 + k
        sq = (lambda q: q[0]) if shared else (lambda q: q)
        plan = (sq(ts), sq(P), sq(V) if with_v else None, sq(A) if with_a else None)
        x[:, 0:3] = np.broadcast_to(P[:, 0], (B, 3))
    else:
        x[:, 0:3] = rng.uniform(-2, 2, (B, 3)) + np.array([0, 0, 2.0])
    x[:, 0:3] += rng.normal(0, 0.03, (B, 3))
    x[:, 3:6], x[:, 6:9], x[:, 9:12] = rng.normal(0, 0.05, (B, 3)), rng.normal(0, 0.02, (B, 3)), rng.normal(0, 0.02, (B, 3))
    wind = rng.normal(0, 0.3, (B, 3))
    return t0, x, plan, wind


def oracle_run(case, dtype, seed=0):
    B, depth, N, shared, with_v, with_a, nsteps = case
    t0, x, plan, wind = random_scene(B, depth, N, shared, with_v, with_a, seed)
    st, buf, t, xx = eo.onboard_reset(B), eo.latency_reset(B, depth, dtype), t0.copy(), x.astype(dtype).astype(float)
    log = eo.edge_loop(eo.params(), eo.sim_params(), st, buf, t, xx, rounded(plan, dtype), nsteps, 0.01, wind=wind.astype(dtype).astype(float), dtype=dtype, margin=MARGIN)
    return dict(log=log, st=st, buf=buf, t=t, x=xx)


def check_random_batch(h, case, seed=0):
    B, depth, N, shared, with_v, with_a, nsteps = case
    t0, x, plan, wind = random_scene(B, depth, N, shared, with_v, with_a, seed)
    dv, ops = Dev(h), h.ops
    want = oracle_run(case, np.float64, seed)          # the reference's arithmetic; a float32 kernel is measured against it too
    f = Fleet(h, t0, x, depth)
    zeros = h.to_dev(np.zeros(B, dtype=np.int32))
    got = ops.edge_loop(OnboardParams.reference_defaults(), ops.lib.simulator_default_params(), f.st, f.buf, *f.state(), *(dv.plan(plan) if plan else ()), nsteps=nsteps,
                        sim_dt=0.01, wind=dv.r(wind), log=True, zero_thrust_steps=zeros)
    log = want["log"]
    keep = ~log["near"]                                # (nsteps, B): no decision of this or an earlier step within the margin
    discarded = float(np.mean(~keep))
    assert np.array_equal(host(h, got["log_time"]), log["time"]) and np.array_equal(host(h, got["log_delayed_time"])[keep], log["delayed_time"][keep])
    e = {}
    for nm, key in (("log_state", "state"), ("log_cmd", "cmd"), ("log_target", "target")):
        d = np.max(np.abs(host(h, got[nm]).astype(float) - log[key]), axis=2)
        e[key] = float(np.max(d[keep], initial=0.0))
    last = keep[-1]
    e["final"] = float(np.max(np.abs(np.concatenate([host(h, a).astype(float) for a in (f.pos, f.vel, f.att, f.om)], axis=1) - want["x"])[last], initial=0.0))
    e["record"] = float(np.max(np.abs(host(h, f.st)[:, :12] - want["st"][:, :12])[last], initial=0.0))
    hits = log["hits"][keep].sum(axis=0)
    print(f"edge random batch {case}: discarded {discarded:.4f} of the (drone, step) cases, branches met {dict(zip(eo.BRANCHES, hits.tolist()))}, largest errors "
          f"{ {k: float('%.3g' % v) for k, v in e.items()} }")
    assert discarded <= MAX_DISCARDED, discarded
    assert np.array_equal(host(h, f.st)[last, 12:14], want["st"][last, 12:14])
    if depth > 0:
        assert np.array_equal(host(h, f.buf["state"])[last], want["buf"]["state"][last])
    assert np.array_equal(host(h, zeros)[last], np.sum(log["cmd"][:, :, 0] == 0, axis=0)[last])
    if N > 0 and depth > 0:
        assert np.all(log["hits"][depth, :, 2]) and log["hits"][:, :, 2].sum() == B        # the stale state: once per drone, at step index depth
    if h.dt == np.float64:
        assert max(e.values()) <= 1e-9, e
    else:
        assert e["state"] <= F32_LOOP_TOL["state"] and e["final"] <= F32_LOOP_TOL["state"] and e["cmd"] <= F32_LOOP_TOL["cmd"] and e["record"] <= F32_LOOP_TOL["cmd"] \
            and e["target"] <= F32_LOOP_TOL["target"], e
    return discarded


def measure_f32_loop_difference():
    """CPU only: the oracle in float64 against the oracle with every stored value rounded to float32 over this file's loops (the golden
    loops and the random batches) -> the largest difference per quantity, and the largest discarded fraction of the random batches."""
    data, meta = golden()
    worst, discarded = dict(state=0.0, cmd=0.0, target=0.0), 0.0
    for loop in meta["loops"]:
        key = loop["key"]
        runs = []
        for dtype in (np.float64, np.float32):
            st, buf = eo.onboard_reset(1), eo.latency_reset(1, loop["depth"], dtype)
            t, x = np.array([data[key + "t"][0]]), data[key + "x"][0][None].astype(dtype).astype(float)
            n, every = loop["nsteps"], loop["every"]
            cuts = sorted(set([0, n] + [i * every for i in range(loop["plans"])]))
            logs = [eo.edge_loop(eo.params(), eo.sim_params(), st, buf, t, x, rounded(golden_plan(data, f"{key}pl{a // every}"), dtype) if loop["plans"] else None, b - a,
                                 loop["sim_dt"], dtype=dtype) for a, b in zip(cuts[:-1], cuts[1:])]
            runs.append({k: np.concatenate([l[k] for l in logs]) for k in ("state", "cmd", "target")})
        for k in worst:
            worst[k] = max(worst[k], float(np.max(np.abs(runs[0][k] - runs[1][k]))))
    for case in BATCHES:
        a, b = oracle_run(case, np.float64), oracle_run(case, np.float32)
        keep = ~(a["log"]["near"] | b["log"]["near"])
        discarded = max(discarded, float(np.mean(a["log"]["near"])))
        for k in worst:
            worst[k] = max(worst[k], float(np.max(np.max(np.abs(a["log"][k] - b["log"][k]), axis=2)[keep], initial=0.0)))
    return worst, discarded


# ---------------------------------------------------------------------------------------------- bit for bit
def _fleet_and_plan(h, B, depth, N=6, seed=3):
    t0, x, plan, wind = random_scene(B, depth, N, False, True, True, seed)
    dv = Dev(h)
    return (lambda: Fleet(h, t0, x, depth)), dv.plan(plan), dv.r(wind)


def check_bit_for_bit(h, B, depth, nsteps):
    """edge_loop(nsteps) == nsteps chained latency_push -> onboard_control -> simulator_step launches: states, clocks, records, the ring and
    the logs, bit for bit."""
    ops = h.ops
    op, sp = OnboardParams.reference_defaults(), ops.lib.simulator_default_params()
    make, plan, wind = _fleet_and_plan(h, B, depth)
    one = make()
    log = ops.edge_loop(op, sp, one.st, one.buf, *one.state(), *plan, nsteps=nsteps, sim_dt=0.01, wind=wind, log=True)
    ch = make()
    for step in range(nsteps):
        before = np.concatenate([host(h, a) for a in (ch.pos, ch.vel, ch.att, ch.om)], axis=1)
        t_before = host(h, ch.time).copy()
        d = ops.latency_push(ch.buf, *ch.state())
        cmd = ops.onboard_control(op, ch.st, d["time"], d["pos"], d["att"], d["omega"], *plan)
        ops.simulator_step(sp, *ch.state(), cmd["thrust"], cmd["torque"], 0.01, wind=wind)
        assert same(host(h, log["log_state"])[step], before) and same(host(h, log["log_time"])[step], t_before), step
        assert same(host(h, log["log_cmd"])[step], np.concatenate([host(h, cmd["thrust"])[:, None], host(h, cmd["torque"])], axis=1)), step
        assert same(host(h, log["log_target"])[step], host(h, cmd["target_pos"])) and same(host(h, log["log_delayed_time"])[step], host(h, d["time"])), step
    for a, b in zip(one.snapshot(), ch.snapshot()):
        assert same(a, b), "the chained launches differ from the one launch"
    late = make()                                                        # the measurement variant: each entry loaded by the push that pops it
    ops.lib.set_edge_loop_variant(1)
    try:
        log_late = ops.edge_loop(op, sp, late.st, late.buf, *late.state(), *plan, nsteps=nsteps, sim_dt=0.01, wind=wind, log=True)
    finally:
        ops.lib.set_edge_loop_variant(0)
    for a, b in zip(one.snapshot(), late.snapshot()):
        assert same(a, b), "loading the popped entry late changes the bits"
    assert all(same(host(h, log[k]), host(h, log_late[k])) for k in log)
    assert nsteps > depth and np.all(host(h, one.buf["state"])[:, 0] == depth)


def check_split_launches(h, B=65, depth=5, nsteps=23):
    """A run split into two launches equals the whole run bit for bit: split inside the filling phase and after the ring has wrapped."""
    ops = h.ops
    op, sp = OnboardParams.reference_defaults(), ops.lib.simulator_default_params()
    make, plan, wind = _fleet_and_plan(h, B, depth)
    run = lambda f, n: ops.edge_loop(op, sp, f.st, f.buf, *f.state(), *plan, nsteps=n, sim_dt=0.01, wind=wind, log=True)
    whole = make()
    lw = run(whole, nsteps)
    for cut in (depth - 2, 2 * depth + 3):
        assert 0 < cut < nsteps
        two = make()
        la, lb = run(two, cut), run(two, nsteps - cut)
        for a, b in zip(whole.snapshot(), two.snapshot()):
            assert same(a, b), cut
        for nm in lw:
            assert same(host(h, lw[nm]), np.concatenate([host(h, la[nm]), host(h, lb[nm])])), (cut, nm)


def check_differing_ring_positions(h, B=70, depth=5):
    """Drones whose buffers were reset at different steps sit at different ring slots inside one wavefront: every drone still equals a run of
    its own (a fleet in which ALL drones were reset at that step)."""
    ops = h.ops
    op, sp = OnboardParams.reference_defaults(), ops.lib.simulator_default_params()
    make, plan, wind = _fleet_and_plan(h, B, depth)
    run = lambda f, n: ops.edge_loop(op, sp, f.st, f.buf, *f.state(), *plan, nsteps=n, sim_dt=0.01, wind=wind)
    groups = [np.arange(B) % 3 == g for g in range(3)]                  # group g is reset after 3 * g + ... steps
    resets = (0, 3, 7)

    def fly(mask_of):
        f = make()
        done = 0
        for g, at in enumerate(resets):
            run(f, at - done)
            done = at
            rec = host(h, f.buf["state"]).copy()
            rec[mask_of(g)] = 0.0                                          # LatencyBuffer.reset (latency.py:104-111)
            f.buf["state"] = h.to_dev(rec)
        run(f, 19 - done)
        return f

    mixed = fly(lambda g: groups[g])
    heads = host(h, mixed.buf["state"])[:, 1]
    assert len(set(heads[:64].tolist())) == 3, heads[:64]                  # three ring positions inside the first wavefront
    for g in range(3):
        alone = fly(lambda gg, g=g: np.ones(B, bool) if gg == g else np.zeros(B, bool))
        for a, b in zip(mixed.snapshot()[:7], alone.snapshot()[:7]):
            assert same(a[groups[g]], b[groups[g]]), g


# ---------------------------------------------------------------------------------------------- ClosedLoopMonteCarlo.run_edge
def check_run_edge(h, B=5, N=8, cycles=3, substeps=12):
    """run_edge == per cycle one solve and one edge_loop launch on the solver's outputs, by hand; run() is untouched by it."""
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    rng = np.random.default_rng(11)
    dv, ops = Dev(h), h.ops
    prm = Params.reference_defaults(horizon=N)
    mc = ClosedLoopMonteCarlo(ops, prm)
    p0, v0, goal = dv.r(rng.uniform(-1, 1, (B, 3)) + [0, 0, 2]), dv.r(rng.normal(0, 0.2, (B, 3))), dv.r(rng.uniform(-3, 3, (B, 3)) + [0, 0, 2])
    sim_dt = 0.0025
    suf = "f64" if h.dt == np.float64 else "f32"
    for depth, log in ((5, False), (0, True), (2, True)):
        r = mc.run_edge(p0, v0, goal, cycles, substeps, sim_dt, latency_depth=depth, log=log)
        op = ops.lib.onboard_default_params()
        pos, vel, att, om = p0.clone(), v0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        time, st, buf = dv.d(np.zeros(B)), ops.onboard_state(B), ops.latency_buffer(B, depth, suf)
        zeros = h.to_dev(np.zeros(B, dtype=np.int32))
        for c in range(cycles):
            sol = ops.solve(prm, pos, vel, goal, want_trajectory="accelerations")
            X = sol["x"]
            ops.edge_loop(op, mc.simulator, st, buf, time, pos, vel, att, om, dv.d((c * substeps * sim_dt) + np.arange(N) * prm.dt), X, X[:, 3 * N:], sol["accelerations"],
                          nsteps=substeps, sim_dt=sim_dt, strides=(9 * N, 9 * N, 3 * N), zero_thrust_steps=zeros)
        for got, want in ((r["pos"], pos), (r["vel"], vel), (r["att"], att), (r["omega"], om), (r["time"], time), (r["onboard_state"], st), (r["zero_thrust_steps"], zeros)):
            assert same(host(h, got), host(h, want))
        if depth > 0:
            assert same(host(h, r["latency"]["state"]), host(h, buf["state"])) and same(host(h, r["latency"]["ring"]), host(h, buf["ring"]))
            assert np.all(host(h, r["zero_thrust_steps"]) >= 1)           # the stale delayed state at step `depth` of the first cycle
        assert len(r["logs"]) == (cycles if log else 0) and "controller_state" not in r
    plain = mc.run(p0, v0, goal, cycles, substeps, sim_dt)
    assert "onboard_state" not in plain and np.all(np.isfinite(host(h, plain["pos"])))


# ---------------------------------------------------------------------------------------------- the mirror classes
def check_mirror(h, monkeypatch):
    """The golden sequences through dart_planner_amd.control.onboard_controller.OnboardController and dart_planner_amd.utils.latency_buffer's
    classes; the private methods against the reference's recorded returns; the buffer sizes; the generic buffer; the compat imports."""
    import importlib
    import sys
    from dart_planner_amd.common.types import DroneState, Trajectory
    import dart_planner_amd.control.onboard_controller as mod
    import dart_planner_amd.utils.latency_buffer as lat
    from dart_planner_amd.utils.pid_controller import PIDController
    data, meta = golden()
    prec = "f64" if h.dt == np.float64 else "f32"

    def make(**kw):
        c = mod.OnboardController(precision=prec, **kw)
        c._ops = h.ops
        return c

    traj = lambda plan: Trajectory(timestamps=plan[0], positions=plan[1], velocities=plan[2], accelerations=plan[3])
    state = lambda t, x: DroneState(timestamp=float(t), position=np.array(x[0:3], float), velocity=np.array(x[3:6], float), attitude=np.array(x[6:9], float),
                                    angular_velocity=np.array(x[9:12], float))
    names = ("pos_x_pid", "pos_y_pid", "pos_z_pid", "roll_pid", "pitch_pid", "yaw_rate_pid")
    for seq in meta["sequences"]:
        key = seq["key"]
        c = make(mass=seq["mass"], g=seq["g"])
        for name, (kp, ki, kd, lim) in zip(names, seq["pid"]):
            setattr(c, name, PIDController(kp, ki, kd, integral_limit=lim or None))     # replaced objects, as the generator did on the reference
        assert c.last_time is None
        plan = traj(golden_plan(data, key + "plan"))
        for e in range(seq["calls"]):
            s = state(data[key + "t"][e], data[key + "x"][e])
            if data[key + "use_plan"][e]:
                cmd, tg = c.compute_control_command(s, plan)
            else:
                cmd, tg = c.get_fallback_command(s), s.position
            got = np.concatenate([[cmd.thrust], cmd.torque, tg])
            ref = np.concatenate([[data[key + "thrust"][e]], data[key + "torque"][e], data[key + "target"][e]])
            rref = data[key + "record"][e]
            assert np.max(np.abs(got - ref)) <= call_tol(h, seq["tag"]), (seq["tag"], e, float(np.max(np.abs(got - ref))))
            assert c.last_time == (rref[12] if rref[13] else None)
        assert abs(c.pos_z_pid.integral - rref[2]) <= call_tol(h, seq["tag"]) and abs(c.yaw_rate_pid.last_error - rref[11]) <= call_tol(h, seq["tag"])
        c.reset()
        assert c.last_time is None and c.roll_pid.integral == 0.0 and c.pos_x_pid.last_error == 0.0
    # the private methods at the reference's recorded arguments
    c = make()
    for a, y, ref in zip(data["m_att_acc"], data["m_att_yaw"], data["m_att_out"]):
        assert np.max(np.abs(np.array(c._compute_desired_attitude_and_thrust(a, float(y))) - ref)) <= tol(h)
    assert c.last_time is None and not np.any(c._record())               # ... on scratch records: self's was not touched
    for x, dt, (r, p), ref, rec in zip(data["m_torque_x"], data["m_torque_dt"], data["m_torque_set"], data["m_torque_out"], data["m_torque_record"]):
        assert np.max(np.abs(c._compute_torque(float(r), float(p), 0.0, state(0.0, x), float(dt)) - ref)) <= tol(h)
        assert np.max(np.abs(c._record()[:12] - rec[:12])) <= tol(h) and c.last_time is None
    c = make()
    for x, dt, tp, ta, ref, rec in zip(data["m_torque_x"], data["m_torque_dt"], data["m_plan_tp"], data["m_plan_ta"], data["m_plan_out"], data["m_plan_record"]):
        assert np.max(np.abs(np.array(c.plan(state(0.0, x), tp, ta, float(dt))) - ref)) <= tol(h)
        assert np.max(np.abs(c._record()[:12] - rec[:12])) <= tol(h)
    c = make()
    for x, dt, (r, p), ref, rec in zip(data["m_torque_x"], data["m_torque_dt"], data["m_torque_set"], data["m_act_out"], data["m_act_record"]):
        cmd = c.act(state(0.0, x), float(r), float(p), float(ref[4]), float(dt))
        assert cmd.thrust == ref[0] == ref[4] and np.max(np.abs(cmd.torque - ref[1:4])) <= tol(h)
        assert np.max(np.abs(c._record()[:12] - rec[:12])) <= tol(h)
    import pytest
    with pytest.raises(ValueError):
        c._compute_torque(0.0, 0.0, 0.1, state(0.0, data["m_torque_x"][0]), 0.01)
    pl = golden_plan(data, "q00_plan")
    for t in (pl[0][0] - 1.0, pl[0][3] + 0.013, pl[0][-1] + 1.0):
        ref = eo.sample(np.array([t]), rounded(pl, h.dt), np.float64)
        assert np.max(np.abs(np.concatenate(c._interpolate_trajectory(float(t), traj(pl))) - np.concatenate([r[0] for r in ref[:3]]))) <= tol(h)
    # the latency buffers
    sizes = meta["buffer_sizes"]
    assert [lat.LatencyBuffer(d / 1000.0, sizes["dt"]).buffer_size for d in sizes["delays_ms"]] == sizes["sizes"]
    assert [lat.create_latency_buffer(d, sizes["dt"] * 1000.0, "drone_state").buffer_size for d in sizes["delays_ms"][:6]] == sizes["sizes"][:6]
    for ps in meta["pushes"]:
        key, depth = ps["key"], ps["depth"]
        b = lat.DroneStateLatencyBuffer(depth * 0.005, 0.005, precision=prec)
        b._ops = h.ops
        assert b.buffer_size == depth and not b.is_ready() and b.total_samples == 0
        for e in range(ps["pushes"]):
            if data[key + "reset"][e]:
                b.reset()
                assert len(b.buffer) == 0 and b.total_samples == 0 and b.get_delayed_data() is None
            s = state(data[key + "t"][e], data[key + "x"][e])
            d = b.push(s, float(data[key + "t"][e]))
            ref = data[key + "record"][e]                                  # len, total_samples, missed_samples, actual_delay_s, last_timestamp
            filling = ref[1] <= depth
            assert (d is s) if filling else (d is not s and d is b.get_delayed_data())
            got = np.concatenate([d.position, d.velocity, d.attitude, d.angular_velocity])
            want = data[key + "d_x"][e] if filling else data[key + "d_x"][e].astype(h.dt).astype(float)      # (filling: the very object that was pushed)
            assert np.array_equal(got, want) and d.timestamp == data[key + "d_t"][e]
            assert [len(b.buffer), b.total_samples, b.missed_samples, b.actual_delay_s, b.last_timestamp] == ref.tolist()
            assert b.get_statistics()["fill_percentage"] == ref[0] / depth * 100 and b.is_ready() == (ref[0] == depth)
    with pytest.raises(ValueError, match="position and velocity"):
        b.push(object())
    b.total_samples, b.actual_delay_s = 3, 0.25                             # assigned as on the reference: the record's words follow
    assert (b.total_samples, b.missed_samples, b.actual_delay_s) == (3, 3, 0.25) and b._record()[2] == 3.0
    with pytest.raises(AttributeError):
        b.missed_samples = 7
    g = lat.LatencyBuffer(0.025, 0.005)                                    # the generic buffer: a host container
    assert [g.push(f"data_{i}", 10.0 + i) for i in range(7)] == ["data_0", "data_1", "data_2", "data_3", "data_4", "data_0", "data_1"]
    assert g.get_statistics() == dict(requested_delay_s=0.025, actual_delay_s=5.0, buffer_size=5, required_size=5, total_samples=7, missed_samples=5, fill_percentage=100.0)
    # import shims
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dart_planner_amd", "compat")
    monkeypatch.syspath_prepend(compat)
    for m in [m for m in sys.modules if m == "dart_planner" or m.startswith("dart_planner.")]:
        monkeypatch.delitem(sys.modules, m)
    assert importlib.import_module("dart_planner.control.onboard_controller").OnboardController is mod.OnboardController
    assert importlib.import_module("dart_planner.utils.latency_buffer").DroneStateLatencyBuffer is lat.DroneStateLatencyBuffer
    assert importlib.import_module("dart_planner.utils.pid_controller").PIDController is PIDController


# ---------------------------------------------------------------------------------------------- arguments, B = 0, dirty buffers, NaN drone
def check_invalid_arguments(h):
    dv, ops, lib = Dev(h), h.ops, h.ops.lib
    suf = "f64" if h.dt == np.float64 else "f32"
    B, N, depth = 3, 4, 2
    op, sp = OnboardParams.reference_defaults(), lib.simulator_default_params()
    ptr = ops.be.ptr
    f = Fleet(h, 1.0, np.zeros((B, 12)), depth)
    ts, P = dv.d(1.0 + np.arange(N) * 0.1), dv.r(np.ones((N, 3)))
    out = [dv.r(np.full((B, 3), 7.0)) for _ in range(4)] + [dv.d(np.full(B, 7.0))]
    th, tq, tg = dv.r(np.full(B, 7.0)), dv.r(np.full((B, 3), 7.0)), dv.r(np.full((B, 3), 7.0))
    before = f.snapshot()
    plan = lambda n=N, t=ts, p=P, s=(0, 0, 0, 0): [n, ptr(t), s[0], ptr(p), s[1], 0, s[2], 0, s[3]]

    def push(B_=B, depth_=depth, time_=f.time, pos_=f.pos, ring=f.buf["ring"], rt=f.buf["ring_time"], st=f.buf["state"], d_time=out[4]):
        return lib.loop_status("latency_push", suf, B_, depth_, ptr(time_), ptr(pos_), ptr(f.vel), ptr(f.att), ptr(f.om), ptr(ring), ptr(rt), ptr(st), ptr(d_time),
                               ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), 0)

    def control(op_=op, B_=B, time_=f.time, pos_=f.pos, pl=None, st=f.st):
        return lib.loop_status("onboard_control", suf, op_, B_, ptr(time_), ptr(pos_), ptr(f.att), ptr(f.om), *(plan() if pl is None else pl), ptr(st), ptr(th), ptr(tq),
                               ptr(tg), 0)

    def loop(op_=op, sp_=sp, B_=B, nsteps=2, sim_dt=0.01, pl=None, time_=f.time, pos_=f.pos, st=f.st, depth_=depth, ring=f.buf["ring"], rt=f.buf["ring_time"],
             lst=f.buf["state"], wind_stride=0, gust_step=-1):
        return lib.loop_status("edge_loop", suf, op_, sp_, B_, nsteps, sim_dt, *(plan() if pl is None else pl), ptr(time_), ptr(pos_), ptr(f.vel), ptr(f.att), ptr(f.om),
                               ptr(st), depth_, ptr(ring), ptr(rt), ptr(lst), 0, wind_stride, gust_step, None, 0, 0, 0, 0, 0, 0, 0)

    NULL, SHAPE, PARAM = -1, -3, -4
    nan, inf = float("nan"), float("inf")
    bad = [op.copy(mass=0.0), op.copy(mass=-1.0), op.copy(mass=nan), op.copy(g=inf), op.copy(first_dt=nan), op.copy(pos_x=(nan, 1, 5, 2)), op.copy(roll=(8, 0, inf, 1)),
           op.copy(yaw_rate=(4, 0, 1, nan)), op.copy(pos_z=(12, -inf, 6, 2))]
    for bp in bad:
        assert control(op_=bp) == PARAM and loop(op_=bp) == PARAM
        assert "onboard parameters" in lib.last_error()
    assert control(op_=None) == NULL and loop(op_=None) == NULL and loop(sp_=None) == NULL
    for fn in (push, control, loop):
        assert fn(B_=-1) == SHAPE
    assert push(depth_=0) == SHAPE and push(depth_=1001) == SHAPE and push(depth_=-1) == SHAPE
    assert loop(depth_=-1) == SHAPE and loop(depth_=1001) == SHAPE and loop(nsteps=-1) == SHAPE and loop(wind_stride=-1) == SHAPE
    assert loop(pl=plan(n=-1)) == SHAPE and loop(pl=plan(n=4097)) == SHAPE and loop(pl=plan(s=(0, -1, 0, 0))) == SHAPE
    assert control(pl=plan(n=-1)) == SHAPE and control(pl=plan(s=(-1, 0, 0, 0))) == SHAPE
    assert loop(sim_dt=nan) == PARAM and loop(sim_dt=inf) == PARAM
    assert push(time_=None) == NULL and push(pos_=None) == NULL and push(ring=None) == NULL and push(rt=None) == NULL and push(st=None) == NULL and push(d_time=None) == NULL
    assert control(time_=None) == NULL and control(pos_=None) == NULL and control(st=None) == NULL and control(pl=plan(p=None)) == NULL and control(pl=plan(t=None)) == NULL
    assert loop(time_=None) == NULL and loop(pos_=None) == NULL and loop(st=None) == NULL and loop(pl=plan(t=None)) == NULL
    assert loop(ring=None) == NULL and loop(rt=None) == NULL and loop(lst=None) == NULL and loop(gust_step=0) == NULL
    assert lib._dll.se3mpc_latency_reset(-1, 2, ptr(f.buf["state"]), 0) == SHAPE and lib._dll.se3mpc_latency_reset(B, 0, ptr(f.buf["state"]), 0) == SHAPE
    assert lib._dll.se3mpc_latency_reset(B, 1001, ptr(f.buf["state"]), 0) == SHAPE and lib._dll.se3mpc_latency_reset(B, 2, None, 0) == NULL
    assert lib._dll.se3mpc_onboard_reset(-1, ptr(f.st), 0) == SHAPE and lib._dll.se3mpc_onboard_reset(B, None, 0) == NULL
    assert lib._dll.se3mpc_onboard_default_params(None) == NULL
    # no-ops: B = 0 and nsteps = 0 (with every pointer NULL)
    none = [0] * 9
    assert lib.loop_status("latency_push", suf, 0, 1, *([0] * 14)) == 0
    assert lib.loop_status("onboard_control", suf, op, 0, 0, 0, 0, 0, *none, 0, 0, 0, 0, 0) == 0
    assert loop(B_=0) == 0 and loop(nsteps=0) == 0
    assert lib._dll.se3mpc_latency_reset(0, 1, None, 0) == 0 and lib._dll.se3mpc_onboard_reset(0, None, 0) == 0
    # every rejected call launched nothing
    for a, b in zip(f.snapshot(), before):
        assert same(a, b)
    for a in out + [th, tq, tg]:
        assert np.all(host(h, a) == 7.0)
    assert bytes(lib.onboard_default_params()) == bytes(OnboardParams.reference_defaults())
    # the loop without a buffer takes NULL for the buffer's three operands; without a plan, NULL plans
    assert loop(depth_=0, ring=None, rt=None, lst=None) == 0 and loop(pl=none) == 0
    # front-end shape checks
    import pytest
    with pytest.raises(ValueError):
        ops.onboard_control(op, dv.d(np.zeros((B, 13))), f.time, f.pos, f.att, f.om, ts, P)
    with pytest.raises(ValueError):
        ops.latency_push(ops.latency_buffer(B + 1, 2, suf), *f.state())
    with pytest.raises(ValueError):
        ops.latency_buffer(B, 1001, suf)
    with pytest.raises(ValueError):
        ops.edge_loop(op, sp, f.st, f.buf, f.time, f.pos, f.vel, f.att, dv.r(np.zeros((B + 1, 3))), ts, P)


def check_dirty_buffers_and_nan_drone(h, B=66, depth=3, N=6):
    """Outputs are fully written whatever they held; a drone whose state and clock are NaN leaves its neighbours' bits alone; a record whose
    length or slot lies outside the ring reads as an empty buffer.

    Every buffer an entry point writes without reading (the records the resets fill, the ring, the delayed state, the command and the six
    logs) is handed to the C ABI filled with one byte pattern: 0xFF in one run, 0x7B in the next.  An element the kernels leave unwritten --
    or a ring slot read before it was written -- keeps its pattern and so differs between the two runs."""
    t0, x, plan, wind = random_scene(B, depth, N, False, True, True, 5)
    dv, ops, lib = Dev(h), h.ops, h.ops.lib
    ptr, suf, nsteps = ops.be.ptr, "f64" if h.dt == np.float64 else "f32", 8
    op, sp = OnboardParams.reference_defaults(), lib.simulator_default_params()

    def run(poison, byte, wild=None):
        def dirty(shape, dtype):
            a = np.empty(shape, dtype=dtype)
            a.view(np.uint8)[...] = byte
            return h.to_dev(a)

        x_, t_ = x.copy(), t0.copy()
        if poison is not None:
            x_[poison] = np.nan; t_[poison] = np.nan
        time, (pos, vel, att, om) = dv.d(t_), (dv.r(x_[:, 3 * i:3 * i + 3]) for i in range(4))
        st, lst = dirty((B, ONBOARD_STATE_WORDS), np.float64), dirty((B, LATENCY_STATE_WORDS), np.float64)
        lib.onboard_reset(B, ptr(st), ops.be.stream())
        lib.latency_reset(B, depth, ptr(lst), ops.be.stream())
        if wild is not None:
            rec = host(h, lst).copy()
            rec[wild] = [depth, 1e9, 0.0, 0.0]                             # a full buffer whose oldest slot lies far outside the ring
            lst = h.to_dev(rec)
        ring, rt = dirty((depth, 12, B), h.dt), dirty((depth, B), np.float64)
        dplan = dv.plan(plan)                                              # (kept alive: pl holds its addresses only)
        pl = ops._plan_ptrs(B, suf, *dplan, None)
        d = [dirty((B, 3), h.dt) for _ in range(4)] + [dirty((B,), np.float64)]
        lib.loop_call("latency_push", suf, B, depth, ptr(time), ptr(pos), ptr(vel), ptr(att), ptr(om), ptr(ring), ptr(rt), ptr(lst), ptr(d[4]), ptr(d[0]), ptr(d[1]),
                      ptr(d[2]), ptr(d[3]), ops.be.stream())
        th, tq, tg = dirty((B,), h.dt), dirty((B, 3), h.dt), dirty((B, 3), h.dt)
        lib.loop_call("onboard_control", suf, op, B, ptr(d[4]), ptr(d[0]), ptr(d[2]), ptr(d[3]), *pl, ptr(st), ptr(th), ptr(tq), ptr(tg), ops.be.stream())
        logs = [dirty((nsteps, B, 12), h.dt), dirty((nsteps, B, 4), h.dt), dirty((nsteps, B), np.float64), dirty((nsteps, B, 3), h.dt), dirty((nsteps, B), np.float64)]
        dw = dv.r(wind)
        lib.loop_call("edge_loop", suf, op, sp, B, nsteps, 0.01, *pl, ptr(time), ptr(pos), ptr(vel), ptr(att), ptr(om), ptr(st), depth, ptr(ring), ptr(rt), ptr(lst), ptr(dw), 3,
                      -1, None, *(ptr(l) for l in logs), 0, ops.be.stream())
        return [host(h, o) for o in d + [th, tq, tg] + logs + [st, lst, ring, rt, pos, time]]

    drone_axis = lambda a: 0 if a.shape[0] == B else (a.ndim - 1 if a.shape[-1] == B else 1)      # (B, ..), (depth, 12, B) / (depth, B), (nsteps, B, ..)
    clean, again, sick = run(None, 0xFF), run(None, 0x7B), run(17, 0xFF)
    for a, b in zip(clean, again):
        assert same(a, b)                                                  # nothing kept the bytes it was handed
    for a in clean:
        assert np.all(np.isfinite(a))                                      # (0xFF.. is a NaN)
    others = np.arange(B) != 17
    for a, c in zip(clean, sick):
        assert same(np.ascontiguousarray(np.compress(others, a, axis=drone_axis(a))), np.ascontiguousarray(np.compress(others, c, axis=drone_axis(a))))
    assert np.all(np.isnan(sick[8][:, 17, 0:3]))
    wild = run(None, 0xFF, wild=5)                                         # drone 5's record points outside the ring: it starts over, nobody else notices
    for a, c in zip(clean, wild):
        keep = np.arange(B) != 5
        assert same(np.ascontiguousarray(np.compress(keep, a, axis=drone_axis(a))), np.ascontiguousarray(np.compress(keep, c, axis=drone_axis(a))))
    assert np.array_equal(wild[14][5, 0:3], [depth, (nsteps + 1) % depth, nsteps + 1.0])      # len, oldest slot, total_samples of a buffer that started empty
