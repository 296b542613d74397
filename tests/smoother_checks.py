"""Checks of the TrajectorySmoother kernels (dart_planner_amd/csrc/smoother.hip) that take a harness (tests/parity_checks.Harness): run by
tests/test_emu_smoother.py on the host emulation and by tests/test_gpu_smoother.py on the device.

References: tests/golden/smoother_cases.npz (the reference's own class, tests/golden/make_golden_smoother.py) and tests/smoother_oracle.py
(pinned to those vectors by tests/test_smoother_oracle_golden.py).

Bounds.  float64: 1e-9 per call and per loop step, branch codes and flag bits exact, clock words exact.  float32: 1e-4 on every position /
velocity / acceleration of a single call (tests/parity_checks.py F32["pos"]); closed loops: the bound of
controller_checks.check_closed_loop_vs_oracle (median over the loops of the largest state error <= 5e-3, at least 90 % of them <= 5e-2)."""
import json
import os

import numpy as np

import smoother_oracle as so
from dart_planner_amd.capi import SMOOTHER_STATE_WORDS, SmootherParams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 1e-6
_cache = {}


def golden():
    """The fixtures, loaded once and shared (read-only)."""
    if "g" not in _cache:
        z = np.load(os.path.join(GOLDEN, "smoother_cases.npz"))
        data = {k: z[k] for k in z.files}
        for v in data.values():
            v.setflags(write=False)
        _cache["g"] = (data, json.load(open(os.path.join(GOLDEN, "smoother_cases.json"))))
    return _cache["g"]


def golden_plan(data, key, pi):
    return (data[f"{key}pl{pi}_ts"], data[f"{key}pl{pi}_P"], data.get(f"{key}pl{pi}_V"), data.get(f"{key}pl{pi}_A"))


def params_of(seq) -> SmootherParams:
    return SmootherParams.reference_defaults(transition_time=seq["transition_time"], **seq["members"])


def tol(h):
    return 1e-9 if h.dt == np.float64 else 1e-4


class Dev:
    """Host arrays -> backend arrays of the harness's precision (clocks and records float64)."""

    def __init__(self, h):
        self.h = h

    def r(self, a):
        return None if a is None else self.h.to_dev(np.ascontiguousarray(np.asarray(a).astype(self.h.dt)))

    def d(self, a):
        return self.h.to_dev(np.array(a, dtype=np.float64))          # (a copy: the fixtures are read-only)

    def plan(self, plan):
        if plan is None:
            return None
        ts, P, V, A = plan
        return (self.d(ts), self.r(P), self.r(V), self.r(A))


def rounded(plan, dt):
    """The plan as the kernel of precision dt sees it (stamps stay float64)."""
    if plan is None:
        return None
    ts, P, V, A = plan
    r = lambda a: None if a is None else np.asarray(a).astype(dt).astype(float)
    return (np.asarray(ts, float), r(P), r(V), r(A))


# ---------------------------------------------------------------------------------------------- golden sequences through the C ABI
def check_golden_sequences(h, only=None):
    """Every recorded call of the reference's class: the returned triple, the whole state record and the branch code."""
    data, meta = golden()
    dv, ops, worst = Dev(h), h.ops, {}
    for seq in meta["sequences"]:
        if only is not None and seq["tag"] not in only:
            continue
        key, mp = seq["key"], params_of(seq)
        plans = [dv.plan(golden_plan(data, key, pi)) for pi in range(seq["plans"])]
        empty = (dv.d(np.zeros(0)), dv.r(np.zeros((0, 3))), None, None)
        st, cur = ops.smoother_state(1), None
        err = 0.0
        for e in range(seq["events"]):
            t = dv.d([data[key + "t"][e]])
            if data[key + "kind"][e] == 1:
                new = plans[int(data[key + "plan"][e])]
                ops.smoother_update(mp, st, t, *new, old=cur)
                cur = new
            else:
                out = ops.smoother_desired(mp, st, t, dv.r(data[key + "pos"][e][None]), dv.r(data[key + "vel"][e][None]), *(cur or empty))
                x = h.to_host(out["target"]).astype(float)[0]
                assert int(h.to_host(out["branch"])[0]) == int(data[key + "branch"][e]), (seq["tag"], e)
                err = max(err, float(np.max(np.abs(x - data[key + "out"][e]))))
            rec = h.to_host(st).astype(float)[0]
            ref = data[key + "state"][e]
            assert np.array_equal(rec[21:25], ref[21:25]), (seq["tag"], e, rec[21:25], ref[21:25])          # clocks and flag bits: exact
            err = max(err, float(np.max(np.abs(rec[:21] - ref[:21]))))
        worst[seq["tag"]] = err
    print("smoother golden sequences, largest error per sequence:", {k: float("%.3g" % v) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= tol(h)}
    assert not bad, bad
    return worst


def run_golden_loop(h, loop):
    """One recorded closed loop through smoother_update + closed_loop_smoothed (three plans, 100 steps each) -> logs."""
    data, _ = golden()
    dv, ops, key = Dev(h), h.ops, loop["key"]
    cp, sp, mp = ops.lib.controller_default_params(), ops.lib.simulator_default_params(), SmootherParams.reference_defaults()
    st, sm = ops.controller_state(cp, 1), ops.smoother_state(1)
    time, pos, vel = dv.d([data[key + "t"][0]]), dv.r(data[key + "pos"][0][None]), dv.r(data[key + "vel"][0][None])
    att, om = dv.r(data[key + "att"][0][None]), dv.r(data[key + "omega"][0][None])
    wind = None if loop["wind"] is None else dv.r(loop["wind"])
    logs, old = [], None
    for c in range(3):
        new = dv.plan(golden_plan(data, key, c))
        ops.smoother_update(mp, sm, time, *new, old=old)
        logs.append(ops.closed_loop_smoothed(mp, cp, sp, st, sm, time, pos, vel, att, om, *new, nsteps=100, sim_dt=loop["sim_dt"], wind=wind, log=True))
        old = new
    cat = lambda nm: np.concatenate([h.to_host(l[nm]).astype(float)[:, 0] for l in logs])
    return dict(state=cat("log_state"), cmd=cat("log_cmd"), time=cat("log_time"), target=cat("log_target"), sm=h.to_host(sm).astype(float)[0])


def check_golden_loops(h):
    data, meta = golden()
    errs = []
    for loop in meta["loops"]:
        key = loop["key"]
        got = run_golden_loop(h, loop)
        ref_state = np.concatenate([data[key + "pos"], data[key + "vel"], data[key + "att"], data[key + "omega"]], axis=1)
        ref_cmd = np.concatenate([data[key + "thrust"][:, None], data[key + "torque"]], axis=1)
        e = dict(state=np.max(np.abs(got["state"] - ref_state)), cmd=np.max(np.abs(got["cmd"] - ref_cmd)), target=np.max(np.abs(got["target"] - data[key + "target"])),
                 time=np.max(np.abs(got["time"] - data[key + "t"])), record=np.max(np.abs(got["sm"] - data[key + "sm_final"])))
        print("smoother golden loop", loop["tag"], {k: float("%.3g" % v) for k, v in e.items()})
        errs.append(e)
        assert e["time"] <= 1e-9 and got["sm"][24] == data[key + "sm_final"][24]
        if h.dt == np.float64:
            assert max(e.values()) <= 1e-9, (loop["tag"], e)
    if h.dt == np.float32:
        worst = np.array([e["state"] for e in errs])
        assert np.median(worst) <= 5e-3 and np.mean(worst <= 5e-2) >= 0.9, worst
    return errs


def commanded_jump(target):
    return float(np.max(np.linalg.norm(np.diff(target[:, 0:3], axis=0), axis=1)))


def raw_plan_jump(h, loop):
    """The same scene without the smoother: the recorded plans sampled at the recorded clocks by the sampler the unsmoothed loops hand to the
    controller (control_plan's target; one "drone" per control step, each with the plan that step was flown on)."""
    data, _ = golden()
    dv, ops, key = Dev(h), h.ops, loop["key"]
    n = loop["nsteps"]
    per = lambda j: np.stack([np.asarray(golden_plan(data, key, i // 100)[j]) for i in range(n)])
    cp = ops.lib.controller_default_params()
    t = dv.d(data[key + "t"])
    out = ops.control_plan(cp, ops.controller_state(cp, n), t, t, dv.r(data[key + "pos"]), dv.r(data[key + "vel"]), dv.r(data[key + "att"]),
                           dv.r(data[key + "omega"]), dv.d(per(0)), dv.r(per(1)), dv.r(per(2)), dv.r(per(3)), want_target=True)
    return commanded_jump(h.to_host(out["target"]).astype(float))


def check_switch_scene(h):
    """The switching scene (the second plan starts (2, 1, 0) m away): the smoother keeps the largest one-step change of the commanded position at
    the value the reference's own run recorded and below a quarter of the raw jump; the plans sampled without the smoother show the raw jump
    (|(2, 1, 0)| m up to the plans' own motion, the value the reference's run recorded)."""
    _, meta = golden()
    loop = [l for l in meta["loops"] if l["tag"] == "switch"][0]
    jump, raw = commanded_jump(run_golden_loop(h, loop)["target"]), raw_plan_jump(h, loop)
    print("switch scene: commanded jump", jump, "reference", loop["smoothed_jump"], "raw", raw, "reference", loop["raw_jump"])
    assert abs(jump - loop["smoothed_jump"]) <= (1e-6 if h.dt == np.float64 else 1e-4)
    assert abs(raw - loop["raw_jump"]) <= tol(h) and abs(raw - np.sqrt(5.0)) < 0.01
    assert jump < 0.25 * raw


# ---------------------------------------------------------------------------------------------- random batches against the oracle
def random_scene(rng, B, N, shared, with_v, with_a, calls=40):
    """40 calls at 10 ms with updates before calls 0, 15 and 28, per-drone clocks; short transition and timeout so that every branch is met."""
    mp = dict(transition_time=0.083, timeout=0.131)
    Bp = 1 if shared else B
    t0 = 100.0 + rng.uniform(0, 1, B)
    plans = []
    base = rng.uniform(-3, 3, (Bp, 1, 3))
    for c in range(3):
        step = rng.uniform(0.011, 0.029, (Bp, 1))
        k = np.arange(N)[None, :] * step
        v = rng.uniform(-1.5, 1.5, (Bp, 1, 3))
        jump = rng.choice([0.0, 0.2, 0.9, 3.0], (Bp, 1, 1)) * rng.normal(0, 1, (Bp, 1, 3)) if c else 0.0
        if c == 0:
            base[::3] = 0.0                                      # some drones start at the exact origin ...
            v[::3] = np.where(np.arange(Bp)[::3, None, None] % 2 == 0, 0.0, v[::3])    # ... half of them with zero velocity: the filter bypass lasts
        P = base + jump + v * k[:, :, None] + rng.normal(0, 0.01, (Bp, N, 3)) * (k[:, :, None] > 0)
        V = v + rng.normal(0, 0.1, (Bp, N, 3)) * (k[:, :, None] > 0)
        A = rng.normal(0, 0.5, (Bp, N, 3))
        ts = rng.uniform(0, 50, (Bp, 1)) + k
        base = P[:, -1:, :]
        sq = (lambda a: a[0]) if shared else (lambda a: a)
        plans.append((sq(ts), sq(P), sq(V) if with_v else None, sq(A) if with_a else None))
    upd = {0: (0, rng.uniform(-0.004, 0.004, B)), 15: (1, rng.uniform(0.001, 0.009, B)), 28: (2, rng.uniform(0.001, 0.009, B))}
    pos, vel = rng.uniform(-3, 3, (calls, B, 3)), rng.uniform(-2, 2, (calls, B, 3))
    return mp, t0, plans, upd, pos, vel


def check_random_batch(h, B, N, shared=False, with_v=True, with_a=True, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * B + N)
    mpd, t0, plans, upd, pos, vel = random_scene(rng, B, N, shared, with_v, with_a)
    prm, mp = so.params(**mpd), SmootherParams.reference_defaults(**mpd)
    dv, ops = Dev(h), h.ops
    rp = [rounded(p, h.dt) for p in plans]
    dplans = [dv.plan(p) for p in plans]
    ost, dst = so.reset(B), ops.smoother_state(B)
    margin = np.full(B, np.inf)
    cur, dcur = None, None
    seen = np.zeros(5, int)
    worst = 0.0
    bad_branch = np.zeros(B, bool)
    for k in range(pos.shape[0]):
        t = t0 + k * 0.01
        if k in upd:
            pi, off = upd[k]
            d = {}
            so.update(prm, ost, t + off, cur, rp[pi], diag=d)
            margin = np.minimum(margin, d["margin"])
            ops.smoother_update(mp, dst, dv.d(t + off), *dplans[pi], old=dcur)
            cur, dcur = rp[pi], dplans[pi]
        d = {}
        p_, v_ = pos[k].astype(h.dt).astype(float), vel[k].astype(h.dt).astype(float)
        x, br = so.desired(prm, ost, t, p_, v_, cur, diag=d)
        margin = np.minimum(margin, d["margin"])
        out = ops.smoother_desired(mp, dst, dv.d(t), dv.r(pos[k]), dv.r(vel[k]), *dcur)
        keep = margin >= MARGIN
        seen += np.bincount(br[keep], minlength=5)
        bad_branch |= h.to_host(out["branch"]) != br
        rec = h.to_host(dst).astype(float)
        e = np.maximum(np.max(np.abs(h.to_host(out["target"]).astype(float) - x), axis=1), np.max(np.abs(rec[:, :21] - ost[:, :21]), axis=1))
        worst = max(worst, float(np.max(e[keep], initial=0.0)))
        assert np.array_equal(rec[keep, 21:25], ost[keep, 21:25])
    keep = margin >= MARGIN
    print(f"smoother random batch B={B} N={N} shared={shared} V={with_v} A={with_a}: discarded {int((~keep).sum())}, branches met {seen.tolist()}, "
          f"largest error {worst:.3g}")
    assert (~keep).sum() <= 0.02 * B, ("drones inside the margin", int((~keep).sum()), B)
    assert not np.any(bad_branch & keep)
    assert worst <= tol(h), worst
    return seen


def check_empty_plan(h):
    """An empty plan (N = 0) samples as zeros (smoother.py:221-222), as the new plan of an update and as the plan followed."""
    dv, ops = Dev(h), h.ops
    mp, prm = SmootherParams.reference_defaults(), so.params()
    B = 3
    full = (np.arange(4) * 0.1, np.arange(12.0).reshape(4, 3) * 0.1 + 1.0, np.ones((4, 3)) * 0.2, None)
    empty = (np.zeros(0), np.zeros((0, 3)), None, None)
    ost, dst = so.reset(B), ops.smoother_state(B)
    now = np.array([5.0, 5.001, 5.002])
    for t, old, new in ((now, None, full), (now + 0.05, full, empty), (now + 0.1, empty, full)):
        so.update(prm, ost, t, rounded(old, h.dt), rounded(new, h.dt))
        ops.smoother_update(mp, dst, dv.d(t), *dv.plan(new), old=dv.plan(old))
        x, br = so.desired(prm, ost, t + 0.003, np.zeros((B, 3)), np.zeros((B, 3)), rounded(new, h.dt))
        out = ops.smoother_desired(mp, dst, dv.d(t + 0.003), dv.r(np.zeros((B, 3))), dv.r(np.zeros((B, 3))), *dv.plan(new))
        assert np.array_equal(h.to_host(out["branch"]), br)
        assert np.max(np.abs(h.to_host(out["target"]).astype(float) - x)) <= tol(h)
        assert np.max(np.abs(h.to_host(dst).astype(float) - ost)) <= tol(h)
    assert ost[0, 24] == 3                                       # the jump from the plan to the zeros of the empty one started a transition


# ---------------------------------------------------------------------------------------------- bit for bit
def _loop_inputs(rng, B, N):
    ts = 7.0 + np.arange(N) * 0.004
    P = rng.uniform(-2, 2, (B, 1, 3)) + np.cumsum(rng.normal(0, 0.01, (B, N, 3)), axis=1)
    V, A = rng.normal(0, 0.5, (B, N, 3)), rng.normal(0, 0.5, (B, N, 3))
    P2 = P + rng.choice([0.0, 1.0], (B, 1, 1)) * rng.normal(0, 1, (B, 1, 3))
    return ts, P, V, A, P2, P[:, 0] + rng.normal(0, 0.05, (B, 3)), rng.normal(0, 0.2, (B, 3)), rng.normal(0, 0.05, (B, 3)), rng.normal(0, 0.1, (B, 3)), rng.normal(0, 1.0, (B, 3))


def check_bit_for_bit(h, B=65, N=6, n=20):
    """closed_loop_smoothed(nsteps = n) == n chained smoother_desired -> control -> simulator_step launches == two calls of n / 2: states, clocks,
    both records and the logs, bit for bit."""
    rng = np.random.default_rng(5)
    ts, P, V, A, P2, pos, vel, att, om, wind = _loop_inputs(rng, B, N)
    dv, ops = Dev(h), h.ops
    cp, sp = ops.lib.controller_default_params(), ops.lib.simulator_default_params()
    mp = SmootherParams.reference_defaults(transition_time=0.012)          # the transition ends inside the run
    sim_dt = 0.001
    plan1, plan2 = (dv.d(ts), dv.r(P), dv.r(V), dv.r(A)), (dv.d(ts), dv.r(P2), dv.r(V), dv.r(A))

    def start():
        s = dict(st=ops.controller_state(cp, B), sm=ops.smoother_state(B), time=dv.d(np.full(B, 7.0)), pos=dv.r(pos), vel=dv.r(vel), att=dv.r(att), om=dv.r(om))
        ops.smoother_update(mp, s["sm"], s["time"], *plan1)
        ops.smoother_update(mp, s["sm"], dv.d(np.full(B, 7.0)), *plan2, old=plan1)
        return s

    def smoothed(s, steps):
        return ops.closed_loop_smoothed(mp, cp, sp, s["st"], s["sm"], s["time"], s["pos"], s["vel"], s["att"], s["om"], *plan2, nsteps=steps, sim_dt=sim_dt,
                                        wind=dv.r(wind), log=True)

    host = lambda a: np.array(h.to_host(a))
    snap = lambda s: [host(s[k]) for k in ("st", "sm", "time", "pos", "vel", "att", "om")]
    same = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    one = start()
    bits0 = host(one["sm"])[:, 24].copy()
    log_one = smoothed(one, n)
    two = start()
    la, lb = smoothed(two, n // 2), smoothed(two, n - n // 2)
    for a, b in zip(snap(one), snap(two)):
        assert same(a, b), "two calls of n / 2 steps differ from one of n"
    for nm in ("log_state", "log_cmd", "log_time", "log_target"):
        assert same(host(log_one[nm]), np.concatenate([host(la[nm]), host(lb[nm])]))
    ch = start()
    for step in range(n):
        t_before, state_before = host(ch["time"]).copy(), np.concatenate([host(ch[k]) for k in ("pos", "vel", "att", "om")], axis=1)
        tg = ops.smoother_desired(mp, ch["sm"], ch["time"], ch["pos"], ch["vel"], *plan2)["target"]
        tgh = host(tg)
        cmd = ops.control(cp, ch["st"], ch["time"], ch["pos"], ch["vel"], ch["att"], ch["om"], dv.r(tgh[:, 0:3]), dv.r(tgh[:, 3:6]), dv.r(tgh[:, 6:9]))
        ops.simulator_step(sp, ch["time"], ch["pos"], ch["vel"], ch["att"], ch["om"], cmd["thrust"], cmd["torque"], sim_dt, wind=dv.r(wind))
        assert same(host(log_one["log_target"])[step], tgh), step
        assert same(host(log_one["log_time"])[step], t_before) and same(host(log_one["log_state"])[step], state_before), step
        assert same(host(log_one["log_cmd"])[step], np.concatenate([host(cmd["thrust"])[:, None], host(cmd["torque"])], axis=1)), step
    for a, b in zip(snap(one), snap(ch)):
        assert same(a, b), "the chained launches differ from the one launch"
    done = host(one["sm"])[:, 24]
    assert np.any(bits0 == 3) and np.any(bits0 == 1)             # some drones entered the loop inside a transition, some following
    if n * sim_dt > mp.transition_time:
        assert np.all(done == 1)                                 # ... and every transition ran to its end inside the loop (bit 2 set before, cleared after)
    else:
        assert np.array_equal(done, bits0)                       # ... and none could: the loop is shorter than the transition


# ---------------------------------------------------------------------------------------------- ClosedLoopMonteCarlo
def check_monte_carlo_option(h, B=5, N=8, cycles=3, substeps=10):
    """run(smoother=None) is run() byte for byte; run(smoother=...) is the chain solve -> smoother_update -> closed_loop_smoothed; the fused forms
    and capture refuse the option."""
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
    a, b = mc.run(p0, v0, goal, cycles, substeps, sim_dt), mc.run(p0, v0, goal, cycles, substeps, sim_dt, smoother=None)
    for k in ("pos", "vel", "att", "omega", "time", "controller_state"):
        assert np.array_equal(h.to_host(a[k]).view(np.uint8), h.to_host(b[k]).view(np.uint8)), k
    assert "smoother_state" not in b
    mp = SmootherParams.reference_defaults()
    for log in (False, True):
        s = mc.run(p0, v0, goal, cycles, substeps, sim_dt, smoother=mp, log=log)
        # the same cycle by hand
        pos, vel, att, om = p0.clone(), v0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        time = dv.d(np.zeros(B))
        st, sm, old = ops.controller_state(mc.controller, B), ops.smoother_state(B), None
        for c in range(cycles):
            sol = ops.solve(prm, pos, vel, goal)
            new = (dv.d((c * substeps * sim_dt) + np.arange(N) * prm.dt), sol["x"][:, :3 * N].reshape(B, N, 3).contiguous(), sol["x"][:, 3 * N:6 * N].reshape(B, N, 3).contiguous(),
                   sol["accelerations"].reshape(B, N, 3).contiguous())
            ops.smoother_update(mp, sm, time, *new, old=old)
            ops.closed_loop_smoothed(mp, mc.controller, mc.simulator, st, sm, time, pos, vel, att, om, *new, nsteps=substeps, sim_dt=sim_dt)
            old = new
        for got, want in ((s["pos"], pos), (s["vel"], vel), (s["att"], att), (s["omega"], om), (s["time"], time), (s["controller_state"], st), (s["smoother_state"], sm)):
            assert np.array_equal(h.to_host(got).view(np.uint8), h.to_host(want).view(np.uint8))
        assert len(s["logs"]) == (cycles if log else 0)
    assert np.all(h.to_host(s["smoother_state"])[:, 24] >= 1)
    with pytest.raises(ValueError, match="smoother"):
        mc.run_fused(p0, v0, goal, cycles, substeps, sim_dt, smoother=mp)
    with pytest.raises(ValueError, match="smoother"):
        mc.run_mppi_fused(p0, v0, goal, cycles, substeps, sim_dt, 64, 1, 1.0, 1.0, smoother=mp)
    with pytest.raises(ValueError, match="smoother"):
        mc.capture(B, torch.float64, cycles, substeps, sim_dt, smoother=mp)
    # MPPI as the planner: the option runs, and None is today's path
    m0 = mc.run_mppi(p0, v0, goal, 2, substeps, sim_dt, 64, 2, 1.0, 1.0, seed=3)
    m1 = mc.run_mppi(p0, v0, goal, 2, substeps, sim_dt, 64, 2, 1.0, 1.0, seed=3, smoother=None)
    assert np.array_equal(h.to_host(m0["pos"]).view(np.uint8), h.to_host(m1["pos"]).view(np.uint8))
    m2 = mc.run_mppi(p0, v0, goal, 2, substeps, sim_dt, 64, 2, 1.0, 1.0, seed=3, smoother=mp)
    assert np.all(np.isfinite(h.to_host(m2["pos"]))) and np.allclose(h.to_host(m2["time"]), 2 * substeps * sim_dt) and m2["clearance"] is None
    assert np.all(h.to_host(m2["smoother_state"])[:, 24] >= 1)
    # the same two cycles by hand, the plan's three blocks (plan_last (B, 3, N, 3) = P, V, A) copied out into tensors of their own
    st, sm, (time, pos, vel, att, om) = mc._start(p0, v0, mp)
    U = mc._mppi_start(p0, None)
    sh = mc.resolve_shift(substeps, sim_dt, None)
    old = None
    for c in range(2):
        out = ops.mppi_closed_loop(prm, mc.controller, mc.simulator, st, time, pos, vel, att, om, goal, U, 1, 0, sim_dt, 64, 2, 1.0, 1.0, seed=3, cycle_base=c,
                                   shift=sh, want_plan=True, want_clearance=False)
        pl = out["plan_last"]
        assert tuple(pl.shape) == (B, 3, N, 3)
        new = (dv.d((c * substeps * sim_dt) + np.arange(N) * prm.dt), pl[:, 0].contiguous(), pl[:, 1].contiguous(), pl[:, 2].contiguous())
        ops.smoother_update(mp, sm, time, *new, old=old)
        ops.closed_loop_smoothed(mp, mc.controller, mc.simulator, st, sm, time, pos, vel, att, om, *new, nsteps=substeps, sim_dt=sim_dt)
        old = new
    for got, want in ((m2["pos"], pos), (m2["vel"], vel), (m2["att"], att), (m2["omega"], om), (m2["time"], time), (m2["controller_state"], st),
                      (m2["smoother_state"], sm), (m2["U"], U)):
        assert np.array_equal(h.to_host(got).view(np.uint8), h.to_host(want).view(np.uint8))


# ---------------------------------------------------------------------------------------------- the mirror class
def check_mirror(h, monkeypatch):
    """The golden sequences through dart_planner_amd.control.trajectory_smoother.TrajectorySmoother with its module's clock patched; the status
    methods; the private methods against the reference's recorded returns; the compat import and the container accessor."""
    import importlib
    import sys
    from dart_planner_amd.common.types import DroneState, Trajectory
    import dart_planner_amd.control.trajectory_smoother as mod
    data, meta = golden()
    clock = {"t": 0.0}
    monkeypatch.setattr(mod.time, "time", lambda: clock["t"])
    prec = "f64" if h.dt == np.float64 else "f32"

    def make(**kw):
        s = mod.TrajectorySmoother(precision=prec, **kw)
        s._ops = h.ops
        return s

    def traj(plan):
        return Trajectory(timestamps=plan[0], positions=plan[1], velocities=plan[2], accelerations=plan[3])

    state = lambda t, p, v: DroneState(timestamp=float(t), position=np.array(p, float), velocity=np.array(v, float))
    for seq in meta["sequences"]:
        key = seq["key"]
        clock["t"] = 0.0
        s = make(transition_time=seq["transition_time"])
        for k, v in seq["members"].items():
            setattr(s, k, v)
        assert s.get_status() == dict(has_trajectory=False, in_transition=False, last_update_age=0.0, trajectory_valid=False), s.get_status()
        for e in range(seq["events"]):
            t = float(data[key + "t"][e])
            if data[key + "kind"][e] == 1:
                clock["t"] = t
                s.update_trajectory(traj(golden_plan(data, key, int(data[key + "plan"][e]))), state(t, data[key + "pos"][e], data[key + "vel"][e]))
                assert s.is_trajectory_valid() and s.get_status()["last_update_age"] == 0.0
            else:
                out = np.concatenate(s.get_desired_state(t, state(t, data[key + "pos"][e], data[key + "vel"][e])))
                assert np.max(np.abs(out - data[key + "out"][e])) <= tol(h), (seq["tag"], e)
            ref = data[key + "state"][e]
            assert s.in_transition == bool(int(ref[24]) & 2) and s.last_cloud_update == ref[22] and s.trajectory_start_time == ref[23]
        assert np.max(np.abs(s.last_filtered_pos - ref[0:3])) <= tol(h) and np.max(np.abs(s.transition_target_vel - ref[18:21])) <= tol(h)
        clock["t"] = float(ref[22]) + 2.5
        assert s.is_trajectory_valid() is False and abs(s.get_status()["last_update_age"] - 2.5) < 1e-9
    # the private methods at the reference's recorded arguments
    s = make()
    pl = (data["m_plan_ts"], data["m_plan_P"], data["m_plan_V"], data["m_plan_A"])
    for t, ref in zip(data["m_interp_t"], data["m_interp_out"]):
        assert np.max(np.abs(np.concatenate(s._interpolate_trajectory(float(t), traj(pl), float(data["m_interp_start"]))) - ref)) <= tol(h)
    rec = data["m_trans_record"]
    s.transition_start_pos, s.transition_start_vel, s.transition_target_pos, s.transition_target_vel = rec[9:12], rec[12:15], rec[15:18], rec[18:21]
    for p, ref in zip(data["m_trans_progress"], data["m_trans_out"]):
        assert np.max(np.abs(np.concatenate(s._generate_transition_state(float(p))) - ref)) <= tol(h), p
    s.last_cloud_update = 300.0
    for t, p, v, ref in zip(data["m_fail_t"], data["m_fail_pos"], data["m_fail_vel"], data["m_fail_out"]):
        assert np.max(np.abs(np.concatenate(s._get_failsafe_trajectory(float(t), state(t, p, v))) - ref)) <= tol(h)
    rec = data["m_limits_record"]
    s.last_filtered_vel, s.last_filtered_acc = rec[3:6], rec[6:9]
    for x, ref in zip(data["m_limits_in"], data["m_limits_out"]):
        assert np.max(np.abs(np.concatenate(s._apply_trajectory_limits(x[0:3], x[3:6], x[6:9], float(data["m_limits_dt"]))) - ref)) <= tol(h)
    assert np.array_equal(s.last_filtered_vel, np.asarray(rec[3:6]).astype(float))      # the limits alone do not move the filter
    # _smooth_trajectory_point at the reference's recorded arguments: the calls chain through the filter state, which it moves
    rec = data["m_smooth_record"]
    s.last_filtered_pos, s.last_filtered_vel, s.last_filtered_acc = rec[0:3], rec[3:6], rec[6:9]
    for x, ref, after in zip(data["m_limits_in"], data["m_smooth_out"], data["m_smooth_state"]):
        got = np.concatenate(s._smooth_trajectory_point(x[0:3], x[3:6], x[6:9], float(data["m_limits_dt"])))
        assert np.max(np.abs(got - ref)) <= tol(h) and np.max(np.abs(s._record()[0:9] - after[0:9])) <= tol(h)
        assert np.array_equal(s._record()[9:25], np.concatenate([data["m_trans_record"][9:21], [0.0, 300.0, 0.0, 0.0]]))      # nothing else moved
    # current_trajectory assigned directly, as code written against the reference may: the device follows the plan and the record's bit follows
    s = make()
    s.velocity_limit = s.acceleration_limit = s.jerk_limit = float("inf")           # the plain sample: no per-call clamp (the filter is bypassed at the origin)
    s.current_trajectory = traj(pl)
    assert s._record()[24] == 1 and s.get_status()["has_trajectory"] is True
    t = float(data["m_interp_t"][5]) - float(data["m_interp_start"])               # trajectory_start_time stays 0, as in the reference
    assert np.max(np.abs(np.concatenate(s.get_desired_state(t, state(t, (0, 0, 0), (0, 0, 0)))) - data["m_interp_out"][5])) <= tol(h)
    s.current_trajectory = None
    assert s._record()[24] == 0 and s.current_trajectory is None and s.get_status()["has_trajectory"] is False
    out = s.get_desired_state(t, state(t, (1, 2, 3), (4, 5, 6)))
    assert np.array_equal(np.concatenate(out), [1, 2, 3, 0, 0, 0, 0, 0, 0])          # :213 no trajectory
    # import shim and container
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dart_planner_amd", "compat")
    monkeypatch.syspath_prepend(compat)
    for m in [m for m in sys.modules if m == "dart_planner" or m.startswith("dart_planner.")]:
        monkeypatch.delitem(sys.modules, m)
    shim = importlib.import_module("dart_planner.control.trajectory_smoother")
    assert shim.TrajectorySmoother is mod.TrajectorySmoother
    from dart_planner_amd.common.di_container_v2 import get_container, reset_container
    reset_container()
    cc = get_container().create_control_container()
    assert isinstance(cc.get_trajectory_smoother(), mod.TrajectorySmoother) and cc.get_trajectory_smoother() is cc.get_trajectory_smoother()
    reset_container()


# ---------------------------------------------------------------------------------------------- arguments, B = 0, dirty buffers, NaN drone
def check_invalid_arguments(h):
    dv, ops, lib = Dev(h), h.ops, h.ops.lib
    suf = "f64" if h.dt == np.float64 else "f32"
    B, N = 3, 4
    mp, cp, sp = SmootherParams.reference_defaults(), lib.controller_default_params(), lib.simulator_default_params()
    ptr = ops.be.ptr
    now, pos, vel, att, om = dv.d(np.full(B, 1.0)), dv.r(np.zeros((B, 3))), dv.r(np.zeros((B, 3))), dv.r(np.zeros((B, 3))), dv.r(np.zeros((B, 3)))
    ts, P = dv.d(np.arange(N) * 0.1), dv.r(np.ones((N, 3)))
    sm, st = ops.smoother_state(B), ops.controller_state(cp, B)
    before = (np.array(h.to_host(sm)).copy(), np.array(h.to_host(st)).copy(), np.array(h.to_host(pos)).copy())
    tg, br = dv.r(np.full((B, 9), 7.0)), h.to_dev(np.full(B, 7, dtype=np.int32))
    plan = lambda n=N, t=ts, p=P, s=(0, 0, 0, 0): [n, ptr(t), s[0], ptr(p), s[1], 0, s[2], 0, s[3]]
    none = [0, 0, 0, 0, 0, 0, 0, 0, 0]

    def update(mp_=mp, B_=B, now_=now, old=none, new=None, sm_=sm):
        return lib.loop_status("smoother_update", suf, mp_, B_, ptr(now_), *old, *(plan() if new is None else new), ptr(sm_), 0)

    def desired(mp_=mp, B_=B, now_=now, pos_=pos, vel_=vel, pl=None, sm_=sm):
        return lib.loop_status("smoother_desired", suf, mp_, B_, ptr(now_), ptr(pos_), ptr(vel_), *(plan() if pl is None else pl), ptr(sm_), ptr(tg), ptr(br), 0)

    def loop(mp_=mp, cp_=cp, sp_=sp, B_=B, nsteps=2, sim_dt=0.01, pl=None, time_=now, pos_=pos, st_=st, sm_=sm, wind_stride=0, gust_step=-1):
        return lib.loop_status("closed_loop_smoothed", suf, mp_, cp_, sp_, B_, nsteps, sim_dt, *(plan() if pl is None else pl), ptr(time_), ptr(pos_), ptr(vel),
                               ptr(att), ptr(om), ptr(st_), ptr(sm_), 0, wind_stride, gust_step, None, 0, 0, 0, 0, 0)

    NULL, SHAPE, PARAM = -1, -3, -4
    bad_params = [mp.copy(transition_time=0.0), mp.copy(transition_time=-1.0), mp.copy(transition_time=float("nan")), mp.copy(transition_time=float("inf")),
                  mp.copy(update_dt=0.0), mp.copy(update_dt=float("nan")), mp.copy(smoothing_window=0.0), mp.copy(smoothing_window=float("inf"))]
    for bp in bad_params:
        assert update(mp_=bp) == PARAM and desired(mp_=bp) == PARAM and loop(mp_=bp) == PARAM
        assert "smoother parameters" in lib.last_error()
    assert lib.loop_status("smoother_update", suf, None, B, ptr(now), *none, *plan(), ptr(sm), 0) == NULL
    for fn in (update, desired, loop):
        assert fn(B_=-1) == SHAPE
    assert update(now_=None) == NULL and update(sm_=None) == NULL and update(new=plan(p=None)) == NULL and update(new=plan(t=None)) == NULL
    assert update(new=plan(n=-1)) == SHAPE and update(new=plan(n=4097)) == SHAPE and update(old=plan(n=-1)) == SHAPE and update(new=plan(s=(0, -1, 0, 0))) == SHAPE
    assert update(old=plan(s=(-1, 0, 0, 0))) == SHAPE
    assert desired(now_=None) == NULL and desired(pos_=None) == NULL and desired(vel_=None) == NULL and desired(sm_=None) == NULL
    assert desired(pl=plan(p=None)) == NULL and desired(pl=plan(n=-1)) == SHAPE and desired(pl=plan(s=(0, 0, 0, -3))) == SHAPE
    assert loop(nsteps=-1) == SHAPE and loop(wind_stride=-1) == SHAPE and loop(pl=plan(n=-2)) == SHAPE
    assert loop(sim_dt=float("nan")) == PARAM and loop(sim_dt=float("inf")) == PARAM
    assert loop(time_=None) == NULL and loop(pos_=None) == NULL and loop(st_=None) == NULL and loop(sm_=None) == NULL and loop(pl=plan(t=None)) == NULL
    assert loop(gust_step=0) == NULL                                         # a gust step without a gust vector
    assert loop(cp_=None) == NULL and loop(sp_=None) == NULL
    assert lib._dll.se3mpc_smoother_reset(-1, ptr(sm), 0) == SHAPE and lib._dll.se3mpc_smoother_reset(B, None, 0) == NULL
    assert lib._dll.se3mpc_smoother_default_params(None) == NULL
    # no-ops: B = 0 and nsteps = 0 (with every pointer NULL)
    assert lib.loop_status("smoother_update", suf, mp, 0, 0, *none, *none, 0, 0) == 0
    assert lib.loop_status("smoother_desired", suf, mp, 0, 0, 0, 0, *none, 0, 0, 0, 0) == 0
    assert loop(B_=0) == 0 and loop(nsteps=0) == 0 and lib._dll.se3mpc_smoother_reset(0, None, 0) == 0
    # every rejected call launched nothing
    for now_, then in zip((sm, st, pos), before):
        assert np.array_equal(np.array(h.to_host(now_)).view(np.uint8), then.view(np.uint8))        # (bytes: the controller record holds a NaN)
    assert np.all(h.to_host(tg) == 7.0) and np.all(h.to_host(br) == 7)
    assert bytes(lib.smoother_default_params()) == bytes(SmootherParams.reference_defaults())
    # front-end shape checks
    import pytest
    with pytest.raises(ValueError):
        ops.smoother_desired(mp, dv.d(np.zeros((B, 24))), now, pos, vel, ts, P)
    with pytest.raises(ValueError):
        ops.smoother_update(mp, sm, dv.d(np.zeros(B + 1)), ts, P)
    with pytest.raises(ValueError):
        ops.closed_loop_smoothed(mp, cp, sp, st, sm, now, pos, vel, att, dv.r(np.zeros((B + 1, 3))), ts, P)


def check_dirty_buffers_and_nan_drone(h, B=66, N=6):
    """Outputs are fully written whatever they held; a drone whose state, plan and clock are NaN leaves its neighbours' bits alone.

    Every buffer an entry point writes without reading (the record se3mpc_smoother_reset fills, target, branch and the four logs) is the
    caller's here, handed to the C ABI filled with one byte pattern: 0xFF (a NaN in both float formats, -1 as int32) in one run, 0x7B in the
    next.  An element the kernels leave unwritten keeps its pattern and so differs between the two runs."""
    rng = np.random.default_rng(21)
    ts, P, V, A, P2, pos, vel, att, om, wind = _loop_inputs(rng, B, N)
    dv, ops, lib = Dev(h), h.ops, h.ops.lib
    ptr, suf, nsteps = ops.be.ptr, "f64" if h.dt == np.float64 else "f32", 8
    cp, sp, mp = lib.controller_default_params(), lib.simulator_default_params(), SmootherParams.reference_defaults()

    def run(poison, byte):
        def dirty(shape, dtype):
            a = np.empty(shape, dtype=dtype)
            a.view(np.uint8)[...] = byte
            return h.to_dev(a)

        p_, v_, P_, P2_ = pos.copy(), vel.copy(), P.copy(), P2.copy()
        t_ = np.full(B, 7.0)
        if poison is not None:
            p_[poison] = v_[poison] = np.nan; P_[poison] = P2_[poison] = np.nan; t_[poison] = np.nan
        st, time = ops.controller_state(cp, B), dv.d(t_)
        dp, dvl, da, do, dw = dv.r(p_), dv.r(v_), dv.r(att), dv.r(om), dv.r(wind)
        pl1, pl2 = (dv.d(ts), dv.r(P_), dv.r(V), dv.r(A)), (dv.d(ts), dv.r(P2_), dv.r(V), dv.r(A))
        sm = dirty((B, SMOOTHER_STATE_WORDS), np.float64)
        lib.smoother_reset(B, ptr(sm), ops.be.stream())
        ops.smoother_update(mp, sm, time, *pl1)
        ops.smoother_update(mp, sm, time, *pl2, old=pl1)
        plan = ops._plan_ptrs(B, suf, *pl2, None)
        tg, br = dirty((B, 9), h.dt), dirty((B,), np.int32)
        lib.loop_call("smoother_desired", suf, mp, B, ptr(time), ptr(dp), ptr(dvl), *plan, ptr(sm), ptr(tg), ptr(br), ops.be.stream())
        ls, lc, lt, lg = dirty((nsteps, B, 12), h.dt), dirty((nsteps, B, 4), h.dt), dirty((nsteps, B), np.float64), dirty((nsteps, B, 9), h.dt)
        lib.loop_call("closed_loop_smoothed", suf, mp, cp, sp, B, nsteps, 0.002, *plan, ptr(time), ptr(dp), ptr(dvl), ptr(da), ptr(do), ptr(st), ptr(sm),
                      ptr(dw), 3, -1, None, ptr(ls), ptr(lc), ptr(lt), ptr(lg), ops.be.stream())
        return [np.array(h.to_host(o)) for o in (tg, br, ls, lc, lt, lg, sm, st, dp, time)]

    clean, again, sick = run(None, 0xFF), run(None, 0x7B), run(17, 0xFF)
    for a, b in zip(clean, again):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))        # nothing kept the bytes it was handed
    for a in (clean[0], clean[2], clean[3], clean[4], clean[5], clean[6]):
        assert np.all(np.isfinite(a))                                        # (0xFF.. is a NaN)
    assert np.all((clean[1] >= 0) & (clean[1] <= 4))
    others = np.arange(B) != 17
    for a, c in zip(clean, sick):
        ax = 0 if a.shape[0] == B else 1
        assert np.array_equal(np.compress(others, a, axis=ax).view(np.uint8), np.compress(others, c, axis=ax).view(np.uint8))
    assert np.all(np.isnan(sick[5][:, 17, 0:3]))
