"""Batched NumPy restatement of the reference's TrajectorySmoother ("smoother.py" = src/dart_planner/control/trajectory_smoother.py), the
oracle of dart_planner_amd/csrc/smoother.hip.  Lives under tests/ because oracle/ is frozen (as tests/mppi_oracle.py).  Pinned to vectors
of the reference's own class by tests/test_smoother_oracle_golden.py.

One drone per row.  Clocks are float64 whatever `dtype` says; per-axis arithmetic is done in `dtype` (float64 by default; float32 gives the
rounding-order yardstick of the float32 kernels).  State: (B, 25) float64 records laid out as SE3MPC_SMOOTHER_STATE_WORDS in
include/se3mpc.h.  A plan is (ts, P, V, A): ts (N,) or (B, N) float64, P / V / A (N, 3) or (B, N, 3) (V, A may be None), N >= 0.

`diag`, when a dict is passed, collects what the golden generator and the random tests assert about a call: "margin" (B,) = the smallest
relative distance of any discontinuous decision (transition thresholds, progress >= 1, timeout, knot comparisons that are not exact
ties) from its threshold, and "clamps" (B, 5) booleans = (transition velocity norm, transition acceleration norm, per-call velocity,
per-call acceleration, per-call jerk) clamp fired."""
import numpy as np

STATE_WORDS = 25
HAS_TRAJECTORY, IN_TRANSITION = 1, 2
FAILSAFE, TRANSITION, TRANSITION_DONE, NORMAL, NO_TRAJECTORY = 0, 1, 2, 3, 4
CLAMPS = ("transition_velocity", "transition_acceleration", "velocity_change", "acceleration_change", "jerk")

DEFAULTS = dict(transition_time=0.5, velocity_limit=5.0, acceleration_limit=3.0, jerk_limit=10.0, update_dt=0.01, smoothing_window=0.1,
                pos_diff_threshold=0.5, vel_diff_threshold=1.0, timeout=2.0, decay_rate=2.0, decay_cap=5.0)


def params(**overrides):
    p = dict(DEFAULTS)
    for k, v in overrides.items():
        if k not in p:
            raise KeyError(k)
        p[k] = float(v)
    return p


def reset(B):
    return np.zeros((B, STATE_WORDS))                                            # smoother.py:28-46


def _rel(a, b):
    """Relative distance of a from the threshold b."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


def _norm(x):
    return np.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])


def _note(diag, key, B, value):
    if diag is None:
        return
    if key == "margin":
        diag["margin"] = np.minimum(diag.get("margin", np.full(B, np.inf)), value)
    else:
        diag[key] = value


def sample(tt, plan, B, dtype=np.float64, diag=None, active=None):
    """_interpolate_trajectory (smoother.py:215-278) at trajectory_time tt (B,) -> (B, 9)."""
    R = dtype
    if plan is None:
        return np.zeros((B, 9), R)
    ts, P, V, A = plan
    ts = np.asarray(ts, float)
    N = ts.shape[-1]
    if N == 0:                                                                    # :221-222
        return np.zeros((B, 9), R)
    ts = np.broadcast_to(ts, (B, N))
    rows = np.zeros((B, N, 9), R)
    for j, X in enumerate((P, V, A)):
        if X is not None:                                                         # :233, :238 missing velocities / accelerations are zeros
            rows[:, :, 3 * j:3 * j + 3] = np.broadcast_to(np.asarray(X, R), (B, N, 3))
    rel = ts - ts[:, :1]                                                          # :225
    idx = np.sum(rel < tt[:, None], axis=1)                                       # np.searchsorted(rel, tt)
    first = tt <= rel[:, 0]                                                       # :228
    last = ~first & (tt >= rel[:, -1])                                            # :241
    i1 = np.clip(idx - 1, 0, N - 1)                                               # :256
    i2 = np.clip(idx, 0, N - 1)
    ar = np.arange(B)
    t1, t2 = rel[ar, i1], rel[ar, i2]
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = ((tt - t1) / (t2 - t1)).astype(R)                                 # :257-258
    r1, r2 = rows[ar, i1], rows[ar, i2]
    with np.errstate(invalid="ignore"):
        out = (R(1) - alpha)[:, None] * r1 + alpha[:, None] * r2                  # :260-276
    out = np.where(first[:, None], rows[:, 0], np.where(last[:, None], rows[:, -1], out))
    if diag is not None:
        m = _rel(tt[:, None], rel)
        m = np.where(tt[:, None] == rel, np.inf, m)                               # an exact tie is a placement on purpose
        m = m.min(axis=1)
        if active is not None:
            m = np.where(active, m, np.inf)
        _note(diag, "margin", B, m)
    return out.astype(R)


def _smooth(prm, state, x, mask, dtype, diag):
    """_apply_trajectory_limits (:64-92) + the filter of _smooth_trajectory_point (:94-113) for the rows in `mask`; -> x, state updated."""
    R = dtype
    f = state[:, :9].astype(R)
    dt = R(prm["update_dt"])
    vel_step, acc_step = R(prm["velocity_limit"] * prm["update_dt"]), R(prm["acceleration_limit"] * prm["update_dt"])
    x = x.copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ch = x[:, 3:6] - f[:, 3:6]                                                # :68
        mag = _norm(ch)                                                           # :69
        cv = mag > vel_step                                                       # :71
        x[:, 3:6] = np.where(cv[:, None], f[:, 3:6] + (ch * vel_step) / mag[:, None], x[:, 3:6])   # :72-73
        ch = x[:, 6:9] - f[:, 6:9]                                                # :76
        mag = _norm(ch)
        ca = mag > acc_step                                                       # :79
        x[:, 6:9] = np.where(ca[:, None], f[:, 6:9] + (ch * acc_step) / mag[:, None], x[:, 6:9])   # :80-81
        jerk = (x[:, 6:9] - f[:, 6:9]) / dt                                       # :85
        jm = _norm(jerk)
        cj = jm > R(prm["jerk_limit"])                                            # :88
        x[:, 6:9] = np.where(cj[:, None], f[:, 6:9] + ((jerk * R(prm["jerk_limit"])) / jm[:, None]) * dt, x[:, 6:9])   # :89-90
        alpha = min(1.0, prm["update_dt"] / prm["smoothing_window"])              # :101
        filt = _norm(f[:, :3]) > 0                                                # :103
        x = np.where(filt[:, None], R(alpha) * x + R(1.0 - alpha) * f, x)         # :104-106
    state[mask, :9] = x[mask].astype(float)                                       # :109-111
    if diag is not None:
        cl = diag.setdefault("clamps", np.zeros((len(x), 5), bool))
        cl[:, 2] |= cv & mask; cl[:, 3] |= ca & mask; cl[:, 4] |= cj & mask
    return x


def _transition(prm, state, progress, dtype, diag, mask):
    """_generate_transition_state (:280-319) -> (B, 9)."""
    R = dtype
    t = np.clip(progress, 0.0, 1.0).astype(R)                                     # :285
    t2 = t * t; t3 = t2 * t; t4 = t3 * t; t5 = t4 * t
    s = ((R(10) * t3 - R(15) * t4) + R(6) * t5)[:, None]                          # :288
    sd = (((R(30) * t2 - R(60) * t3) + R(30) * t4) / R(prm["transition_time"]))[:, None]          # :289-291
    sdd = (((R(60) * t - R(180) * t2) + R(120) * t3) / R(prm["transition_time"] * prm["transition_time"]))[:, None]   # :292-294
    tr = state[:, 9:21].astype(R)
    sp, sv, tp, tv = tr[:, 0:3], tr[:, 3:6], tr[:, 6:9], tr[:, 9:12]
    pd = tp - sp                                                                  # :300
    pos = (R(1) - s) * sp + s * tp                                                # :297
    vel = ((R(1) - s) * sv + s * tv) + sd * pd                                    # :301-305
    acc = sdd * pd                                                                # :308
    with np.errstate(invalid="ignore", divide="ignore"):
        vn = _norm(vel)
        cv = vn > R(prm["velocity_limit"])                                        # :312
        vel = np.where(cv[:, None], vel * (R(prm["velocity_limit"]) / vn)[:, None], vel)
        an = _norm(acc)
        ca = an > R(prm["acceleration_limit"])                                    # :316
        acc = np.where(ca[:, None], acc * (R(prm["acceleration_limit"]) / an)[:, None], acc)
    if diag is not None:
        cl = diag.setdefault("clamps", np.zeros((len(t), 5), bool))
        cl[:, 0] |= cv & mask; cl[:, 1] |= ca & mask
    return np.concatenate([pos, vel, acc], axis=1).astype(R)


def update(prm, state, now, old_plan, new_plan, dtype=np.float64, diag=None):
    """update_trajectory (:115-165) at the clocks now (B,); `state` is updated in place."""
    R = dtype
    B = state.shape[0]
    now = np.asarray(now, float)
    bits = state[:, 24].astype(int)
    had = (bits & HAS_TRAJECTORY) != 0
    state[:, 22] = now                                                            # :123
    cur = sample(now - state[:, 23], old_plan, B, R, diag, active=had)            # :134-140
    new = sample(now - now, new_plan, B, R)                                       # :143-145
    pos_diff, vel_diff = _norm(new[:, 0:3] - cur[:, 0:3]), _norm(new[:, 3:6] - cur[:, 3:6])   # :148-149
    with np.errstate(invalid="ignore"):
        start = had & ((pos_diff > R(prm["pos_diff_threshold"])) | (vel_diff > R(prm["vel_diff_threshold"])))   # :151
    if diag is not None:
        m = np.minimum(_rel(pos_diff, prm["pos_diff_threshold"]), _rel(vel_diff, prm["vel_diff_threshold"]))
        _note(diag, "margin", B, np.where(had, m, np.inf))
        diag["pos_diff"], diag["vel_diff"], diag["started"] = np.where(had, pos_diff, np.nan), np.where(had, vel_diff, np.nan), start
    bits = np.where(had, bits, HAS_TRAJECTORY)                                    # :125-131 (in_transition = False)
    bits = np.where(start, bits | IN_TRANSITION, bits)                            # :153
    state[start, 21] = now[start]                                                 # :154
    state[start, 9:15] = cur[start, 0:6].astype(float)                            # :155-156
    state[start, 15:21] = new[start, 0:6].astype(float)                           # :157-158
    state[:, 23] = now                                                            # :128 / :165
    state[:, 24] = bits


def desired(prm, state, now, pos, vel, plan, dtype=np.float64, diag=None):
    """get_desired_state (:167-213) at the clocks now (B,) for drones at (pos, vel) (B, 3) -> target (B, 9), branch (B,) int32."""
    R = dtype
    B = state.shape[0]
    now = np.asarray(now, float)
    pos, vel = np.asarray(pos, R), np.asarray(vel, R)
    bits = state[:, 24].astype(int)
    age = now - state[:, 22]
    with np.errstate(invalid="ignore", over="ignore"):
        failsafe = age > prm["timeout"]                                           # :176
        decay = np.exp(-prm["decay_rate"] * np.minimum(age - prm["timeout"], prm["decay_cap"])).astype(R)   # :330-332
        fv = vel * decay[:, None]                                                 # :333
        fs = np.concatenate([pos, fv, R(-prm["decay_rate"]) * fv], axis=1)        # :326, :336
        in_tr = ~failsafe & ((bits & IN_TRANSITION) != 0)                         # :182
        progress = (now - state[:, 21]) / prm["transition_time"]                  # :183-185
        done = in_tr & (progress >= 1.0)                                          # :187
    point = in_tr & ~done
    bits = np.where(done, bits & ~IN_TRANSITION, bits)                            # :189
    has = (bits & HAS_TRAJECTORY) != 0
    follow = ~failsafe & ~point & has                                             # :201
    nothing = ~failsafe & ~point & ~has                                           # :213
    if diag is not None:
        _note(diag, "margin", B, _rel(age, prm["timeout"]))
        _note(diag, "margin", B, np.where(in_tr, _rel(progress, 1.0), np.inf))
    x = np.where(point[:, None], _transition(prm, state, progress, R, diag, point),
                 sample(now - state[:, 23], plan, B, R, diag, active=follow))     # :192 / :202-204
    smoothed = _smooth(prm, state, x, point | follow, R, diag)                    # :195 / :207
    hover = np.concatenate([pos, np.zeros((B, 6), R)], axis=1)
    out = np.where(failsafe[:, None], fs, np.where(nothing[:, None], hover, smoothed)).astype(R)
    state[:, 24] = bits
    branch = np.where(failsafe, FAILSAFE, np.where(point, TRANSITION, np.where(nothing, NO_TRAJECTORY, np.where(done, TRANSITION_DONE, NORMAL))))
    return out, branch.astype(np.int32)
