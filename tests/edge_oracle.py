"""NumPy restatement of the reference's edge loop (edge/main.py:80-95) for B drones at once -- TEST ORACLE of dart_planner_amd/csrc/edge_loop.hip:

* ``pid_update``      PIDController.update                       src/dart_planner/utils/pid_controller.py:25-51
* ``control``         OnboardController.compute_control_command  src/dart_planner/control/onboard_controller.py:95-180 (sense :136-142 with the
                      sampler :43-93, the dt <= 0 command :176-177, plan :144-161 with :95-113, act :163-170 with :115-134) and
                      get_fallback_command (:182-184) with edge/main.py:94's target when there is no plan
* ``push``            LatencyBuffer.push                          src/dart_planner/utils/latency_buffer.py:34-82 (the deque as a ring)
* ``sim_step``        DroneSimulator.step                         src/dart_planner/utils/drone_simulator.py:52-72
* ``edge_loop``       the loop body, ``nsteps`` times

Pinned to the reference's own classes call by call by tests/golden/make_golden_edge.py.  ``dtype`` is the precision every stored value and
every intermediate is rounded to (float64: the reference; float32: what an f32 kernel can be asked for); clocks are float64 always.

Decisions and margins.  The clock decisions (dt <= 0, the sampler's search) are taken on float64 clocks that the kernels form with the same
additions, so they are exact on both sides and have no margin.  The integral clamps (pid.py:37-40) and the thrust clip (onboard.py:101) are
continuous (a value a rounding error away from the threshold gives a result a rounding error away), but WHICH side was taken is what the
coverage counters count, so ``diag['margin']`` reports the smallest relative distance of any of them from its threshold per drone."""
import numpy as np

ONBOARD_WORDS, LATENCY_WORDS = 14, 4
BRANCHES = ("filling", "full", "dt_le_0", "thrust_clipped", "clamp_pos_x", "clamp_pos_y", "clamp_pos_z", "clamp_roll", "clamp_pitch", "clamp_yaw_rate",
            "sample_before", "sample_inside", "sample_behind", "fallback")


def params(**over):
    """OnboardController() (onboard.py:25-35): pid rows pos_x, pos_y, pos_z, roll, pitch, yaw_rate; columns Kp, Ki, Kd, integral_limit."""
    p = dict(mass=1.0, g=9.81, first_dt=0.01,
             pid=np.array([[10.0, 1.0, 5.0, 2.0], [10.0, 1.0, 5.0, 2.0], [12.0, 1.5, 6.0, 2.0], [8.0, 0.0, 2.0, 1.0], [8.0, 0.0, 2.0, 1.0], [4.0, 0.0, 1.0, 0.5]]))
    p.update(over)
    return p


def sim_params(**over):
    p = dict(mass=1.5, gravity=9.81, inertia=np.array([0.1, 0.1, 0.2]), max_thrust=20.0, max_torque=10.0)      # simulator.py:41-50
    p.update(over)
    return p


def onboard_reset(B):
    return np.zeros((B, ONBOARD_WORDS))                              # onboard.py:186-193 (last_time None: word 13 = 0)


def latency_reset(B, depth, dtype=np.float64):
    """-> the buffer of `depth` slots (0: none): ring (depth, 12, B), ring_time (depth, B), state (B, 4) = len, oldest slot, total_samples, actual_delay_s."""
    if depth == 0:
        return dict(depth=0, ring=None, ring_time=None, state=None)
    return dict(depth=depth, ring=np.zeros((depth, 12, B), dtype), ring_time=np.zeros((depth, B)), state=np.zeros((B, LATENCY_WORDS)))


def buffer_size(delay_s, dt, max_buffer_size=1000):
    return min(max(1, int(round(delay_s / dt))), max_buffer_size)   # latency.py:40-41 (Python's round: half to even)


def push(buf, t, x, diag=None):
    """push(state, timestamp = state.timestamp) (latency.py:54-82): t (B,), x (B, 12) = pos, vel, att, omega -> delayed (t, x)."""
    depth, st = buf["depth"], buf["state"]
    B = t.shape[0]
    idx = np.arange(B)
    count, head = st[:, 0].astype(int), st[:, 1].astype(int)
    filling = count < depth                                          # :68
    slot = np.where(filling, (head + count) % depth, head)
    dt_out, x_out = np.where(filling, t, buf["ring_time"][slot, idx]), np.where(filling[:, None], x, buf["ring"][slot, :, idx])   # :73 / :76
    buf["ring"][slot, :, idx] = x                                    # :70 / :77
    buf["ring_time"][slot, idx] = t
    st[:, 3] = np.where(filling, st[:, 3], t - dt_out)               # :81
    st[:, 0] = np.where(filling, count + 1, count)
    st[:, 1] = np.where(filling, head, (head + 1) % depth)
    st[:, 2] += 1.0                                                  # :71 / :78
    if diag is not None:
        diag["filling"] = filling
    return dt_out, x_out.astype(buf["ring"].dtype)


def sample(t, plan, dtype):
    """_interpolate_trajectory (onboard.py:43-93) per drone.  plan = (ts (N,) or (B, N), P, V, A (N, 3) or (B, N, 3); V, A may be None)
    -> tp, tv, ta (B, 3), where (B,) = 0 before the plan, 1 inside, 2 behind."""
    ts, P, V, A = plan
    B = t.shape[0]
    N = ts.shape[-1]
    row = lambda a, b: None if a is None else (a[b] if a.ndim == 3 else a)
    out, where = np.zeros((3, B, 3), dtype), np.zeros(B, int)
    for b in range(B):
        tsb = ts[b] if ts.ndim == 2 else ts
        rows = [row(P, b), row(V, b), row(A, b)]
        # first i with ts[i] >= t.  A NaN clock is where oracle and kernel DEVIATE from the reference: np.searchsorted sorts NaN last (idx = N: the
        # plan's last row), the kernel's scan `ts[i] < t` is false at once (idx = 0: its first row).  Every output of such a drone is NaN either
        # way (dt is NaN), and only the NaN-drone test, which compares the neighbours alone, gets here.
        idx = int(np.searchsorted(tsb, t[b])) if t[b] == t[b] else 0
        if idx == 0 or idx >= N:                                     # :52-75
            i = 0 if idx == 0 else N - 1
            where[b] = 0 if idx == 0 else 2
            for k in range(3):
                out[k, b] = 0.0 if rows[k] is None else rows[k][i].astype(dtype)
            continue
        where[b] = 1
        f = dtype((t[b] - tsb[idx - 1]) / (tsb[idx] - tsb[idx - 1]))  # :80 (double clock arithmetic, then the kernel's precision)
        for k in range(3):
            if rows[k] is not None:
                r1, r2 = rows[k][idx - 1].astype(dtype), rows[k][idx].astype(dtype)
                out[k, b] = r1 + f * (r2 - r1)                       # :81-91
    return out[0], out[1], out[2], where


def pid_update(prm, st, i, setpoint, measured, dt, dtype, diag):
    """PIDController.update (pid.py:25-51) of PID row i for the drones in diag['live'] (the others keep their record)."""
    live = diag["live"]
    kp, ki, kd, lim = (dtype(v) for v in prm["pid"][i])
    error = setpoint - measured                                      # :30
    P_out = kp * error                                               # :33
    I = st[:, i].astype(dtype) + error * dt                          # :36
    if lim != 0:                                                     # :37
        with np.errstate(invalid="ignore"):
            diag["margin"] = np.where(live, np.minimum(diag["margin"], np.abs(np.abs(I.astype(float)) - float(lim)) / abs(float(lim))), diag["margin"])
            diag["hits"][:, 4 + i] = live & (np.abs(I) > abs(lim))
        I = np.minimum(np.maximum(I, -lim), lim)                     # :38-40 np.clip
    I_out = ki * I                                                   # :41
    with np.errstate(divide="ignore", invalid="ignore"):
        derivative = (error - st[:, 6 + i].astype(dtype)) / dt       # :44
    D_out = kd * derivative                                          # :45
    out = (P_out + I_out) + D_out                                    # :48
    st[:, i] = np.where(live, I, st[:, i])
    st[:, 6 + i] = np.where(live, error, st[:, 6 + i])               # :50
    return out.astype(dtype)


def control(prm, st, t, pos, att, omega, plan, dtype=np.float64, diag=None):
    """compute_control_command for B drones (plan = None: the fallback, record untouched) -> thrust (B,), torque (B, 3), target (B, 3)."""
    B = t.shape[0]
    d = diag if diag is not None else {}
    d.setdefault("margin", np.full(B, np.inf))
    d["hits"] = np.zeros((B, len(BRANCHES)), bool)
    pos, att, omega = (np.asarray(a).astype(dtype) for a in (pos, att, omega))
    if plan is None:                                                 # onboard.py:182-184, edge/main.py:91-94
        d["hits"][:, 13] = True
        return np.full(B, dtype(prm["mass"] * prm["g"])), np.zeros((B, 3), dtype), pos.copy()
    has = st[:, 13] != 0
    with np.errstate(invalid="ignore"):
        dt_d = np.where(has, t - st[:, 12], prm["first_dt"])         # :139
        st[:, 12], st[:, 13] = t, 1.0                                # :140
        tp, tv, ta, where = sample(t, plan, dtype)                   # :141
        stale = dt_d <= 0                                            # :176
    live = ~stale
    d["live"] = live
    d["hits"][:, 2] = stale
    for k in range(3):
        d["hits"][:, 10 + k] = where == k
    dt = np.where(live, dt_d, 1.0).astype(dtype)
    mass, g = dtype(prm["mass"]), dtype(prm["g"])
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.stack([ta[:, i] + pid_update(prm, st, i, tp[:, i], pos[:, i], dt, dtype, d) for i in range(3)], axis=1)   # :147-157
        raw = mass * (acc[:, 2] + g)                                 # :100
        d["margin"] = np.where(live, np.minimum(d["margin"], np.abs(raw.astype(float)) / (float(mass) * np.maximum(np.abs(acc[:, 2].astype(float)), float(g)))), d["margin"])
        d["hits"][:, 3] = live & ~(raw > 0)
        thrust = np.where(raw > 0, raw, dtype(0))                    # :101 max(0.0, thrust)
        sy, cy = np.sin(att[:, 2]), np.cos(att[:, 2])
        inv_g = dtype(1) / g
        roll = inv_g * (acc[:, 0] * sy - acc[:, 1] * cy)             # :104-107
        pitch = inv_g * (acc[:, 0] * cy + acc[:, 1] * sy)            # :108-111
        tq = np.stack([pid_update(prm, st, 3, roll, att[:, 0], dt, dtype, d), pid_update(prm, st, 4, pitch, att[:, 1], dt, dtype, d),
                       pid_update(prm, st, 5, np.zeros(B, dtype), omega[:, 2], dt, dtype, d)], axis=1)    # :125-132
    z = dtype(0)
    return (np.where(live, thrust, z).astype(dtype), np.where(live[:, None], tq, z).astype(dtype), np.where(live[:, None], tp, z).astype(dtype))


def sim_step(sp, t, x, thrust, torque, dt_d, wind, dtype=np.float64):
    """DroneSimulator.step (simulator.py:52-72) on x (B, 12) = pos, vel, att, omega -> (t, x)."""
    x = x.astype(dtype).copy()
    dt = dtype(dt_d)
    mass, grav = dtype(sp["mass"]), dtype(sp["gravity"])
    with np.errstate(invalid="ignore"):
        th = np.fmin(np.fmax(thrust.astype(dtype), dtype(0)), dtype(sp["max_thrust"]))          # :54
        tq = np.fmin(np.fmax(torque.astype(dtype), dtype(-sp["max_torque"])), dtype(sp["max_torque"]))   # :55
    for i in range(3):
        wa = wind[:, i].astype(dtype) / mass                         # :57
        acc = ((-grav if i == 2 else dtype(0)) + (th / mass if i == 2 else dtype(0))) + wa       # :59
        x[:, 3 + i] = x[:, 3 + i] + acc * dt                         # :60
        x[:, i] = x[:, i] + x[:, 3 + i] * dt                         # :61
        x[:, 9 + i] = x[:, 9 + i] + (tq[:, i] / dtype(sp["inertia"][i])) * dt                    # :63-64
        x[:, 6 + i] = x[:, 6 + i] + x[:, 9 + i] * dt                 # :65
    return t + dt_d, x


def edge_loop(prm, sp, st, buf, t, x, plan, nsteps, sim_dt, wind=None, dtype=np.float64, margin=1e-6):
    """nsteps x (push -> control or fallback -> DroneSimulator.step) (edge/main.py:80-95).  st, buf, t, x are updated in place.
    -> dict(state (nsteps, B, 12) and time (nsteps, B) BEFORE each step, cmd (nsteps, B, 4), target (nsteps, B, 3), delayed_time (nsteps, B),
    hits (nsteps, B, len(BRANCHES)), near (nsteps, B): a decision of this or an earlier step lay within `margin` of its threshold)."""
    B = t.shape[0]
    wind = np.zeros((B, 3)) if wind is None else np.broadcast_to(np.asarray(wind, float), (B, 3))
    log = {k: [] for k in ("state", "time", "cmd", "target", "delayed_time", "hits", "near")}
    near = np.zeros(B, bool)
    x[...] = x.astype(dtype)
    for _ in range(nsteps):
        log["state"].append(x.astype(float).copy()); log["time"].append(t.copy())
        d = {}
        if buf["depth"] > 0:
            dl_t, dl_x = push(buf, t, x.astype(dtype), diag=d)
        else:
            dl_t, dl_x, d["filling"] = t.copy(), x.astype(dtype), None
        th, tq, tg = control(prm, st, dl_t, dl_x[:, 0:3], dl_x[:, 6:9], dl_x[:, 9:12], plan, dtype, d)
        if d["filling"] is not None:
            d["hits"][:, 0], d["hits"][:, 1] = d["filling"], ~d["filling"]
        near = near | ~(d["margin"] >= margin)
        t_new, x_new = sim_step(sp, t, x, th, tq, sim_dt, wind, dtype)
        t[...], x[...] = t_new, x_new
        for k, v in (("cmd", np.concatenate([th[:, None], tq], axis=1).astype(float)), ("target", tg.astype(float)), ("delayed_time", dl_t.copy()),
                     ("hits", d["hits"].copy()), ("near", near.copy())):
            log[k].append(v)
    return {k: np.array(v) for k, v in log.items()}
