"""Checks of MPPI around moving spheres (se3mpc_mppi_moving_*, se3mpc_mppi_closed_loop_moving_*, Ops.mppi / Ops.mppi_closed_loop with
sphere_vel, SE3MPCPlanner.add_moving_obstacle, ClosedLoopMonteCarlo.run_mppi / run_mppi_fused with sphere_velocities) shared by the
host-emulation suite (tests/test_emu_mppi_moving.py) and the MI355X suite (tests/test_gpu_mppi_moving.py).  Every check takes a
parity_checks.Harness whose arrays are torch tensors.

Bounds: none new.  Against the float64 oracle (tests/mppi_moving_oracle.py) U, cost and trace are held to the bounds of
tests/mppi_checks.py; the clearance to 1e-12 (f64) / 1e-5 m (f32), the rounding of one sqrt and one multiply-add at metre scale; everything
else is bit for bit."""
import numpy as np

import mppi_checks as mc
import mppi_closed_loop_checks as lc
import mppi_moving_oracle as mvo
import mppi_oracle as mo
from dart_planner_amd.capi import ControllerParams, Params, SimulatorParams
from oracle import controller_oracle as co
from oracle import se3mpc_oracle as orc

CLEARANCE_ABS = {np.float64: 1e-12, np.float32: 1e-5}
T0 = 1.3                              # seconds between the table's time and the plan's start in the oracle checks


def velocities(K, seed, lo=0.5, hi=3.0):
    """K velocities of speed in [lo, hi] m/s, random directions."""
    rng = np.random.default_rng(seed + 77)
    d = rng.normal(0, 1, (K, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True) if K else 1.0
    return d * rng.uniform(lo, hi, (K, 1))


def _round(h, a):
    return np.asarray(a, float).astype(h.dt).astype(float)


class Run(mc.Run):
    """mppi_checks.Run on the moving entry: the velocity table and sphere_t0 ride along."""

    def __init__(self, h, prm, p0, v0, goal, U, sph, vel, w_obs=0.0, t0=0.0):
        super().__init__(h, prm, p0, v0, goal, U, sph, w_obs)
        self.vel = h.to_dev(np.ascontiguousarray(np.asarray(vel, float).reshape(-1, 3).astype(h.dt)))
        self.t0 = t0

    def __call__(self, S, iters, sigma, lam, t0=None, **kw):
        return super().__call__(S, iters, sigma, lam, sphere_vel=self.vel, sphere_t0=self.t0 if t0 is None else t0, **kw)


class Scene(lc.Scene):
    """mppi_closed_loop_checks.Scene with a velocity table; call(..., moving=False) takes the static entry."""

    def __init__(self, h, N, B, K=0, vel=None, t0=0.0, **kw):
        super().__init__(h, N, B, K=K, **kw)
        self.vel = _round(h, np.zeros((self.K, 3)) if vel is None else np.asarray(vel, float).reshape(-1, 3))
        self.vel_d = self.d(self.vel)
        self.t0 = t0

    def call(self, st, *a, moving=True, **kw):
        if moving:
            kw.setdefault("sphere_vel", self.vel_d)
            kw.setdefault("sphere_t0", self.t0)
        return super().call(st, *a, **kw)


def _same_outputs(a, b, what, keys=("U", "cost", "trace", "keys")):
    for k in keys:
        assert lc.bits_equal(a[k], b[k]), f"{what}: {k}"


# ---- 1. zero velocity is the static kernel ---------------------------------------------------------------------------------------------
def check_zero_velocity_planner(h, N, S, nprob, K, iters=2, seed=5, sigma=1.0, w_obs=40.0):
    """se3mpc_mppi_moving_* with sphere_vel = 0 at sphere_t0 = 0 and 3.7: U, cost, trace and keys of se3mpc_mppi_*, bit for bit."""
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, nprob, seed, K=K)
    static = mc.Run(h, prm, p0, v0, goal, U, sph, w_obs)
    ref = static(S, iters, sigma, 50.0, seed=seed, iter_base=2, index_base=3)
    mov = Run(h, prm, p0, v0, goal, U, sph, np.zeros((K, 3)), w_obs)
    for t0 in (0.0, 3.7):
        _same_outputs(mov(S, iters, sigma, 50.0, t0=t0, seed=seed, iter_base=2, index_base=3), ref, f"zero velocity, sphere_t0 = {t0}")
    if K >= 3 and N > 1:
        pen = orc.obstacle_penalty_grad(_round(h, p0)[:, None], _round(h, v0)[:, None], _round(h, U)[:, None], _round(h, sph), cfg, w_obs)[0]
        assert np.any(pen > 0), "the check wants nominals inside the spheres' margins"


def check_zero_velocity_closed_loop(h, N, B, K, S=64, cycles=2, substeps=3, sim_dt=0.01, shift=1, seed=5):
    """se3mpc_mppi_closed_loop_moving_* with sphere_vel = 0: state, U, cost, trace, plan_last and clearance of se3mpc_mppi_closed_loop_*."""
    for t0 in (0.0, 3.7):
        sc = Scene(h, N, B, K=K, S=S, seed=seed, t0=t0)
        a, b = sc.fresh(), sc.fresh()
        oa = sc.call(a, cycles, substeps, sim_dt, shift, iter_base=7, moving=False)
        ob = sc.call(b, cycles, substeps, sim_dt, shift, iter_base=7)
        lc.same_bits(a, b, f"zero velocity, sphere_t0 = {t0}")
        _same_outputs(oa, ob, f"zero velocity, sphere_t0 = {t0}", ("cost", "trace", "plan_last"))


# ---- 2. against the oracle -------------------------------------------------------------------------------------------------------------
def crossing_problem(h, N, nprob, K, seed, t0=T0, params=None):
    """mppi_checks.problem with velocities up to 3 m/s, sphere 0 (r = 0.5 m) aimed so that it covers problem 0's nominal at its last step
    and is far from it at the table's time."""
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, nprob, seed, K=K, params=params)
    p0, v0, goal, U = (_round(h, a) for a in (p0, v0, goal, U))
    vel = velocities(K, seed)
    if K and N > 1:
        P, _ = orc.rollout(p0[0], v0[0], U[0], cfg)
        k = N - 1
        tau = t0 + k * cfg.dt
        vel[0] *= 2.5 / np.linalg.norm(vel[0])
        sph[0, 3] = 0.5
        sph[0, :3] = P[k] + [0.1, -0.05, 0.08] - vel[0] * tau
    return prm, cfg, p0, v0, goal, U, _round(h, sph), _round(h, vel)


def check_against_oracle(h, N, S, nprob, iters, K, seed=5, sigma=1.0, w_obs=40.0, t0=T0, params=None):
    """U, cost, trace of se3mpc_mppi_moving_* against the float64 oracle, velocities up to 3 m/s (iters = 0 included)."""
    prm, cfg, p0, v0, goal, U, sph, vel = crossing_problem(h, N, nprob, K, seed, t0, params=params)
    tR = mvo.step_times(N, cfg.dt, t0, h.dt)
    if K and N > 1:
        P, _ = orc.rollout(p0[0], v0[0], U[0], cfg)
        moving_c = mvo.residuals(P, sph, vel, tR, cfg)
        static_c = mvo.residuals(P, sph, np.zeros_like(vel), tR, cfg)
        assert moving_c[N - 1, 0] < 0 < static_c[N - 1, 0], "sphere 0 covers the nominal at step N - 1 and not at the table's time"
        assert mvo.penalty(p0[0], v0[0], U[0], sph, vel, tR, cfg, w_obs) != mvo.penalty(p0[0], v0[0], U[0], sph, 0 * vel, tR, cfg, w_obs)
    run = Run(h, prm, p0, v0, goal, U, sph, vel, w_obs, t0)
    T, _, _ = mo.samples(U[0], 0, 0, S, sigma, seed, cfg)
    c = mvo.cost(p0[0], v0[0], goal[0], T, cfg, sph, vel, tR, w_obs)
    lam = float(np.median(c) - np.min(c))
    for it in (iters, 0):
        Ud, cd, trd, keys = run.host(run(S, it, sigma, lam, seed=seed, iter_base=2, index_base=0))
        for p in range(nprob):
            Ur, cr, trr = mvo.mppi(p0[p], v0[p], goal[p], U[p], p, S, it, sigma, lam, seed, cfg, iter_base=2, spheres=sph, vel=vel, sphere_t0=t0,
                                   obstacle_weight=w_obs, dtype=h.dt)
            if h.dt == np.float32:
                errU = np.max(np.abs(Ud[p] - Ur))
                c_at = mvo.cost(p0[p], v0[p], goal[p], Ud[p], cfg, sph, vel, tR, w_obs)          # the cost of the nominal the kernel returned
                print(f"problem {p}: U err {errU:.3e}, cost rel {abs(cd[p] - c_at) / abs(c_at):.3e}")
                assert errU <= mc.F32_U_ABS, f"U of problem {p}: {errU}"
                assert abs(cd[p] - c_at) <= mc.F32_COST_REL * abs(c_at), f"cost of problem {p}"
                assert np.all(np.abs(trd[:it, p] - trr) <= mc.F32_TRACE_REL * np.abs(trr)), f"trace of problem {p}: {trd[:it, p]} vs {trr}"
            else:
                assert np.max(np.abs(Ud[p] - Ur)) <= mc.F64_REL * 25, f"U of problem {p}: {np.max(np.abs(Ud[p] - Ur))}"
                assert abs(cd[p] - cr) <= mc.F64_REL * abs(cr), f"cost of problem {p}"
                assert np.all(np.abs(trd[:it, p] - trr) <= mc.F64_REL * np.abs(trr)), f"trace of problem {p}"
            k = int(keys[p]) & 0xFFFFFFFFFFFFFFFF
            assert h.ops.lib.key_index(k) == p and h.ops.lib.key_cost(k) == np.float32(cd[p]), "key = orderable(cost) << 32 | q"
        if it == 0:
            assert np.array_equal(Ud, U), "iters = 0 copies U_in"


# ---- 3. iterations in one call, slices -------------------------------------------------------------------------------------------------
def check_chunking_and_slices(h, N, S, nprob, K, iters=3, seed=13, sigma=1.0, t0=T0):
    """mppi_checks.check_chunking_and_slices for the moving entry: iters = n in one call == n calls with iter_base stepping; problems [lo, hi)
    with index_base = lo == that slice of the batch; a second launch == the first (all bit for bit)."""
    prm, cfg, p0, v0, goal, U, sph, vel = crossing_problem(h, N, nprob, K, seed, t0)
    run = Run(h, prm, p0, v0, goal, U, sph, vel, 40.0, t0)
    lam = 50.0
    full_o = run(S, iters, sigma, lam, seed=seed, iter_base=100)
    _same_outputs(run(S, iters, sigma, lam, seed=seed, iter_base=100), full_o, "run-to-run identity")
    full = run.host(full_o)
    Ucur = run.U
    for i in range(iters):
        o = run(S, 1, sigma, lam, seed=seed, iter_base=100 + i, U=Ucur)
        Ucur = o["U"]
        step = run.host(o)
        assert np.array_equal(step[2][0], full[2][i]), f"trace row {i} from one-iteration calls"
    assert np.array_equal(step[0], full[0]) and np.array_equal(step[1], full[1]), "iters = n == n calls"
    lo, hi = 1, nprob - 1
    sub = Run(h, prm, p0[lo:hi], v0[lo:hi], goal[lo:hi], U[lo:hi], sph, vel, 40.0, t0)
    part = sub.host(sub(S, iters, sigma, lam, seed=seed, iter_base=100, index_base=lo))
    assert np.array_equal(part[0], full[0][lo:hi]) and np.array_equal(part[1], full[1][lo:hi]), "slice [lo, hi) == the batch's"
    assert np.array_equal(part[2], full[2][:, lo:hi]) and np.array_equal(part[3], full[3][lo:hi]), "slice trace / keys"


# ---- 4. cycles in one call -------------------------------------------------------------------------------------------------------------
def check_cycle_equivalence(h, N, B, K, S=64, cycles=3, substeps=3, sim_dt=0.01, shift=1, wind="per_drone", seed=5, t0=T0, **scene_kw):
    """cycles = C in one call == C chained calls with cycle_base = 0 .. C - 1, bit for bit, on what
    mppi_closed_loop_checks.check_cycle_equivalence compares: the tau bookkeeping of plan and clearance across launches."""
    import torch
    sc = Scene(h, N, B, K=K, S=S, wind=wind, seed=seed, vel=velocities(K, seed), t0=t0, **scene_kw)
    one = sc.fresh()
    o1 = sc.call(one, cycles, substeps, sim_dt, shift, iter_base=7)
    many = sc.fresh()
    for c in range(cycles):
        oc = sc.call(many, 1, substeps, sim_dt, shift, cycle_base=c, iter_base=7)
        assert lc.bits_equal(oc["trace"][:, 0], o1["trace"][:, c]), f"trace of cycle {c}"
    lc.same_bits(one, many, "cycles = C vs C calls")
    assert lc.bits_equal(o1["cost"], oc["cost"]) and lc.bits_equal(o1["plan_last"], oc["plan_last"]), "last cost / plan"
    assert torch.isfinite(one["pos"]).all() and float((one["pos"] - sc.d(sc.p0)).abs().max()) > 0
    if K:
        assert torch.isfinite(one["clearance"]).all()
        still = sc.fresh()
        sc.call(still, cycles, substeps, sim_dt, shift, iter_base=7, moving=False)
        assert not lc.bits_equal(still["clearance"], one["clearance"]), "the moving table must change the clearance"
    lo, hi = 1, B - 1
    part = sc.fresh(lo, hi)
    op = sc.call(part, cycles, substeps, sim_dt, shift, lo=lo, hi=hi, iter_base=7)
    for k in lc.STATE_KEYS + (("clearance",) if K else ()):
        assert lc.bits_equal(part[k], one[k][lo:hi]), f"slice [lo, hi): {k}"
    assert lc.bits_equal(op["cost"], o1["cost"][lo:hi]) and lc.bits_equal(op["trace"], o1["trace"][lo:hi])


# ---- 5. the planner inside -------------------------------------------------------------------------------------------------------------
def check_planner_inside(h, N, B, K, S=64, run_substeps=4, sim_dt=0.01, seed=6, t0=T0, **scene_kw):
    """For C in {0, 2}: (a) cycles = 1, substeps = 0, shift = 0 at cycle_base = C == se3mpc_mppi_moving_* at the same sphere_t0 (with no
    simulator steps the cycle's base time is 0) and iteration numbers; (b) the same cycle of a run with `run_substeps` steps per cycle and
    sphere_t0 = 0 == se3mpc_mppi_moving_* called with (double)(C * run_substeps) * sim_dt -- U, cost and trace bit for bit."""
    sc = Scene(h, N, B, K=K, S=S, seed=seed, vel=velocities(K, seed), t0=t0, **scene_kw)
    run = Run(h, sc.prm, sc.p0, sc.v0, sc.goal, sc.U0, sc.sph if K else None, sc.vel, sc.w_obs, t0)
    for C in (0, 2):
        for substeps, t_loop, t_plan in ((0, t0, t0), (run_substeps, 0.0, float(C * run_substeps) * sim_dt)):
            st = sc.fresh()
            out = sc.call(st, 1, substeps, sim_dt, 0, cycle_base=C, iter_base=11, sphere_t0=t_loop)
            ref = run(S, sc.iters, sc.sigma, sc.lam, t0=t_plan, seed=sc.seed, iter_base=11 + C * sc.iters)
            what = f"cycle_base {C}, substeps {substeps}"
            assert lc.bits_equal(st["U"], ref["U"].T.reshape(B, N, 3).contiguous()), f"{what}: U == se3mpc_mppi_moving_*"
            assert lc.bits_equal(out["cost"], ref["cost"]), f"{what}: cost == se3mpc_mppi_moving_*"
            assert lc.bits_equal(out["trace"][:, 0].T.contiguous(), ref["trace"]), f"{what}: trace == se3mpc_mppi_moving_*"
    if K >= 3:
        still = mc.Run(h, sc.prm, sc.p0, sc.v0, sc.goal, sc.U0, sc.sph, sc.w_obs)(S, sc.iters, sc.sigma, sc.lam, seed=sc.seed, iter_base=11)
        assert not lc.bits_equal(still["cost"], run(S, sc.iters, sc.sigma, sc.lam, seed=sc.seed, iter_base=11)["cost"]), "the motion must matter"


# ---- 6. clearance ----------------------------------------------------------------------------------------------------------------------
def check_clearance(h, N, B, K, S=64, cycles=6, sim_dt=0.02, seed=8, t0=T0):
    """Chained calls of one cycle of one simulator step: every position comes back, and the oracle's minimum of |pos - centre| - r over them,
    centres at sphere_t0 + (call + 1) * sim_dt, meets `clearance` to 1e-12 (f64) / 1e-5 m (f32); the one-launch run equals the chain bit
    for bit."""
    sc = Scene(h, N, B, K=K, S=S, seed=seed, vel=velocities(K, seed), t0=t0)
    st = sc.fresh()
    visited = []
    for c in range(cycles):
        sc.call(st, 1, 1, sim_dt, 0, cycle_base=c, iter_base=3)
        visited.append(h.to_host(st["pos"]).astype(float).copy())
    tau = t0 + (np.arange(cycles) + 1.0) * sim_dt
    want = mvo.clearance(np.stack(visited), tau, sc.sph, sc.vel, h.dt)
    got = h.to_host(st["clearance"]).astype(float)
    err = float(np.max(np.abs(got - want)))
    print(f"clearance {got} vs oracle {want}: max abs err {err:.3e} (bound {CLEARANCE_ABS[h.dt]:.0e})")
    static = mvo.clearance(np.stack(visited), tau, sc.sph, 0 * sc.vel, h.dt)
    assert np.min(np.abs(static - want)) > 1e-2, "the oracle must tell the moving table from the static one"
    assert err <= CLEARANCE_ABS[h.dt], err
    one = sc.fresh()
    sc.call(one, cycles, 1, sim_dt, 0, iter_base=3)
    lc.same_bits(one, st, "one launch vs the chain")


# ---- 7. behaviour ----------------------------------------------------------------------------------------------------------------------
BEHAVIOUR = dict(S=64, iters=2, sigma=3.0, lam=200.0, cycles=15, substeps=10, sim_dt=0.01, shift=1, w_obs=2000.0)


def behaviour_scene(B=2, N=8):
    """Drones hovering AT their goals, 3 m up (the vertical scene of mppi_closed_loop_checks.behaviour_scene: this simulator's thrust acts
    along world z, so a drone can only dodge up or down).  One sphere of radius 0.6 m flies along y at 2 m/s on a line 0.2 m below the
    goals and passes under them 1.0 s into the 1.5 s run; sphere_t0 = 0, the table holds at the run's start."""
    prm = Params.reference_defaults(horizon=N, dt=0.1, mass=1.0, gravity=9.80665, max_thrust=20.0, max_tilt_angle=0.02)
    off = (np.arange(B) - (B - 1) / 2) * 0.25
    p0 = np.stack([off, np.zeros(B), np.full(B, 3.0)], axis=1)
    return dict(prm=prm, ccfg=co.ControllerConfig(), sim=co.SimulatorConfig(mass=1.0, gravity=9.80665),
                sp=SimulatorParams.reference_defaults(mass=1.0, gravity=9.80665), p0=p0, v0=np.zeros((B, 3)), goal=p0.copy(),
                sph=np.array([[0.0, -2.0, 2.8, 0.6]]), U=np.tile([0.0, 0.0, prm.mass * prm.gravity], (B, N, 1))), np.array([[0.0, 2.0, 0.0]])


def check_behaviour(h, B=2, N=8):
    """One sphere's straight path crosses the hovering drones' goal point during the run.  With obstacle_weight = 0 the run's clearance is
    negative (the sphere went through the drones: the act phase moves it); with the penalty it is positive (the planner saw it coming).
    Both at least 0.2 m from zero on the float64 emulation, so float32 cannot flip either: emulated values (f64, B = 2, N = 8, 15 cycles)
    -0.375 m and -0.379 m without the penalty, +0.931 m and +0.930 m with it."""
    bs, vel = behaviour_scene(B, N)
    kw = BEHAVIOUR
    res = {}
    for w in (0.0, kw["w_obs"]):
        sc = Scene(h, N, B, K=1, S=kw["S"], iters=kw["iters"], sigma=kw["sigma"], lam=kw["lam"], w_obs=w, wind=None, seed=21, vel=vel, t0=0.0, **bs)
        sc.w_obs = w
        st = sc.fresh()
        sc.call(st, kw["cycles"], kw["substeps"], kw["sim_dt"], kw["shift"])
        res[w] = h.to_host(st["clearance"]).astype(float)
        print(f"obstacle_weight {w}: clearance {res[w]}, final position {h.to_host(st['pos'])}")
    c0, c1 = res[0.0], res[kw["w_obs"]]
    assert np.all(c0 <= -0.2), f"without the penalty the sphere goes through every drone: {c0}"
    assert np.all(c1 >= 0.2), f"with the penalty every drone keeps clear: {c1}"


# ---- 8. determinism, dirty buffers, a NaN drone ----------------------------------------------------------------------------------------
def check_determinism_and_dirty_buffers(h, N=6, B=3, K=3, t0=T0):
    """Two runs give the same bytes; outputs pre-filled with NaN come back fully written (both entries); a drone with a NaN state does not
    disturb its neighbours."""
    sc = Scene(h, N, B, K=K, seed=4, vel=velocities(K, 4), t0=t0)
    a, b = sc.fresh(), sc.fresh()
    oa = sc.call(a, 2, 3, 0.01, 1)
    ob = sc.call(b, 2, 3, 0.01, 1)
    lc.same_bits(a, b, "run to run")
    _same_outputs(oa, ob, "run to run", ("cost", "trace", "plan_last"))
    d = sc.fresh()
    suf = "f32" if h.dt == np.float32 else "f64"
    be = h.ops.be
    trace = sc.d(np.full((B, 2, sc.iters), np.nan)); plan = sc.d(np.full((B, 3, N, 3), np.nan)); cost = sc.d(np.full(B, np.nan))
    h.ops.lib.loop_call("mppi_closed_loop_moving", suf, sc.prm, sc.cp, sc.sp, B, 2, 3, 0.01, 0, 1, sc.S, sc.iters, sc.sigma, sc.lam, sc.seed, 0, 0,
                        be.ptr(sc.goal_d), be.ptr(sc.sph_d), be.ptr(sc.vel_d), t0, K, sc.w_obs, be.ptr(sc.wind_d), 3, be.ptr(d["time"]),
                        be.ptr(d["pos"]), be.ptr(d["vel"]), be.ptr(d["att"]), be.ptr(d["omega"]), be.ptr(d["state"]), be.ptr(d["U"]), be.ptr(cost),
                        be.ptr(trace), be.ptr(plan), be.ptr(d["clearance"]), be.stream())
    lc.same_bits(a, d, "dirty buffers")
    assert lc.bits_equal(trace, oa["trace"]) and lc.bits_equal(plan, oa["plan_last"]) and lc.bits_equal(cost, oa["cost"])
    # the planner entry, outputs full of NaN
    run = Run(h, sc.prm, sc.p0, sc.v0, sc.goal, sc.U0, sc.sph, sc.vel, sc.w_obs, t0)
    ref = run(64, 2, 1.0, 50.0, seed=3)
    nan = lambda shape, dt=h.dt: h.to_dev(np.full(shape, np.nan, dt))
    out = (nan((3 * N, B)), nan((B,)), nan((2, B)), h.to_dev(np.full((B,), -1, np.int64)))
    _same_outputs(run(64, 2, 1.0, 50.0, seed=3, out=out), ref, "dirty buffers, planner")
    # a drone whose state is NaN: its neighbours' bytes are those of the clean run
    p0 = sc.p0.copy(); p0[1] = np.nan
    sn = Scene(h, N, B, K=K, seed=4, vel=sc.vel, t0=t0, p0=p0)
    n = sn.fresh()
    sn.call(n, 2, 3, 0.01, 1)
    for k in lc.STATE_KEYS + ("clearance",):
        for i in (0, 2):
            assert lc.bits_equal(n[k][i], a[k][i]), f"NaN neighbour: {k} of drone {i}"


# ---- 9. invalid arguments --------------------------------------------------------------------------------------------------------------
def check_invalid_arguments(h, N=6):
    """Both entries: NULL sphere_vel with K > 0 (-1), a non-finite sphere_t0 (-4), and every refusal the static entries make; each sets
    se3mpc_last_error and launches nothing."""
    nan, inf = float("nan"), float("inf")
    suf = "f32" if h.dt == np.float32 else "f64"
    ops, be, lib = h.ops, h.ops.be, h.ops.lib
    # ---- se3mpc_mppi_moving_*
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, 2, 1, K=2)
    run = Run(h, prm, p0, v0, goal, U, sph, velocities(2, 1), 1.0)
    Uo = h.to_dev(np.zeros((3 * N, 2), h.dt))
    cost = h.to_dev(np.zeros(2, h.dt))
    ok = dict(prm=prm, nprob=2, ld=2, S=64, iters=1, sigma=1.0, lam=1.0, K=2, w=1.0, U=be.ptr(run.U), spheres=be.ptr(run.sph), vel=be.ptr(run.vel),
              t0=0.5)

    def status(**kw):
        a = dict(ok, **kw)
        return lib.call_status("mppi_moving", suf, a["nprob"], a["ld"], a["S"], a["iters"], a["sigma"], a["lam"], 0, 0, None, 0, be.ptr(run.p0),
                               be.ptr(run.v0), be.ptr(run.goal), a["U"], be.ptr(Uo), a["spheres"], a["vel"], a["t0"], a["K"], a["w"], be.ptr(cost),
                               None, None, be.stream(), params=a["prm"])

    cases = [(dict(vel=None), -1), (dict(t0=nan), -4), (dict(t0=inf), -4), (dict(t0=-inf), -4),
             (dict(S=0), -3), (dict(S=63), -3), (dict(S=96), -3), (dict(S=65536 + 64), -3), (dict(S=-64), -3), (dict(lam=0.0), -4),
             (dict(lam=-1.0), -4), (dict(lam=nan), -4), (dict(lam=inf), -4), (dict(sigma=-0.5), -4),
             (dict(sigma=nan), -4), (dict(K=-1), -3), (dict(K=257), -3), (dict(prm=prm.copy(horizon=65)), -2),
             (dict(prm=prm.copy(dt=0.0)), -4), (dict(prm=None), -1), (dict(nprob=-1), -3), (dict(ld=1), -3), (dict(iters=-1), -3),
             (dict(w=nan), -4), (dict(w=-1.0), -4), (dict(U=None), -1), (dict(spheres=None), -1)]
    for kw, want in cases:
        got = status(**kw)
        assert got == want, f"se3mpc_mppi_moving {kw}: {got} != {want}"
        assert lib.last_error(), f"{kw}: se3mpc_last_error not set"
    assert np.all(h.to_host(Uo) == 0), "a rejected call launched"
    assert status() == 0 and status(nprob=0, U=None) == 0 and status(K=0, spheres=None, vel=None) == 0
    assert not np.all(h.to_host(Uo) == 0)
    # ---- se3mpc_mppi_closed_loop_moving_*
    B = 2
    sc = Scene(h, N, B, K=2, seed=1, vel=velocities(2, 1), t0=0.5)
    st = sc.fresh()
    keep = {k: v.clone() for k, v in st.items()}
    cost = sc.d(np.zeros(B))
    ok = dict(prm=sc.prm, cp=sc.cp, sp=sc.sp, B=B, cycles=1, substeps=2, sim_dt=0.01, shift=1, S=64, iters=1, sigma=1.0, lam=1.0, goal=be.ptr(sc.goal_d),
              spheres=be.ptr(sc.sph_d), vel=be.ptr(sc.vel_d), t0=0.5, K=2, w=1.0, wind=be.ptr(sc.wind_d), wstride=3, time=be.ptr(st["time"]),
              pos=be.ptr(st["pos"]), state=be.ptr(st["state"]), U=be.ptr(st["U"]), cost=be.ptr(cost))

    def lstatus(**kw):
        a = dict(ok, **kw)
        return lib.loop_status("mppi_closed_loop_moving", suf, a["prm"], a["cp"], a["sp"], a["B"], a["cycles"], a["substeps"], a["sim_dt"], 0, a["shift"],
                               a["S"], a["iters"], a["sigma"], a["lam"], 0, 0, 0, a["goal"], a["spheres"], a["vel"], a["t0"], a["K"], a["w"], a["wind"],
                               a["wstride"], a["time"], a["pos"], be.ptr(st["vel"]), be.ptr(st["att"]), be.ptr(st["omega"]), a["state"], a["U"],
                               a["cost"], None, None, be.ptr(st["clearance"]), be.stream())

    bad_cp = ControllerParams.from_config(sc.ccfg); bad_cp.mass = 0.0
    bad_sp = SimulatorParams.reference_defaults(mass=-1.0)
    cases = [(dict(vel=None), -1), (dict(t0=nan), -4), (dict(t0=inf), -4), (dict(t0=-inf), -4),
             (dict(S=0), -3), (dict(S=63), -3), (dict(S=96), -3), (dict(S=65536 + 64), -3), (dict(S=-64), -3), (dict(lam=0.0), -4),
             (dict(lam=-1.0), -4), (dict(lam=nan), -4), (dict(lam=inf), -4), (dict(sigma=-0.5), -4), (dict(sigma=nan), -4), (dict(sigma=inf), -4),
             (dict(K=-1), -3), (dict(K=257), -3), (dict(prm=sc.prm.copy(horizon=65)), -2), (dict(prm=sc.prm.copy(dt=0.0)), -4), (dict(prm=None), -1),
             (dict(cp=None), -1), (dict(sp=None), -1), (dict(cp=bad_cp), -4), (dict(sp=bad_sp), -4), (dict(B=-1), -3), (dict(cycles=-1), -3),
             (dict(substeps=-1), -3), (dict(iters=-1), -3), (dict(shift=-1), -3), (dict(shift=N + 1), -3), (dict(w=nan), -4), (dict(w=-1.0), -4),
             (dict(w=inf), -4), (dict(sim_dt=nan), -4), (dict(sim_dt=inf), -4), (dict(wstride=2), -3), (dict(U=None), -1), (dict(spheres=None), -1),
             (dict(goal=None), -1), (dict(time=None), -1), (dict(pos=None), -1), (dict(state=None), -1), (dict(cost=None), -1)]
    for kw, want in cases:
        got = lstatus(**kw)
        assert got == want, f"se3mpc_mppi_closed_loop_moving {kw}: {got} != {want}"
        assert lib.last_error(), f"{kw}: se3mpc_last_error not set"
    for k, v in keep.items():
        assert lc.bits_equal(st[k], v), f"a rejected call launched ({k})"
    assert lstatus(B=0, U=None) == 0 and lstatus(cycles=0, U=None) == 0
    for k, v in keep.items():
        assert lc.bits_equal(st[k], v), f"B = 0 / cycles = 0 are no-ops ({k})"
    assert lstatus(K=0, spheres=None, vel=None) == 0 and lstatus(wind=None, wstride=0) == 0
    assert not lc.bits_equal(st["pos"], keep["pos"])


# ---- 10. front end ---------------------------------------------------------------------------------------------------------------------
def check_front_end(h, make_planner, N=6, B=3, K=2):
    """SE3MPCPlanner.add_moving_obstacle through plan_mppi and plan_batch_mppi to the moving entry; the float64 host rebase (a state
    timestamp of 1.7e9 plans what timestamp 0 plans); clear_obstacles; the ValueErrors; run_mppi == run_mppi_fused with velocities."""
    import pytest
    from dart_planner_amd.common.types import DroneState
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    prec = "f32" if h.dt == np.float32 else "f64"
    kw = dict(n_samples=64, iters=2, sigma=2.0, temperature=50.0, seed=1, precision=prec, warm_start=False, obstacle_weight=40.0)
    goal = np.array([3.0, 1.0, 2.0])
    pos, velo = np.array([0.0, 0.0, 2.0]), np.zeros(3)
    c, r, v = np.array([0.2, -1.0, 2.1]), 0.5, np.array([0.0, 2.5, 0.0])

    def planned(now, obstacle_time, moving=True):
        pl = make_planner(N)
        pl.add_obstacle(np.array([5.0, 5.0, 5.0]), 0.3)
        if moving:
            pl.add_moving_obstacle(c, r, v, obstacle_time)
        else:
            pl.add_obstacle(c + v * (now - obstacle_time), r)
        tr = pl.plan_mppi(DroneState(timestamp=now, position=pos, velocity=velo), goal, **kw)
        return pl, tr, dict(pl.last_result)

    pl, tr, r0 = planned(10.0, 9.5)
    assert np.all(np.isfinite(tr.positions)) and r0["penalty"] > 0, r0
    assert r0["penalty"] == r0["cost_with_penalty"] - r0["cost"]
    # the same call made by hand on the rebased table
    ops, prm = pl._get_ops(), pl._params()
    tab = pl._moving_obstacle_table(None, 10.0)
    assert tab.shape == (2, 7) and np.array_equal(tab[1], [*(c + v * 0.5), r, *v]) and np.array_equal(tab[0], [5.0, 5.0, 5.0, 0.3, 0, 0, 0])
    col = lambda a: ops.be.from_host(np.ascontiguousarray(np.asarray(a, float).reshape(-1, 1).astype(h.dt)))
    dev = lambda a: ops.be.from_host(np.ascontiguousarray(np.asarray(a, float).astype(h.dt)))
    o = ops.mppi(prm, col(pos), col(velo), col(goal), col(np.tile([0.0, 0.0, pl.hover_thrust], (N, 1))), 64, 2, 2.0, 50.0, seed=1, spheres=dev(tab[:, :4]),
                 obstacle_weight=40.0, sphere_vel=dev(tab[:, 4:]), sphere_t0=0.0)
    assert np.array_equal(np.asarray(ops.be.to_host(o["U"]), float)[:, 0].reshape(N, 3), r0["U"]), "plan_mppi == Ops.mppi on the rebased table"
    assert float(np.asarray(ops.be.to_host(o["cost"]), float)[0]) == r0["cost_with_penalty"], "cost_with_penalty is the moving entry's cost"
    _, _, snap = planned(10.0, 9.5, moving=False)
    assert not np.array_equal(snap["U"], r0["U"]), "a snapshot of the obstacle plans something else"
    # the host rebase: epoch-sized timestamps
    _, _, r1 = planned(1.7e9, 1.7e9 - 0.5)
    _, _, r2 = planned(0.0, -0.5)
    assert np.array_equal(r1["U"], r2["U"]) and r1["cost_with_penalty"] == r2["cost_with_penalty"], "the rebase is done in float64 on the host"
    assert np.array_equal(r1["U"], r0["U"])
    # plan_batch_mppi rows are single problems on the same table
    res = pl.plan_batch_mppi(pos[None], velo[None], goal[None], n_samples=64, iters=2, sigma=2.0, temperature=50.0, seed=1, precision=prec,
                             obstacle_weight=40.0, timestamp=10.0)
    assert np.array_equal(res["thrust_vectors"][0], r0["U"]) and res["cost"][0] == r0["cost_with_penalty"]
    # (K, 7) arrays and the ValueErrors
    fresh = make_planner(N)                                     # (a planner's iteration counter advances from plan to plan)
    fresh.plan_mppi(DroneState(timestamp=3.0, position=pos, velocity=velo), goal, obstacles=tab, **kw)
    assert np.array_equal(fresh.last_result["U"], r0["U"]), "an explicit (K, 7) table holds at the state's timestamp"
    with pytest.raises(ValueError, match="split"):
        pl.plan_mppi(DroneState(timestamp=10.0, position=pos, velocity=velo), goal, splits=1, **kw)
    with pytest.raises(ValueError, match="split"):
        pl.plan_batch_mppi(pos[None], velo[None], goal[None], n_samples=128, iters=1, precision=prec, splits=2, timestamp=10.0)
    pl.clear_obstacles()
    assert pl.obstacles == [] and pl.moving_obstacles == [] and pl._moving_obstacle_table(None, 0.0) is None
    # ClosedLoopMonteCarlo
    sc = Scene(h, N, B, K=K, seed=2, vel=velocities(K, 2))
    mcl = ClosedLoopMonteCarlo(h.ops, sc.prm)
    p0, v0 = sc.d(sc.p0), sc.d(sc.v0)
    args = (p0, v0, sc.goal_d, 3, 10, 0.01, 64, 2, 1.0, 50.0)
    kw = dict(seed=9, spheres=sc.sph_d, obstacle_weight=40.0, wind=sc.wind_d)
    mv = dict(sphere_velocities=sc.vel_d, sphere_t0=0.7)
    a = mcl.run_mppi(*args, log=True, **kw, **mv)
    b = mcl.run_mppi_fused(*args, log=True, **kw, **mv)
    s = mcl.run_mppi_fused(*args, **kw)
    for k in ("pos", "vel", "att", "omega", "time", "controller_state", "U", "cost", "trace", "clearance"):
        assert lc.bits_equal(a[k], b[k]), k
    assert lc.bits_equal(a["logs"][-1]["plan_last"], b["logs"][0]["plan_last"])
    assert not lc.bits_equal(s["clearance"], b["clearance"]), "the velocities reach the kernel"
    for name in ("run_mppi_fused_staged", "run_mppi_edge", "run_mppi_edge_fused"):
        with pytest.raises(ValueError, match="moving"):
            getattr(mcl, name)(*args, **kw, **mv)
    sm = mcl.run_mppi(*args, smoother=h.ops.lib.smoother_default_params(), **kw, **mv)
    assert sm["clearance"] is None
    with pytest.raises(ValueError, match="sphere_vel"):                     # the smoothed chain's planner-only call gets the velocities
        mcl.run_mppi(*args, smoother=h.ops.lib.smoother_default_params(), **kw, sphere_velocities=sc.vel_d[:1].contiguous())
