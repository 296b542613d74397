"""Checks of MPPI around tracked spheres and of the swarm's shared plans (se3mpc_mppi_tracks_*, se3mpc_mppi_closed_loop_tracks_*,
se3mpc_swarm_intent_*, se3mpc_mppi_closed_loop_swarm_intent_*; Ops.mppi_tracks / mppi_closed_loop_tracks / swarm_intent /
mppi_closed_loop_swarm(share_plans=True); SE3MPCPlanner.add_tracked_obstacle; ClosedLoopMonteCarlo.run_mppi_fused(tracks=) /
run_mppi_swarm(share_plans=True)) shared by the host-emulation suite (tests/test_emu_mppi_tracks.py) and the MI355X suite
(tests/test_gpu_mppi_tracks.py).  Every check takes a parity_checks.Harness whose arrays are torch tensors.

Bounds: none new.  Against the float64 oracles (tests/mppi_tracks_oracle.py, tests/swarm_intent_oracle.py) U, cost and trace are held to the
bounds of tests/mppi_checks.py and the intent to parity_checks' position bound; selection and separation are exact against
tests/swarm_oracle.py; everything else is bit for bit."""
import numpy as np

import mppi_checks as mc
import mppi_closed_loop_checks as lc
import mppi_moving_checks as mv
import mppi_moving_oracle as mvo
import mppi_oracle as mo
import mppi_swarm_checks as sw
import mppi_tracks_oracle as mto
import swarm_intent_oracle as sio
import swarm_oracle as so
from dart_planner_amd.capi import ControllerParams, SimulatorParams
from oracle import se3mpc_oracle as orc

OUT_KEYS = ("cost", "trace", "plan_last")


def _round(h, a):
    return np.asarray(a, float).astype(h.dt).astype(float)


class Run(mv.Run):
    """mppi_moving_checks.Run on the tracks entry: the slab (N, Kt, 4) or (nprob, N, Kt, 4) rides along."""

    def __init__(self, h, prm, p0, v0, goal, U, sph, vel, tracks, w_obs=0.0, t0=0.0):
        super().__init__(h, prm, p0, v0, goal, U, sph, vel, w_obs, t0)
        self.tracks = h.to_dev(np.ascontiguousarray(np.asarray(tracks, float).astype(h.dt)))

    def __call__(self, S, iters, sigma, lam, t0=None, seed=0, iter_base=0, index_base=0, U=None, **kw):
        return self.h.ops.mppi_tracks(self.prm, self.p0, self.v0, self.goal, self.U if U is None else U, S, iters, sigma, lam, self.tracks, seed=seed,
                                      iter_base=iter_base, index_base=index_base, spheres=self.sph, obstacle_weight=self.w_obs, sphere_vel=self.vel,
                                      sphere_t0=self.t0 if t0 is None else t0, **kw)


def _same(a, b, what, keys):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        assert lc.bits_equal(a[k], b[k]), f"{what}: {k}"


# ---- 1. reduces to what exists ---------------------------------------------------------------------------------------------------------
def check_no_tracks_is_the_moving_planner(h, N, S, nprob, K, iters=2, seed=5, sigma=1.0, w_obs=40.0):
    """se3mpc_mppi_tracks_* with Kt = 0 (one empty slab, and one per problem): U, cost, trace and keys of se3mpc_mppi_moving_*."""
    prm, cfg, p0, v0, goal, U, sph, vel = mv.crossing_problem(h, N, nprob, K, seed)
    ref = mv.Run(h, prm, p0, v0, goal, U, sph, vel, w_obs, mv.T0)(S, iters, sigma, 50.0, seed=seed, iter_base=2, index_base=3)
    for shape in ((N, 0, 4), (nprob, N, 0, 4)):
        got = Run(h, prm, p0, v0, goal, U, sph, vel, np.zeros(shape), w_obs, mv.T0)(S, iters, sigma, 50.0, seed=seed, iter_base=2, index_base=3)
        _same(got, ref, f"Kt = 0, slab {shape}", ("U", "cost", "trace", "keys"))


def check_no_tracks_is_the_moving_loop(h, N, B, K, S=64, cycles=2, substeps=3, sim_dt=0.01, shift=1, seed=5):
    """se3mpc_mppi_closed_loop_tracks_* with Kt = 0: state, U, cost, trace, plan_last and clearance of se3mpc_mppi_closed_loop_moving_*."""
    sc = mv.Scene(h, N, B, K=K, S=S, seed=seed, vel=mv.velocities(K, seed), t0=mv.T0)
    a, b = sc.fresh(), sc.fresh()
    oa = sc.call(a, cycles, substeps, sim_dt, shift, iter_base=7)
    ob = sc.call(b, cycles, substeps, sim_dt, shift, iter_base=7, tracks=sc.d(np.zeros((cycles, B, N, 0, 4))))
    lc.same_bits(a, b, "Kt = 0 vs the moving loop")
    _same(oa, ob, "Kt = 0 vs the moving loop", OUT_KEYS)


def _held_problem(h, N, nprob, K, Kt, seed):
    """mppi_moving_checks.crossing_problem on K + Kt spheres whose last Kt stand still, the first of those on problem 0's nominal."""
    prm, cfg, p0, v0, goal, U, sph, vel = mv.crossing_problem(h, N, nprob, K + Kt, seed)
    vel[K:] = 0.0
    if N > 1:
        P, _ = orc.rollout(p0[0], v0[0], U[0], cfg)
        sph[K, :3] = P[N // 2] + [0.05, -0.1, 0.08]
        sph = _round(h, sph)
    tracks = np.broadcast_to(sph[K:][None], (N, Kt, 4)).copy()
    return prm, cfg, p0, v0, goal, U, sph, vel, tracks


def check_held_tracks_are_still_spheres_planner(h, N, S, nprob, K, Kt, iters=2, seed=5, sigma=1.0, w_obs=40.0):
    """K moving rows + Kt tracks that hold one centre == se3mpc_mppi_moving_* on K + Kt rows whose last Kt velocities are zero, bit for bit."""
    prm, cfg, p0, v0, goal, U, sph, vel, tracks = _held_problem(h, N, nprob, K, Kt, seed)
    if N > 1:
        assert mto.track_penalty(p0[0], v0[0], U[0], tracks, cfg, w_obs) > 0, "the check wants a nominal inside a tracked sphere's margin"
    ref = mv.Run(h, prm, p0, v0, goal, U, sph, vel, w_obs, mv.T0)(S, iters, sigma, 50.0, seed=seed, iter_base=2, index_base=3)
    for slab in (tracks, np.broadcast_to(tracks[None], (nprob, N, Kt, 4))):
        got = Run(h, prm, p0, v0, goal, U, sph[:K], vel[:K], slab, w_obs, mv.T0)(S, iters, sigma, 50.0, seed=seed, iter_base=2, index_base=3)
        _same(got, ref, f"held tracks, slab {np.shape(slab)}", ("U", "cost", "trace", "keys"))


def check_held_tracks_are_still_spheres_loop(h, N, B, K, Kt, S=64, cycles=2, substeps=3, sim_dt=0.01, shift=1, seed=5):
    """The same through the closed loop: state, U, cost, trace and plan_last of se3mpc_mppi_closed_loop_moving_* on K + Kt rows (no
    clearance: the moving loop's sees all K + Kt rows, the tracks loop's the K moving rows)."""
    probe = mv.Scene(h, N, B, K=K + Kt, S=S, seed=seed)
    sph = probe.sph.copy()
    sph[K, :3] = probe.p0[0] + [0.3, -0.2, 0.25]                # the first held track stands on drone 0
    full = mv.Scene(h, N, B, K=K + Kt, S=S, seed=seed, vel=np.concatenate([mv.velocities(K, seed), np.zeros((Kt, 3))]), t0=mv.T0, sph=sph)
    part = mv.Scene(h, N, B, K=K + Kt, S=S, seed=seed, vel=full.vel, t0=mv.T0, sph=sph)
    part.sph_d, part.vel_d = (part.d(full.sph[:K]), part.d(full.vel[:K])) if K else (None, part.d(np.zeros((0, 3))))
    slab = np.broadcast_to(full.sph[K:], (cycles, B, N, Kt, 4))
    a, b = full.fresh(), part.fresh()
    a["clearance"] = b["clearance"] = None
    oa = full.call(a, cycles, substeps, sim_dt, shift, iter_base=7, clearance=None, want_clearance=False)
    ob = part.call(b, cycles, substeps, sim_dt, shift, iter_base=7, clearance=None, want_clearance=False, tracks=part.d(slab))
    _same(a, b, "held tracks vs the moving loop", lc.STATE_KEYS)
    _same(oa, ob, "held tracks vs the moving loop", OUT_KEYS)
    none = part.fresh()
    none["clearance"] = None
    part.call(none, cycles, substeps, sim_dt, shift, iter_base=7, clearance=None, want_clearance=False)
    assert not lc.bits_equal(none["U"], b["U"]), "the tracked rows must reach the planner"


def check_unshared_plans_are_the_swarm_call(h, N=6, S=64, swarms=2, M=5, Kn=3, Ks=2, cycles=2, substeps=3, sim_dt=0.01, shift=1):
    """share_plans=False is the swarm call as it was (the same bytes as a call without the keyword); share_plans=True with swarm_size = 1 or
    neighbours_k = 0 is se3mpc_mppi_closed_loop_moving_* -- mppi_swarm_checks.check_reduces_to_moving's counterpart."""
    sc = sw.Scene(h, N, swarms, M, Ks=Ks, Kn=Kn, S=S)
    a, b = sc.fresh(), sc.fresh()
    oa = sc.swarm(a, cycles, substeps, sim_dt, shift, iter_base=7)
    ob = sc.swarm(b, cycles, substeps, sim_dt, shift, iter_base=7, share_plans=False)
    _same(a, b, "share_plans=False", lc.STATE_KEYS + ("clearance", "separation"))
    _same(oa, ob, "share_plans=False", OUT_KEYS + ("neighbours",))
    for m, kn in ((1, Kn), (M, 0)):
        sc = sw.Scene(h, N, swarms * M // m, m, Ks=Ks, Kn=kn, S=S)
        a, b = sc.fresh(), sc.fresh()
        oa = sc.call(a, cycles, substeps, sim_dt, shift, iter_base=7)
        ob = sc.swarm(b, cycles, substeps, sim_dt, shift, iter_base=7, share_plans=True)
        lc.same_bits(a, b, f"shared plans, M = {m}, Kn = {kn} vs the moving loop")
        _same(oa, ob, f"shared plans, M = {m}, Kn = {kn} vs the moving loop", OUT_KEYS)


# ---- 2. the planner against the oracle -------------------------------------------------------------------------------------------------
def arc_problem(h, N, nprob, K, Kt, seed, t0=mv.T0):
    """mppi_moving_checks.crossing_problem plus Kt tracks per problem.  Track 0 of problem 0 (r = 0.5 m) runs on an arc of radius 6 m at 0.45
    rad per step that passes 0.13 m from the nominal at step km = N - 2; the others wander on arcs of their own.  Problem p's slab is
    problem 0's shifted by 0.1 p m along x.  -> (..., tracks (nprob, N, Kt, 4), km)."""
    prm, cfg, p0, v0, goal, U, sph, vel = mv.crossing_problem(h, N, nprob, K, seed, t0)
    rng = np.random.default_rng(seed + 31)
    km = max(N - 2, 0)
    P, _ = orc.rollout(p0[0], v0[0], U[0], cfg)
    k = np.arange(N, dtype=float)
    tracks = np.empty((nprob, N, Kt, 4))
    for j in range(Kt):
        R, w, ph = (6.0, 0.45, 0.0) if j == 0 else (rng.uniform(1, 3), rng.uniform(-0.5, 0.5), rng.uniform(0, 6))
        at = P[km] + [0.1, -0.05, 0.06] if j == 0 else rng.uniform(-3, 3, 3) + [0, 0, 2]
        th = w * (k - km) + ph
        c = at + R * np.stack([np.cos(th) - np.cos(ph), np.sin(th) - np.sin(ph), 0.1 * (k - km)], axis=1)
        tracks[0, :, j, :3] = c
        tracks[0, :, j, 3] = 0.5 if j == 0 else rng.uniform(0.3, 1.0)
    for p in range(1, nprob):
        tracks[p] = tracks[0] + [0.1 * p, 0, 0, 0]
    return prm, cfg, p0, v0, goal, U, sph, vel, _round(h, tracks), km


def check_against_oracle(h, N, S, nprob, iters, K, Kt, seed=5, sigma=1.0, w_obs=40.0, t0=mv.T0):
    """U, cost, trace of se3mpc_mppi_tracks_* against the float64 oracle on curved tracks, one slab per problem and one for all (track_stride
    = 0), iters = 0 included.  On the oracle first: track 0 covers problem 0's nominal at step km, and the straight-line sphere through the
    track's first two points -- the best a (c, v) pair could do from there -- covers it at no step."""
    prm, cfg, p0, v0, goal, U, sph, vel, tracks, km = arc_problem(h, N, nprob, K, Kt, seed, t0)
    tR = mvo.step_times(N, cfg.dt, t0, h.dt)
    if N > 2:
        P, _ = orc.rollout(p0[0], v0[0], U[0], cfg)
        arc = mto.track_residuals(P, tracks[0], cfg)[:, 0]
        c0, c1 = tracks[0, 0, 0, :3], tracks[0, 1, 0, :3]
        line = np.stack([np.concatenate([c0 + (c1 - c0) * k, [tracks[0, 0, 0, 3]]]) for k in range(N)])[:, None, :]
        straight = mto.track_residuals(P, line, cfg)[:, 0]
        print(f"arc residual at step {km}: {arc[km]:.3f}; the straight line's smallest: {straight.min():.3f}")
        assert arc[km] < 0, "track 0 covers the nominal at step km"
        assert np.all(straight > 0), "the straight-line sphere through the track's first two points covers the nominal nowhere"
    T, _, _ = mo.samples(U[0], 0, 0, S, sigma, seed, cfg)
    c = mto.cost(p0[0], v0[0], goal[0], T, cfg, sph, vel, tR, tracks[0], w_obs)
    lam = float(np.median(c) - np.min(c))
    for slab in (tracks, tracks[0]):
        run = Run(h, prm, p0, v0, goal, U, sph, vel, slab, w_obs, t0)
        for it in (iters, 0):
            Ud, cd, trd, keys = run.host(run(S, it, sigma, lam, seed=seed, iter_base=2, index_base=0))
            for p in range(nprob):
                tr_p = slab[p] if slab.ndim == 4 else slab
                Ur, cr, trr = mto.mppi(p0[p], v0[p], goal[p], U[p], p, S, it, sigma, lam, seed, cfg, iter_base=2, spheres=sph, vel=vel, sphere_t0=t0,
                                       tracks=tr_p, obstacle_weight=w_obs, dtype=h.dt)
                if h.dt == np.float32:
                    errU = np.max(np.abs(Ud[p] - Ur))
                    c_at = mto.cost(p0[p], v0[p], goal[p], Ud[p], cfg, sph, vel, tR, tr_p, w_obs)      # the cost of the nominal the kernel returned
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
    if N > 2:
        none = Run(h, prm, p0, v0, goal, U, sph, vel, np.zeros((N, 0, 4)), w_obs, t0)
        assert not lc.bits_equal(none(S, 0, sigma, lam)["cost"][:1], run(S, 0, sigma, lam)["cost"][:1]), "the track must matter"


# ---- 3. the intent ---------------------------------------------------------------------------------------------------------------------
def check_intent(h, N, B, seed=5):
    """se3mpc_swarm_intent_* against the oracle's rollout to parity_checks' position bound, and bit for bit against the P rows of plan_last
    of se3mpc_mppi_closed_loop_* with iters = 0, substeps = 0, shift = 0 on the same (p0, v0, U): the hand-over is the entry whose recurrence
    the intent shares (roll_state_step).  The states of rollout_cost_grad(..., want_states=True) come from the rollout kernels' own sweep, a
    different summation: mppi_closed_loop_checks.check_planner_inside holds the plan to them by a bound, and so does this check."""
    sc = lc.Scene(h, N, B, seed=seed, iters=0)
    got_d = h.ops.swarm_intent(sc.prm, sc.d(sc.p0), sc.d(sc.v0), sc.d(sc.U0))
    got = h.to_host(got_d).astype(float)
    want = sio.intent(sc.p0, sc.v0, sc.U0, sc.cfg)
    err = float(np.max(np.abs(got - want)))
    print(f"intent: max abs err {err:.3e} (bound {h.tol['pos']:.0e})")
    assert got.shape == (B, N, 3) and err <= h.tol["pos"], err
    assert np.array_equal(got[:, 0], sc.p0), "row 0 is the drone's position"
    st = sc.fresh()
    out = sc.call(st, 1, 0, 0.01, 0)
    assert lc.bits_equal(out["plan_last"][:, 0].contiguous(), got_d), "intent == the plan the loop hands over at that nominal"
    run = mc.Run(h, sc.prm, sc.p0, sc.v0, sc.goal, sc.U0)
    _, _, P, _ = h.ops.rollout_cost_grad(sc.prm, run.p0, run.v0, run.goal, run.U, want_grad=False, want_states=True)
    assert np.max(np.abs(h.unlane(P, (B, N, 3)) - got)) <= h.tol["pos"], "intent vs se3mpc_rollout_cost_grad_*'s states"
    keep = got_d.clone()
    h.ops.swarm_intent(sc.prm, sc.d(sc.p0), sc.d(sc.v0), sc.d(sc.U0), intent=got_d)
    assert lc.bits_equal(keep, got_d), "run to run"


# ---- 4. the chain ----------------------------------------------------------------------------------------------------------------------
def chain(sc, st, cycles, substeps, sim_dt, shift, iter_base=0):
    """`cycles` cycles of every drone through se3mpc_swarm_intent_* and se3mpc_mppi_closed_loop_tracks_* alone: per cycle
    se3mpc_swarm_intent_* on the whole call's (pos, vel, U), then per drone the host builds the slab from the rows swarm_oracle.ranked
    selects and calls the tracks entry with B = 1, index_base = b, cycle_base = C, one cycle, the shared table as its moving rows.
    -> dict(cost, trace, plan_last) as one call would return them, starts = [(pos, vel)] at every cycle's start."""
    import torch
    h, B = sc.h, sc.B
    starts, traces = [], []
    for C in range(cycles):
        pos, vel = sw._host(h, st)
        starts.append((pos, vel))
        intents = h.to_host(h.ops.swarm_intent(sc.prm, st["pos"], st["vel"], st["U"])).copy()
        outs = []
        for b in range(B):
            slab = sio.slab(intents, pos, vel, b, sc.M, sc.Kn, sc.mate_radius, h.dt)
            sub = {k: st[k][b:b + 1] for k in lc.STATE_KEYS}
            sub["clearance"] = None
            outs.append(sc.call(sub, 1, substeps, sim_dt, shift, cycle_base=C, lo=b, hi=b + 1, iter_base=iter_base, obstacle_weight=sc.w_obs,
                                clearance=None, want_clearance=False, tracks=h.to_dev(np.ascontiguousarray(slab[None, None]))))
        traces.append(torch.cat([o["trace"] for o in outs], dim=0))
    return dict(cost=torch.cat([o["cost"] for o in outs]), trace=torch.cat(traces, dim=1), plan_last=torch.cat([o["plan_last"] for o in outs], dim=0),
                starts=starts)


def check_chain(h, N, S, swarms, M, Kn, Ks, cycles=2, substeps=3, sim_dt=0.01, shift=1, seed=5, mates_matter=True, nan_drone=None, **scene_kw):
    """The main check: one se3mpc_mppi_closed_loop_swarm_intent_* call == the chain above, bit for bit on state, U, cost, trace and plan_last;
    the last cycle's neighbours and the separation equal swarm_oracle's exactly.  nan_drone: that drone's position holds a NaN -- it is in
    nobody's slab, and the comparison leaves its own rows out (NaN payloads are nobody's contract)."""
    p0 = np.concatenate([sw._spread(M, seed + s) for s in range(swarms)])
    sw.assert_no_ties(p0, M)
    if nan_drone is not None:
        p0 = p0.copy(); p0[nan_drone, 1] = np.nan
    sc = sw.Scene(h, N, swarms, M, Ks=Ks, Kn=Kn, S=S, seed=seed, p0=p0, **scene_kw)
    rows = [i for i in range(sc.B) if i != nan_drone]
    a, b = sc.fresh(), sc.fresh()
    ref = chain(sc, a, cycles, substeps, sim_dt, shift, iter_base=7)
    out = sc.swarm(b, cycles, substeps, sim_dt, shift, iter_base=7, share_plans=True)
    for k in lc.STATE_KEYS:
        assert lc.bits_equal(a[k][rows], b[k][rows]), f"shared-plans call vs the chain: {k}"
    for k in OUT_KEYS:
        assert lc.bits_equal(ref[k][rows], out[k][rows]), f"shared-plans call vs the chain: {k}"
    pos, vel = ref["starts"][-1]
    nb = h.to_host(out["neighbours"])
    assert np.array_equal(nb, so.neighbours(pos, vel, M, Kn)), "neighbours of the last cycle"
    if nan_drone is not None:
        assert not np.any(nb == nan_drone) and np.all(nb[nan_drone] == -1), "a drone with a NaN snapshot is in nobody's slab and has no mate"
    want = None
    for pos, vel in ref["starts"]:
        want = so.separation(pos, vel, M, h.dt, want)
    assert np.array_equal(h.to_host(b["separation"]), want), "separation = min over the cycle starts"
    if not mates_matter:
        return
    alone, mated = sc.fresh(), sc.fresh()
    sc.swarm(alone, 1, 0, sim_dt, shift, iter_base=7, neighbours=0, share_plans=True)
    sc.swarm(mated, 1, 0, sim_dt, shift, iter_base=7, share_plans=True)
    assert not lc.bits_equal(alone["U"][rows], mated["U"][rows]), "the mates' intents must reach the planner"


# ---- 5. the intent reaches the planner -------------------------------------------------------------------------------------------------
HEAD_ON = dict(N=10, mate_radius=0.3, margin=0.1, w_obs=2000.0)


def check_intent_reaches_the_planner(h):
    """Two drones head on as in mppi_swarm_checks.behaviour_scene (2 m apart at 3 m, 2 m/s each, meeting at step 5).  Drone A's nominal is full
    thrust: it climbs 1.27 m, more than mate_radius + margin = 0.4 m, before the meeting step; drone B's is hover.  With iters = 0 the entry
    returns the nominal's cost: B's carries a sphere penalty under share_plans=False (A extrapolated along its velocity flies through B's
    path) and none under share_plans=True (A's intent is above it).  Both signs on the oracle first, then on the entry."""
    kw = HEAD_ON
    N = kw["N"]
    bs = sw.behaviour_scene()
    prm = bs["prm"].copy(safety_margin=kw["margin"])
    U = bs["U"].copy()
    U[0, :, 2] = prm.max_thrust
    bs = dict(bs, prm=prm, U=U)
    res = {}
    for key, Kn, share in (("alone", 0, False), ("velocity", 1, False), ("plan", 1, True)):
        sc = sw.Scene(h, N, 1, 2, Ks=0, Kn=Kn, mate_radius=kw["mate_radius"], w_obs=kw["w_obs"], S=64, iters=0, wind=None, seed=1, t0=0.0, **bs)
        if key == "alone":
            cfg = sc.cfg
            I = sio.intent(sc.p0, sc.v0, sc.U0, cfg)
            assert I[0, 5, 2] - I[0, 0, 2] > kw["mate_radius"] + kw["margin"], "A climbs by more than mate_radius + margin before the meeting step"
            tR = mvo.step_times(N, cfg.dt, 0.0, h.dt)
            ms, mvel = so.mate_rows(sc.p0, sc.v0, [0], 0.0, kw["mate_radius"], h.dt)
            pen_v = mvo.penalty(sc.p0[1], sc.v0[1], sc.U0[1], ms.astype(float), mvel.astype(float), tR, cfg, kw["w_obs"])
            pen_p = mto.track_penalty(sc.p0[1], sc.v0[1], sc.U0[1], sio.slab(I, sc.p0, sc.v0, 1, 2, 1, kw["mate_radius"], np.float64), cfg, kw["w_obs"])
            print(f"oracle: B's penalty against A extrapolated {pen_v:.1f}, against A's intent {pen_p:.1f}")
            assert pen_v > 0 and pen_p == 0, "the oracle: the extrapolated A covers B's path, A's intent does not"
        st = sc.fresh()
        res[key] = h.to_host(sc.swarm(st, 1, 0, 0.01, 1, share_plans=share)["cost"]).astype(float)
    print(f"B's nominal cost: alone {res['alone'][1]}, velocity {res['velocity'][1]}, plan {res['plan'][1]}")
    assert res["velocity"][1] > res["alone"][1], "share_plans=False: B's nominal cost carries the penalty of A extrapolated"
    assert res["plan"][1] == res["alone"][1], "share_plans=True: B's nominal cost carries no penalty"


# ---- 6. continuation, determinism, dirty buffers ---------------------------------------------------------------------------------------
def check_continuation_and_determinism(h, N=6, S=64, swarms=2, M=5, Kn=3, Ks=2, cycles=3, substeps=3, sim_dt=0.01, shift=1):
    """cycles = 3 in one call == three chained calls, and == a run split 2 + 1 through cycle_base, whose second call needs the intents of the
    first call's end: the entry reseeds them from (pos, vel, U), and se3mpc_swarm_intent_* on the state between the calls shows what it
    reseeds with (the intent image is scratch; nothing is carried).  Two runs give the same bytes; a workspace larger than required and full
    of NaN, and outputs full of NaN, give the same bytes."""
    sc = sw.Scene(h, N, swarms, M, Ks=Ks, Kn=Kn, S=S)
    B = sc.B
    keys = lc.STATE_KEYS + ("clearance", "separation")
    one = sc.fresh()
    o1 = sc.swarm(one, cycles, substeps, sim_dt, shift, iter_base=7, share_plans=True)
    many = sc.fresh()
    for c in range(cycles):
        oc = sc.swarm(many, 1, substeps, sim_dt, shift, cycle_base=c, iter_base=7, share_plans=True)
        assert lc.bits_equal(oc["trace"][:, 0], o1["trace"][:, c]), f"trace of cycle {c}"
    _same(one, many, "cycles = C vs C calls", keys)
    _same(o1, oc, "cycles = C vs C calls", ("cost", "plan_last", "neighbours"))
    split = sc.fresh()
    sc.swarm(split, cycles - 1, substeps, sim_dt, shift, iter_base=7, share_plans=True)
    reseed = h.ops.swarm_intent(sc.prm, split["pos"], split["vel"], split["U"])
    assert bool(np.all(np.isfinite(h.to_host(reseed)))) and lc.bits_equal(reseed[:, 0].contiguous(), split["pos"]), "the reseeded intent starts at the state"
    o2 = sc.swarm(split, 1, substeps, sim_dt, shift, cycle_base=cycles - 1, iter_base=7, share_plans=True)
    _same(one, split, "a run split through cycle_base", keys)
    _same(o1, o2, "a run split through cycle_base", ("cost", "plan_last", "neighbours"))
    again = sc.fresh()
    o3 = sc.swarm(again, cycles, substeps, sim_dt, shift, iter_base=7, share_plans=True)
    _same(one, again, "run to run", keys)
    _same(o1, o3, "run to run", OUT_KEYS + ("neighbours",))
    # garbage everywhere the call only writes, a workspace with room to spare
    import torch
    suf = "f32" if h.dt == np.float32 else "f64"
    be, esz = h.ops.be, np.dtype(h.dt).itemsize
    need = h.ops.lib.mppi_swarm_intent_workspace_bytes(B, N, esz)
    assert need == 2 * (6 + 3 * N) * B * esz
    ws = sc.d(np.full(need // esz + 7, np.nan))
    d = sc.fresh()
    trace = sc.d(np.full((B, cycles, sc.iters), np.nan)); plan = sc.d(np.full((B, 3, N, 3), np.nan)); cost = sc.d(np.full(B, np.nan))
    nb = h.to_dev(np.full((B, Kn), 0x7FC00000, np.int32))
    h.ops.lib.loop_call("mppi_closed_loop_swarm_intent", suf, sc.prm, sc.cp, sc.sp, B, M, Kn, sc.mate_radius, cycles, substeps, sim_dt, 0, shift, S,
                        sc.iters, sc.sigma, sc.lam, sc.seed, 7, 0, be.ptr(sc.goal_d), be.ptr(sc.sph_d), be.ptr(sc.vel_d), sc.t0, Ks, sc.w_obs,
                        be.ptr(sc.wind_d), 3, be.ptr(d["time"]), be.ptr(d["pos"]), be.ptr(d["vel"]), be.ptr(d["att"]), be.ptr(d["omega"]),
                        be.ptr(d["state"]), be.ptr(d["U"]), be.ptr(cost), be.ptr(trace), be.ptr(plan), be.ptr(d["clearance"]),
                        be.ptr(d["separation"]), be.ptr(nb), be.ptr(ws), int(ws.numel()) * esz, be.stream())
    _same(one, d, "dirty buffers", keys)
    assert lc.bits_equal(trace, o1["trace"]) and lc.bits_equal(plan, o1["plan_last"]) and lc.bits_equal(cost, o1["cost"])
    assert torch.equal(nb, o1["neighbours"])


def check_tracks_determinism_and_dirty_buffers(h, N=6, B=3, K=2, Kt=3, cycles=2):
    """The two tracks entries: two runs give the same bytes and outputs pre-filled with NaN come back fully written; cycles = 2 in one call ==
    two chained calls that are handed slab 0 and slab 1."""
    sc = mv.Scene(h, N, B, K=K, seed=4, vel=mv.velocities(K, 4), t0=mv.T0)
    rng = np.random.default_rng(11)
    slab = np.concatenate([rng.uniform(-2, 2, (cycles, B, N, Kt, 3)) + [0, 0, 2], rng.uniform(0.3, 1.0, (cycles, B, N, Kt, 1))], axis=-1)
    slab_d = sc.d(slab)
    a, b = sc.fresh(), sc.fresh()
    oa = sc.call(a, cycles, 3, 0.01, 1, tracks=slab_d)
    ob = sc.call(b, cycles, 3, 0.01, 1, tracks=slab_d)
    lc.same_bits(a, b, "run to run")
    _same(oa, ob, "run to run", OUT_KEYS)
    many = sc.fresh()
    for c in range(cycles):
        oc = sc.call(many, 1, 3, 0.01, 1, cycle_base=c, tracks=slab_d[c:c + 1].contiguous())
    lc.same_bits(a, many, "cycles = C vs C calls on their own slabs")
    _same(oa, oc, "cycles = C vs C calls on their own slabs", ("cost", "plan_last"))
    d = sc.fresh()
    suf = "f32" if h.dt == np.float32 else "f64"
    be = h.ops.be
    trace = sc.d(np.full((B, cycles, sc.iters), np.nan)); plan = sc.d(np.full((B, 3, N, 3), np.nan)); cost = sc.d(np.full(B, np.nan))
    h.ops.lib.loop_call("mppi_closed_loop_tracks", suf, sc.prm, sc.cp, sc.sp, B, cycles, 3, 0.01, 0, 1, sc.S, sc.iters, sc.sigma, sc.lam, sc.seed, 0, 0,
                        be.ptr(sc.goal_d), be.ptr(sc.sph_d), be.ptr(sc.vel_d), mv.T0, K, be.ptr(slab_d), Kt, sc.w_obs, be.ptr(sc.wind_d), 3,
                        be.ptr(d["time"]), be.ptr(d["pos"]), be.ptr(d["vel"]), be.ptr(d["att"]), be.ptr(d["omega"]), be.ptr(d["state"]), be.ptr(d["U"]),
                        be.ptr(cost), be.ptr(trace), be.ptr(plan), be.ptr(d["clearance"]), be.stream())
    lc.same_bits(a, d, "dirty buffers")
    assert lc.bits_equal(trace, oa["trace"]) and lc.bits_equal(plan, oa["plan_last"]) and lc.bits_equal(cost, oa["cost"])
    run = Run(h, sc.prm, sc.p0, sc.v0, sc.goal, sc.U0, sc.sph, sc.vel, slab[0], sc.w_obs, mv.T0)
    ref = run(64, 2, 1.0, 50.0, seed=3)
    nan = lambda shape, dt=h.dt: h.to_dev(np.full(shape, np.nan, dt))
    out = (nan((3 * N, B)), nan((B,)), nan((2, B)), h.to_dev(np.full((B,), -1, np.int64)))
    _same(run(64, 2, 1.0, 50.0, seed=3, out=out), ref, "dirty buffers, planner", ("U", "cost", "trace", "keys"))


# ---- 7. invalid arguments --------------------------------------------------------------------------------------------------------------
def check_invalid_arguments(h, N=6):
    """Every rule of the header for the four entries: the code, se3mpc_last_error set, no output touched."""
    nan, inf = float("nan"), float("inf")
    suf = "f32" if h.dt == np.float32 else "f64"
    be, lib = h.ops.be, h.ops.lib
    esz = np.dtype(h.dt).itemsize
    # ---- se3mpc_mppi_tracks_*
    Kt = 2
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, 2, 1, K=2)
    run = Run(h, prm, p0, v0, goal, U, sph, mv.velocities(2, 1), np.ones((2, N, Kt, 4)), 1.0)
    Uo = h.to_dev(np.zeros((3 * N, 2), h.dt))
    cost = h.to_dev(np.zeros(2, h.dt))
    ok = dict(prm=prm, nprob=2, ld=2, S=64, iters=1, sigma=1.0, lam=1.0, K=2, w=1.0, U=be.ptr(run.U), spheres=be.ptr(run.sph), vel=be.ptr(run.vel),
              t0=0.5, tracks=be.ptr(run.tracks), Kt=Kt, stride=4 * N * Kt)

    def status(**kw):
        a = dict(ok, **kw)
        return lib.call_status("mppi_tracks", suf, a["nprob"], a["ld"], a["S"], a["iters"], a["sigma"], a["lam"], 0, 0, None, 0, be.ptr(run.p0),
                               be.ptr(run.v0), be.ptr(run.goal), a["U"], be.ptr(Uo), a["spheres"], a["vel"], a["t0"], a["K"], a["tracks"], a["Kt"],
                               a["stride"], a["w"], be.ptr(cost), None, None, be.stream(), params=a["prm"])

    cases = [  # the tracks' own
             (dict(Kt=-1), -3), (dict(Kt=17), -3), (dict(K=255, Kt=2), -3), (dict(stride=4 * N * Kt - 1), -3), (dict(stride=-1), -3),
             (dict(tracks=None), -1),
             # those of se3mpc_mppi_moving_*
             (dict(vel=None), -1), (dict(t0=nan), -4), (dict(t0=inf), -4), (dict(t0=-inf), -4),
             (dict(S=0), -3), (dict(S=63), -3), (dict(S=96), -3), (dict(S=65536 + 64), -3), (dict(S=-64), -3), (dict(lam=0.0), -4),
             (dict(lam=-1.0), -4), (dict(lam=nan), -4), (dict(lam=inf), -4), (dict(sigma=-0.5), -4),
             (dict(sigma=nan), -4), (dict(K=-1), -3), (dict(K=257), -3), (dict(prm=prm.copy(horizon=65)), -2),
             (dict(prm=prm.copy(dt=0.0)), -4), (dict(prm=None), -1), (dict(nprob=-1), -3), (dict(ld=1), -3), (dict(iters=-1), -3),
             (dict(w=nan), -4), (dict(w=-1.0), -4), (dict(U=None), -1), (dict(spheres=None), -1)]
    for kw, want in cases:
        got = status(**kw)
        assert got == want, f"se3mpc_mppi_tracks {kw}: {got} != {want}"
        assert lib.last_error(), f"{kw}: se3mpc_last_error not set"
    assert np.all(h.to_host(Uo) == 0) and np.all(h.to_host(cost) == 0), "a rejected call launched"
    assert status(nprob=0, U=None) == 0 and np.all(h.to_host(Uo) == 0)
    assert status() == 0 and status(stride=0) == 0 and status(Kt=0, tracks=None) == 0 and status(K=0, spheres=None, vel=None) == 0
    assert not np.all(h.to_host(Uo) == 0)
    # ---- se3mpc_mppi_closed_loop_tracks_*
    B = 2
    sc = mv.Scene(h, N, B, K=2, seed=1, vel=mv.velocities(2, 1), t0=0.5)
    st = sc.fresh()
    slab = sc.d(np.ones((1, B, N, Kt, 4)))
    cost = sc.d(np.zeros(B))
    keep = {k: v.clone() for k, v in dict(st, cost=cost).items()}
    ok = dict(prm=sc.prm, cp=sc.cp, sp=sc.sp, B=B, cycles=1, substeps=2, sim_dt=0.01, shift=1, S=64, iters=1, sigma=1.0, lam=1.0, goal=be.ptr(sc.goal_d),
              spheres=be.ptr(sc.sph_d), vel=be.ptr(sc.vel_d), t0=0.5, K=2, w=1.0, wind=be.ptr(sc.wind_d), wstride=3, time=be.ptr(st["time"]),
              pos=be.ptr(st["pos"]), state=be.ptr(st["state"]), U=be.ptr(st["U"]), cost=be.ptr(cost), tracks=be.ptr(slab), Kt=Kt)

    def lstatus(**kw):
        a = dict(ok, **kw)
        return lib.loop_status("mppi_closed_loop_tracks", suf, a["prm"], a["cp"], a["sp"], a["B"], a["cycles"], a["substeps"], a["sim_dt"], 0, a["shift"],
                               a["S"], a["iters"], a["sigma"], a["lam"], 0, 0, 0, a["goal"], a["spheres"], a["vel"], a["t0"], a["K"], a["tracks"], a["Kt"],
                               a["w"], a["wind"], a["wstride"], a["time"], a["pos"], be.ptr(st["vel"]), be.ptr(st["att"]), be.ptr(st["omega"]),
                               a["state"], a["U"], a["cost"], None, None, be.ptr(st["clearance"]), be.stream())

    bad_cp = ControllerParams.from_config(sc.ccfg); bad_cp.mass = 0.0
    bad_sp = SimulatorParams.reference_defaults(mass=-1.0)
    loop_cases = [(dict(vel=None), -1), (dict(t0=nan), -4), (dict(t0=inf), -4), (dict(t0=-inf), -4),
                  (dict(S=0), -3), (dict(S=63), -3), (dict(S=96), -3), (dict(S=65536 + 64), -3), (dict(S=-64), -3), (dict(lam=0.0), -4),
                  (dict(lam=-1.0), -4), (dict(lam=nan), -4), (dict(lam=inf), -4), (dict(sigma=-0.5), -4), (dict(sigma=nan), -4), (dict(sigma=inf), -4),
                  (dict(K=-1), -3), (dict(K=257), -3), (dict(prm=sc.prm.copy(horizon=65)), -2), (dict(prm=sc.prm.copy(dt=0.0)), -4), (dict(prm=None), -1),
                  (dict(cp=None), -1), (dict(sp=None), -1), (dict(cp=bad_cp), -4), (dict(sp=bad_sp), -4), (dict(B=-1), -3), (dict(cycles=-1), -3),
                  (dict(substeps=-1), -3), (dict(iters=-1), -3), (dict(shift=-1), -3), (dict(shift=N + 1), -3), (dict(w=nan), -4), (dict(w=-1.0), -4),
                  (dict(w=inf), -4), (dict(sim_dt=nan), -4), (dict(sim_dt=inf), -4), (dict(wstride=2), -3), (dict(U=None), -1), (dict(spheres=None), -1),
                  (dict(goal=None), -1), (dict(time=None), -1), (dict(pos=None), -1), (dict(state=None), -1), (dict(cost=None), -1)]
    for kw, want in [(dict(Kt=-1), -3), (dict(Kt=17), -3), (dict(K=255, Kt=2), -3), (dict(tracks=None), -1)] + loop_cases:
        got = lstatus(**kw)
        assert got == want, f"se3mpc_mppi_closed_loop_tracks {kw}: {got} != {want}"
        assert lib.last_error(), f"{kw}: se3mpc_last_error not set"
    for k, v in keep.items():
        assert lc.bits_equal(dict(st, cost=cost)[k], v), f"a rejected call launched ({k})"
    assert lstatus(B=0, U=None) == 0 and lstatus(cycles=0, U=None) == 0
    for k, v in keep.items():
        assert lc.bits_equal(dict(st, cost=cost)[k], v), f"B = 0 / cycles = 0 are no-ops ({k})"
    assert lstatus(Kt=0, tracks=None) == 0 and lstatus(K=0, spheres=None, vel=None) == 0 and lstatus(wind=None, wstride=0) == 0
    assert not lc.bits_equal(st["pos"], keep["pos"])
    # ---- se3mpc_swarm_intent_*
    it = sc.d(np.full((B, N, 3), 5.0))
    istat = lambda **kw: (lambda a: lib.loop_status("swarm_intent", suf, a["prm"], a["B"], a["pos"], a["vel"], a["U"], a["intent"], be.stream()))(
        dict(dict(prm=sc.prm, B=B, pos=be.ptr(st["pos"]), vel=be.ptr(st["vel"]), U=be.ptr(st["U"]), intent=be.ptr(it)), **kw))
    for kw, want in [(dict(prm=None), -1), (dict(prm=sc.prm.copy(horizon=65)), -2), (dict(prm=sc.prm.copy(dt=0.0)), -4), (dict(B=-1), -3), (dict(pos=None), -1),
                     (dict(vel=None), -1), (dict(U=None), -1), (dict(intent=None), -1)]:
        got = istat(**kw)
        assert got == want, f"se3mpc_swarm_intent {kw}: {got} != {want}"
        assert lib.last_error(), f"{kw}: se3mpc_last_error not set"
    assert istat(B=0, pos=None) == 0 and np.all(h.to_host(it) == 5.0), "a rejected call launched"
    assert istat() == 0 and not np.any(h.to_host(it) == 5.0)
    # ---- se3mpc_mppi_closed_loop_swarm_intent_*
    for bad in ((-1, N, esz), (4, 0, esz), (4, 65, esz), (4, N, 2), (4, N, 0), (4, N, 16)):
        assert lib.mppi_swarm_intent_workspace_bytes(*bad) == 0, bad
    assert lib.mppi_swarm_intent_workspace_bytes(0, N, esz) == 0 and lib.mppi_swarm_intent_workspace_bytes(6, N, esz) == 12 * (6 + 3 * N) * esz
    M, swarms, Ks, Kn = 3, 2, 2, 2
    B = M * swarms
    sc = sw.Scene(h, N, swarms, M, Ks=Ks, Kn=Kn)
    st = sc.fresh()
    cost = sc.d(np.zeros(B))
    nb = h.to_dev(np.full((B, Kn), 7, np.int32))
    words = 2 * (6 + 3 * N) * B
    ws = sc.d(np.zeros(words))
    keep = {k: v.clone() for k, v in dict(st, cost=cost, nb=nb, ws=ws).items()}
    ok = dict(prm=sc.prm, cp=sc.cp, sp=sc.sp, B=B, M=M, Kn=Kn, radius=0.3, cycles=1, substeps=2, sim_dt=0.01, shift=1, S=64, iters=1, sigma=1.0, lam=1.0,
              goal=be.ptr(sc.goal_d), spheres=be.ptr(sc.sph_d), vel=be.ptr(sc.vel_d), t0=0.5, K=Ks, w=1.0, wind=be.ptr(sc.wind_d), wstride=3,
              time=be.ptr(st["time"]), pos=be.ptr(st["pos"]), state=be.ptr(st["state"]), U=be.ptr(st["U"]), cost=be.ptr(cost),
              sep=be.ptr(st["separation"]), ws=be.ptr(ws), ws_bytes=words * esz)

    def sstatus(**kw):
        a = dict(ok, **kw)
        return lib.loop_status("mppi_closed_loop_swarm_intent", suf, a["prm"], a["cp"], a["sp"], a["B"], a["M"], a["Kn"], a["radius"], a["cycles"],
                               a["substeps"], a["sim_dt"], 0, a["shift"], a["S"], a["iters"], a["sigma"], a["lam"], 0, 0, 0, a["goal"], a["spheres"],
                               a["vel"], a["t0"], a["K"], a["w"], a["wind"], a["wstride"], a["time"], a["pos"], be.ptr(st["vel"]), be.ptr(st["att"]),
                               be.ptr(st["omega"]), a["state"], a["U"], a["cost"], None, None, be.ptr(st["clearance"]), a["sep"], be.ptr(nb), a["ws"],
                               a["ws_bytes"], be.stream())

    own = [(dict(M=0), -3), (dict(M=-1), -3), (dict(M=1025, B=1025), -3), (dict(M=4), -3), (dict(M=5), -3), (dict(Kn=-1), -3), (dict(Kn=17), -3),
           (dict(K=255, Kn=2), -3), (dict(ws_bytes=words * esz - 1), -3), (dict(ws_bytes=12 * B * esz), -3), (dict(ws_bytes=0), -3),
           (dict(radius=-0.1), -4), (dict(radius=nan), -4), (dict(radius=inf), -4), (dict(ws=None), -1), (dict(sep=None), -1)]

    def untouched(what):
        for k, v in keep.items():
            cur = dict(st, cost=cost, nb=nb, ws=ws)[k]
            assert (v is None and cur is None) or lc.bits_equal(cur, v), f"{what} ({k})"

    for kw, want in own + loop_cases:
        got = sstatus(**kw)
        assert got == want, f"se3mpc_mppi_closed_loop_swarm_intent {kw}: {got} != {want}"
        assert lib.last_error(), f"{kw}: se3mpc_last_error not set"
    untouched("a rejected call launched")
    assert sstatus(B=0, U=None) == 0 and sstatus(cycles=0, U=None) == 0
    untouched("B = 0 / cycles = 0 are no-ops")
    assert sstatus(Kn=0, ws=None, ws_bytes=0, sep=None) == 0 and sstatus(M=1, ws=None, ws_bytes=0, sep=None) == 0
    assert sstatus(K=0, spheres=None, vel=None) == 0 and sstatus(wind=None, wstride=0) == 0
    assert not lc.bits_equal(st["pos"], keep["pos"])


# ---- 8. front end ----------------------------------------------------------------------------------------------------------------------
def check_front_end(h, make_planner, N=6, B=3, K=2, Kt=2):
    """SE3MPCPlanner.add_tracked_obstacle through plan_mppi and plan_batch_mppi to the tracks entry: the float64 host resampling (linear,
    held at both ends, rebased to the state's timestamp); clear_obstacles; the ValueErrors; Ops' shape checks; run_mppi_fused(tracks=) and
    run_mppi_swarm(share_plans=True) against Ops."""
    import pytest
    from dart_planner_amd.common.types import DroneState
    prec = "f32" if h.dt == np.float32 else "f64"
    kw = dict(n_samples=64, iters=2, sigma=2.0, temperature=50.0, seed=1, precision=prec, warm_start=False, obstacle_weight=40.0)
    goal = np.array([3.0, 1.0, 2.0])
    pos, velo = np.array([0.0, 0.0, 2.0]), np.zeros(3)
    times = np.array([0.125, 0.25, 0.5])                       # binary fractions: (1.7e9 + t) - 1.7e9 == t
    cen = np.array([[0.2, -1.0, 2.1], [0.3, 0.0, 2.1], [0.3, 0.1, 2.6]])

    def planned(now, shift_t):
        pl = make_planner(N)
        pl.add_obstacle(np.array([5.0, 5.0, 5.0]), 0.3)
        pl.add_moving_obstacle(np.array([4.0, 4.0, 4.0]), 0.4, np.array([0.0, 0.5, 0.0]), now - 0.5)
        pl.add_tracked_obstacle(times + shift_t, cen, 0.5)
        tr = pl.plan_mppi(DroneState(timestamp=now, position=pos, velocity=velo), goal, **kw)
        return pl, tr, dict(pl.last_result)

    pl, tr, r0 = planned(10.0, 10.0)
    assert np.all(np.isfinite(tr.positions)) and r0["penalty"] > 0, r0
    slab = pl._tracked_obstacle_slab(None, 10.0)
    tau = np.arange(N) * 0.1
    want = np.stack([np.interp(tau, times, cen[:, a]) for a in range(3)], axis=1)
    assert slab.shape == (N, 1, 4) and np.allclose(slab[:, 0, :3], want, rtol=0, atol=1e-12) and np.all(slab[:, 0, 3] == 0.5)
    assert np.array_equal(slab[0, 0, :3], cen[0]) and np.array_equal(slab[-1, 0, :3], cen[-1]), "held at both ends"
    assert np.allclose(slab[2, 0, :3], [0.26, -0.4, 2.1], rtol=0, atol=1e-12), "linear in between"
    # the same call made by hand
    ops, prm = pl._get_ops(), pl._params()
    tab = pl._moving_obstacle_table(None, 10.0)
    col = lambda a: ops.be.from_host(np.ascontiguousarray(np.asarray(a, float).reshape(-1, 1).astype(h.dt)))
    dev = lambda a: ops.be.from_host(np.ascontiguousarray(np.asarray(a, float).astype(h.dt)))
    o = ops.mppi_tracks(prm, col(pos), col(velo), col(goal), col(np.tile([0.0, 0.0, pl.hover_thrust], (N, 1))), 64, 2, 2.0, 50.0, dev(slab), seed=1,
                        spheres=dev(tab[:, :4]), obstacle_weight=40.0, sphere_vel=dev(tab[:, 4:]), sphere_t0=0.0)
    assert np.array_equal(np.asarray(ops.be.to_host(o["U"]), float)[:, 0].reshape(N, 3), r0["U"]), "plan_mppi == Ops.mppi_tracks on the resampled slab"
    assert float(np.asarray(ops.be.to_host(o["cost"]), float)[0]) == r0["cost_with_penalty"]
    _, _, r1 = planned(1.7e9, 1.7e9)
    assert np.array_equal(r1["U"], r0["U"]) and r1["cost_with_penalty"] == r0["cost_with_penalty"], "the rebase is done in float64 on the host"
    res = pl.plan_batch_mppi(pos[None], velo[None], goal[None], n_samples=64, iters=2, sigma=2.0, temperature=50.0, seed=1, precision=prec,
                             obstacle_weight=40.0, timestamp=10.0)
    assert np.array_equal(res["thrust_vectors"][0], r0["U"]) and res["cost"][0] == r0["cost_with_penalty"]
    with pytest.raises(ValueError, match="split"):
        pl.plan_mppi(DroneState(timestamp=10.0, position=pos, velocity=velo), goal, splits=1, **kw)
    with pytest.raises(ValueError, match="split"):
        pl.plan_batch_mppi(pos[None], velo[None], goal[None], n_samples=128, iters=1, precision=prec, splits=2, timestamp=10.0)
    with pytest.raises(ValueError, match="rising"):
        pl.add_tracked_obstacle([0.0, 0.0], cen[:2], 0.5)
    only = make_planner(N)                                      # tracked obstacles alone: no moving table at all
    only.add_tracked_obstacle(times + 10.0, cen, 0.5)
    only.plan_mppi(DroneState(timestamp=10.0, position=pos, velocity=velo), goal, **kw)
    assert only.last_result["penalty"] > 0
    pl.clear_obstacles()
    assert pl.obstacles == [] and pl.moving_obstacles == [] and pl.tracked_obstacles == [] and pl._tracked_obstacle_slab(None, 0.0) is None
    # Ops' shape rules
    with pytest.raises(ValueError, match="tracks"):
        ops.mppi_tracks(prm, col(pos), col(velo), col(goal), col(np.zeros((N, 3))), 64, 1, 1.0, 1.0, dev(np.zeros((N, 17, 4))))
    with pytest.raises(ValueError, match="tracks"):
        ops.mppi_tracks(prm, col(pos), col(velo), col(goal), col(np.zeros((N, 3))), 64, 1, 1.0, 1.0, dev(np.zeros((N + 1, 2, 4))))
    # ClosedLoopMonteCarlo
    sc = mv.Scene(h, N, B, K=K, seed=2, vel=mv.velocities(K, 2))
    mcl = sw._monte_carlo(h, sc)
    args = (sc.d(sc.p0), sc.d(sc.v0), sc.goal_d, 3, 10, 0.01, 64, 2, 1.0, 50.0)
    mkw = dict(seed=9, spheres=sc.sph_d, obstacle_weight=40.0, wind=sc.wind_d, sphere_velocities=sc.vel_d, sphere_t0=0.7, nominal=sc.d(sc.U0))
    rng = np.random.default_rng(3)
    slab = sc.d(np.concatenate([np.broadcast_to(sc.p0[None, :, None, None, :], (3, B, N, Kt, 3)) + rng.uniform(-0.5, 0.5, (3, B, N, Kt, 3)),
                                np.full((3, B, N, Kt, 1), 0.4)], axis=-1))
    a = mcl.run_mppi_fused(*args, log=True, **mkw, tracks=slab)
    none = mcl.run_mppi_fused(*args, log=True, **mkw)
    empty = mcl.run_mppi_fused(*args, log=True, **mkw, tracks=sc.d(np.zeros((3, B, N, 0, 4))))
    for k in ("pos", "vel", "att", "omega", "time", "controller_state", "U", "cost", "trace", "clearance"):
        assert lc.bits_equal(none[k], empty[k]), k
    assert not lc.bits_equal(a["U"], none["U"]), "the tracks reach the kernel"
    st = sc.fresh()
    sc.call(st, 3, 10, 0.01, mcl.resolve_shift(10, 0.01, None), seed=9, sphere_t0=0.7, tracks=slab, obstacle_weight=40.0)
    assert lc.bits_equal(a["pos"], st["pos"]) and lc.bits_equal(a["clearance"], st["clearance"]), "run_mppi_fused(tracks=) == Ops"
    with pytest.raises(ValueError, match="tracks"):
        mcl.run_mppi_fused(*args, **mkw, tracks=slab[:2].contiguous())
    ss = sw.Scene(h, N, 2, 3, Ks=K, Kn=2)
    mcl = sw._monte_carlo(h, ss)
    args = (ss.d(ss.p0), ss.d(ss.v0), ss.goal_d, 2, 3, 0.01, 64, 2, 1.0, 50.0)
    skw = dict(seed=9, spheres=ss.sph_d, obstacle_weight=40.0, wind=ss.wind_d, sphere_velocities=ss.vel_d, sphere_t0=0.7, swarm_size=3, neighbours=2,
               mate_radius=0.3, want_neighbours=True, nominal=ss.d(ss.U0))
    shared, plain = mcl.run_mppi_swarm(*args, **skw, share_plans=True), mcl.run_mppi_swarm(*args, **skw)
    assert tuple(shared["neighbours"].shape) == (6, 2) and tuple(shared["separation"].shape) == (6,)
    assert not lc.bits_equal(shared["U"], plain["U"]), "share_plans reaches the kernel"
    st = ss.fresh()
    ss.swarm(st, 2, 3, 0.01, mcl.resolve_shift(3, 0.01, None), seed=9, sphere_t0=0.7, obstacle_weight=40.0, share_plans=True)
    assert lc.bits_equal(shared["pos"], st["pos"]) and lc.bits_equal(shared["U"], st["U"]), "run_mppi_swarm(share_plans=True) == Ops"
    with pytest.raises(Exception, match="SE3MPC_ERR_SHAPE"):
        mcl.run_mppi_swarm(*args, **dict(skw, neighbours=17), share_plans=True)


# ---- 9. behaviour ----------------------------------------------------------------------------------------------------------------------
SEEDS = tuple(range(8))                # fixed before anything was measured


def behaviour_runs(h, seeds=SEEDS):
    """The head-on scene of mppi_swarm_checks.check_behaviour over `seeds`, with and without shared plans -> {share_plans: separations
    (len(seeds),)}, the smaller of the two drones' per run."""
    kw = sw.BEHAVIOUR
    res = {False: [], True: []}
    for seed in seeds:
        for share in (False, True):
            sc = sw.Scene(h, kw["N"], 1, 2, Ks=0, Kn=1, mate_radius=kw["mate_radius"], w_obs=kw["w_obs"], S=kw["S"], iters=kw["iters"],
                          sigma=kw["sigma"], lam=kw["lam"], wind=None, seed=seed, t0=0.0, **sw.behaviour_scene())
            out = sw._monte_carlo(h, sc).run_mppi_swarm(sc.d(sc.p0), sc.d(sc.v0), sc.goal_d, kw["cycles"], kw["substeps"], kw["sim_dt"], kw["S"],
                                                        kw["iters"], kw["sigma"], kw["lam"], seed=seed, obstacle_weight=kw["w_obs"], shift=kw["shift"],
                                                        swarm_size=2, neighbours=1, mate_radius=kw["mate_radius"], share_plans=share)
            res[share].append(float(np.min(h.to_host(out["separation"]).astype(float))))
    return {k: np.array(v) for k, v in res.items()}


def check_behaviour(h):
    """Over seeds 0-7: the number of runs whose separation stays at or above mate_radius with shared plans is not below the number without
    (the parent's mode is the yardstick).  The table is DESIGN.md 5.8h's."""
    res = behaviour_runs(h)
    r = sw.BEHAVIOUR["mate_radius"]
    for seed, a, b in zip(SEEDS, res[False], res[True]):
        print(f"seed {seed}: separation {a:.3f} m extrapolated, {b:.3f} m with shared plans")
    ok = {k: int(np.sum(v >= r)) for k, v in res.items()}
    print(f"runs that keep mate_radius = {r} m: {ok[False]} of {len(SEEDS)} extrapolated, {ok[True]} of {len(SEEDS)} with shared plans")
    assert ok[True] >= ok[False], ok
