"""Checks of the swarm MPPI closed loop (se3mpc_mppi_closed_loop_swarm_*, se3mpc_swarm_separation_*, Ops.mppi_closed_loop_swarm /
swarm_separation, ClosedLoopMonteCarlo.run_mppi_swarm) shared by the host-emulation suite (tests/test_emu_mppi_swarm.py) and the MI355X
suite (tests/test_gpu_mppi_swarm.py).  Every check takes a parity_checks.Harness whose arrays are torch tensors.

Bounds: none new.  The kernel is pinned bit for bit to se3mpc_mppi_closed_loop_moving_* (one call over all drones where no mate enters a
table; one call per drone and cycle on the table tests/swarm_oracle.py builds where mates do); selection and separation are exact against
that oracle (float64 d2 on the rounded values); the clearance is held to mppi_moving_checks.CLEARANCE_ABS."""
import functools
import json
import os

import numpy as np

import mppi_closed_loop_checks as lc
import mppi_moving_checks as mv
import mppi_moving_oracle as mvo
import swarm_oracle as so
from dart_planner_amd.capi import ControllerParams, Params, SimulatorParams
from oracle import controller_oracle as co

OUT_KEYS = ("cost", "trace", "plan_last")
TIE_REL = 1e-3                         # the chain check wants every drone's mate distances further apart than this, relatively


class Scene(mv.Scene):
    """mppi_moving_checks.Scene of swarms x M drones: Ks shared moving spheres, Kn mates per table, a separation per drone."""

    def __init__(self, h, N, swarms, M, Ks=0, Kn=0, mate_radius=0.3, w_obs=40.0, seed=5, **kw):
        kw.setdefault("vel", mv.velocities(Ks, seed))
        kw.setdefault("t0", mv.T0)
        super().__init__(h, N, swarms * M, K=Ks, w_obs=w_obs, seed=seed, **kw)
        self.w_obs = w_obs                                   # the mates are penalised with no shared sphere too
        self.M, self.Kn, self.mate_radius = M, Kn, mate_radius

    def fresh(self, *a, **kw):
        st = super().fresh(*a, **kw)
        st["separation"] = self.d(np.full(len(self.h.to_host(st["pos"])), np.inf))
        return st

    def swarm(self, st, cycles, substeps, sim_dt, shift, cycle_base=0, iter_base=0, **kw):
        """One se3mpc_mppi_closed_loop_swarm_* call on every drone of the scene, in place on st."""
        a = dict(swarm_size=self.M, neighbours=self.Kn, mate_radius=self.mate_radius, seed=self.seed, cycle_base=cycle_base, shift=shift,
                 iter_base=iter_base, spheres=self.sph_d, obstacle_weight=self.w_obs, wind=self.wind_d, want_plan=True, clearance=st["clearance"],
                 sphere_vel=self.vel_d if self.K else None, sphere_t0=self.t0, separation=st["separation"], want_neighbours=True)
        a.update(kw)
        return self.h.ops.mppi_closed_loop_swarm(self.prm, self.cp, self.sp, st["state"], st["time"], st["pos"], st["vel"], st["att"], st["omega"],
                                                 self.goal_d, st["U"], cycles, substeps, sim_dt, self.S, self.iters, self.sigma, self.lam, **a)


def _same(a, b, what, keys):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        assert lc.bits_equal(a[k], b[k]), f"{what}: {k}"


def _host(h, st):
    return h.to_host(st["pos"]).copy(), h.to_host(st["vel"]).copy()


# ---- 1. no mates in the table: the moving loop -----------------------------------------------------------------------------------------
def check_reduces_to_moving(h, N, S, swarms, M, Kn, Ks, cycles=2, substeps=3, sim_dt=0.01, shift=1, seed=5):
    """swarm_size = 1 (any neighbours_k) and neighbours_k = 0 (any swarm_size): state, U, cost, trace, plan_last and clearance of ONE
    se3mpc_mppi_closed_loop_moving_* call with the same cycles, bit for bit."""
    assert M == 1 or Kn == 0
    sc = Scene(h, N, swarms, M, Ks=Ks, Kn=Kn, S=S, seed=seed)
    a, b = sc.fresh(), sc.fresh()
    oa = sc.call(a, cycles, substeps, sim_dt, shift, iter_base=7)
    ob = sc.swarm(b, cycles, substeps, sim_dt, shift, iter_base=7)
    lc.same_bits(a, b, f"M = {M}, Kn = {Kn} vs the moving loop")
    _same(oa, ob, "vs the moving loop", OUT_KEYS)
    if Kn:
        assert np.all(h.to_host(ob["neighbours"]) == -1), "a drone alone has no neighbours"


# ---- 2. mates in the table: the per-drone chain of the moving entry --------------------------------------------------------------------
def spread_positions(n, seed, lo=0.1, box=1.5):
    """n positions in a box of +-`box` m around (0, 0, 2), float32-exact, placed one after another so that for every drone no two of its
    distances to the others agree to TIE_REL relatively (nor any pair is nearer than `lo`)."""
    rng = np.random.default_rng(seed)
    tol = 1.1 * TIE_REL
    P = (rng.uniform(-box, box, (1, 3)) + [0, 0, 2]).astype(np.float32).astype(float)
    D = np.zeros((1, 1))
    while len(P) < n:
        k = len(P)
        X = (rng.uniform(-box, box, (256, 3)) + [0, 0, 2]).astype(np.float32).astype(float)          # candidates, judged together
        d = np.linalg.norm(P[None] - X[:, None], axis=2)                                              # (256, k)
        ok = d.min(axis=1) >= lo
        if k > 1:
            s = np.sort(d, axis=1)
            ok &= np.min(np.diff(s, axis=1) / s[:, 1:], axis=1) > tol                                 # the newcomer's own distances
            rel = np.abs(D[None] - d[:, :, None]) / np.maximum(D[None], d[:, :, None])                # drone i: its old distances vs the new one
            rel[:, np.arange(k), np.arange(k)] = 1.0
            ok &= rel.min(axis=(1, 2)) > tol
        if not ok.any():
            continue
        c = int(np.argmax(ok))
        D = np.block([[D, d[c][:, None]], [d[c][None, :], np.zeros((1, 1))]])
        P = np.vstack([P, X[c]])
    return P


GOLDEN_70 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swarm_positions_70.json")


@functools.lru_cache(maxsize=None)
def _spread(n, seed):
    """spread_positions(n, seed); the 70 of one large swarm take half a minute to place, so they are a fixture (spread_positions(70, 5)) --
    assert_no_ties checks either."""
    if n > 16:
        with open(GOLDEN_70) as f:
            return np.array(json.load(f)["positions"])[:n]
    return spread_positions(n, seed)


def assert_no_ties(pos, M):
    for b in range(len(pos)):
        base = (b // M) * M
        d = np.sqrt(np.delete(so.d2_row(pos, b, M), b - base))
        s = np.sort(d)
        if len(s) > 1:
            assert np.min(np.diff(s) / s[1:]) > TIE_REL, f"drone {b}: two mates at nearly one distance"


def chain(sc, st, cycles, substeps, sim_dt, shift, iter_base=0):
    """`cycles` cycles of every drone through se3mpc_mppi_closed_loop_moving_* alone: per cycle the host takes (pos, vel), builds every drone's
    table with swarm_oracle and calls the moving entry on that drone with B = 1, index_base = b, cycle_base = C, cycles = 1, K = Ks + Kn_eff,
    clearance = NULL.  -> dict(cost, trace, plan_last) as one call would return them, starts = [(pos, vel)] at every cycle's start."""
    import torch
    h, B = sc.h, sc.B
    starts, traces = [], []
    for C in range(cycles):
        pos, vel = _host(h, st)
        starts.append((pos, vel))
        tR0 = so.cycle_time(sc.t0, C, substeps, sim_dt, h.dt)
        outs = []
        for b in range(B):
            who, _ = so.ranked(pos, vel, b, sc.M)
            ms, mvel = so.mate_rows(pos, vel, who[:sc.Kn], tR0, sc.mate_radius, h.dt)
            sph = np.concatenate([sc.sph.reshape(-1, 4).astype(h.dt), ms])
            v = np.concatenate([sc.vel.reshape(-1, 3).astype(h.dt), mvel])
            sub = {k: st[k][b:b + 1] for k in lc.STATE_KEYS}
            sub["clearance"] = None
            outs.append(sc.call(sub, 1, substeps, sim_dt, shift, cycle_base=C, lo=b, hi=b + 1, iter_base=iter_base,
                                spheres=h.to_dev(np.ascontiguousarray(sph)) if len(sph) else None, sphere_vel=h.to_dev(np.ascontiguousarray(v)),
                                obstacle_weight=sc.w_obs, clearance=None, want_clearance=False))
        traces.append(torch.cat([o["trace"] for o in outs], dim=0))
    return dict(cost=torch.cat([o["cost"] for o in outs]), trace=torch.cat(traces, dim=1), plan_last=torch.cat([o["plan_last"] for o in outs], dim=0),
                starts=starts)


def check_chain(h, N, S, swarms, M, Kn, Ks, cycles=2, substeps=3, sim_dt=0.01, shift=1, seed=5, mates_matter=True, **scene_kw):
    """The main check: one swarm call == the per-drone chain of se3mpc_mppi_closed_loop_moving_* on swarm_oracle's tables, bit for bit on
    state, U, cost, trace and plan_last; the last cycle's neighbours and the separation (the cycle starts) equal the oracle's exactly."""
    p0 = np.concatenate([_spread(M, seed + s) for s in range(swarms)])
    sc = Scene(h, N, swarms, M, Ks=Ks, Kn=Kn, S=S, seed=seed, p0=p0, **scene_kw)
    assert_no_ties(sc.p0, M)
    a, b = sc.fresh(), sc.fresh()
    ref = chain(sc, a, cycles, substeps, sim_dt, shift, iter_base=7)
    out = sc.swarm(b, cycles, substeps, sim_dt, shift, iter_base=7)
    _same(a, b, "swarm call vs the per-drone chain", lc.STATE_KEYS)
    _same(ref, out, "swarm call vs the per-drone chain", OUT_KEYS)
    pos, vel = ref["starts"][-1]
    assert np.array_equal(h.to_host(out["neighbours"]), so.neighbours(pos, vel, M, Kn)), "neighbours of the last cycle"
    want = None
    for pos, vel in ref["starts"]:
        want = so.separation(pos, vel, M, h.dt, want)
    assert np.array_equal(h.to_host(b["separation"]), want), "separation = min over the cycle starts"
    # the mates must matter: the same drones without them plan something else (one cycle shows it)
    if not mates_matter:
        return
    alone, mated = sc.fresh(), sc.fresh()
    sc.swarm(alone, 1, 0, sim_dt, shift, iter_base=7, neighbours=0)
    sc.swarm(mated, 1, 0, sim_dt, shift, iter_base=7)
    assert not lc.bits_equal(alone["U"], mated["U"]), "the mates' rows must reach the planner"


# ---- 3. selection ----------------------------------------------------------------------------------------------------------------------
def check_selection(h, N=6, S=64):
    """neighbours == swarm_oracle.neighbours exactly: an exact tie (mates at own +- (1, 0, 0)) goes to the lower index; Kn > E leaves -1
    behind; a drone whose snapshot holds a NaN is in nobody's table, its mates stay finite and every other swarm keeps its bytes."""
    # an exact tie, seen from the drone in the middle (index 1) and from one whose tied mates are 1 and 2 (index 0 of the second swarm)
    own = np.array([0.25, -0.5, 2.0])
    p0 = np.array([own + [1, 0, 0], own, own - [1, 0, 0], own, own + [0, 1, 0], own - [0, 1, 0]])
    sc = Scene(h, N, 2, 3, Kn=1, S=S, p0=p0)
    st = sc.fresh()
    nb = h.to_host(sc.swarm(st, 1, 2, 0.01, 1)["neighbours"])
    assert nb[1, 0] == 0 and nb[3, 0] == 4, f"equal d2 resolves to the lower index: {nb.ravel()}"
    assert np.array_equal(nb, so.neighbours(sc.p0, sc.v0, 3, 1))
    # Kn > E
    sc = Scene(h, N, 2, 5, Kn=8, Ks=2, S=S)
    st = sc.fresh()
    nb = h.to_host(sc.swarm(st, 1, 2, 0.01, 1)["neighbours"])
    assert nb.shape == (10, 8) and np.all(nb[:, 4:] == -1) and np.all(nb[:, :4] >= 0)
    assert np.array_equal(nb, so.neighbours(sc.p0, sc.v0, 5, 8))
    # a NaN drone in the middle swarm
    M, bad = 5, 6
    clean = Scene(h, N, 3, M, Kn=3, Ks=2, S=S)
    p0 = clean.p0.copy(); p0[bad, 1] = np.nan
    dirty = Scene(h, N, 3, M, Kn=3, Ks=2, S=S, p0=p0)
    a, b = clean.fresh(), dirty.fresh()
    oa, ob = clean.swarm(a, 2, 3, 0.01, 1), dirty.swarm(b, 2, 3, 0.01, 1)
    nb = h.to_host(ob["neighbours"])
    assert not np.any(nb == bad), "a drone with a NaN snapshot is in nobody's table"
    assert np.all(nb[bad] == -1), "... and has no eligible mate itself"
    mates = [i for i in range(M, 2 * M) if i != bad]
    assert np.all(nb[mates, :3] >= 0) and np.all(nb[mates][:, :3] // M == 1)
    import torch
    for k in ("pos", "vel", "U", "clearance", "separation"):
        assert torch.isfinite(b[k][mates]).all(), f"mates of the NaN drone: {k}"
    assert torch.isfinite(ob["cost"][mates]).all()
    others = list(range(M)) + list(range(2 * M, 3 * M))
    for k in lc.STATE_KEYS + ("clearance", "separation"):
        assert lc.bits_equal(a[k][others], b[k][others]), f"the other swarms keep their bytes: {k}"
    for k in OUT_KEYS + ("neighbours",):
        assert lc.bits_equal(oa[k][others], ob[k][others]), f"the other swarms keep their bytes: {k}"


# ---- 4. separation ---------------------------------------------------------------------------------------------------------------------
def check_separation_entry(h, M, swarms=2, seed=3):
    """se3mpc_swarm_separation_* against NumPy on random positions (one drone not finite, one running value already smaller)."""
    rng = np.random.default_rng(seed)
    B = swarms * M
    pos = rng.uniform(-3, 3, (B, 3)).astype(h.dt)
    vel = rng.normal(0, 1, (B, 3)).astype(h.dt)
    vel[B - 1, 2] = np.inf
    run = np.full(B, np.inf, h.dt)
    run[0] = 1e-3
    got = h.ops.swarm_separation(h.to_dev(pos), h.to_dev(vel), M, separation=h.to_dev(run.copy()))
    want = so.separation(pos, vel, M, h.dt, run)
    assert np.array_equal(h.to_host(got), want), np.max(np.abs(h.to_host(got) - want))
    assert want[0] == h.dt(1e-3) and np.isinf(want[B - 1]) and np.all(np.isfinite(want[:M]))
    fresh = h.to_host(h.ops.swarm_separation(h.to_dev(pos), h.to_dev(vel), M))
    assert np.array_equal(fresh, so.separation(pos, vel, M, h.dt))
    alone = h.to_host(h.ops.swarm_separation(h.to_dev(pos), h.to_dev(vel), 1))
    assert np.all(np.isinf(alone)), "a swarm of one has no separation"


def _monte_carlo(h, sc):
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    return ClosedLoopMonteCarlo(h.ops, sc.prm, controller=sc.cp, simulator=sc.sp)


def check_separation_of_a_run(h, N=6, S=64, swarms=2, M=5, Kn=3, Ks=2, cycles=3, substeps=3, sim_dt=0.01):
    """run_mppi_swarm's separation == the minimum, over the cycle starts and the final state of a chained cycles = 1 run, of the pairwise
    (R)sqrt(float64 d2) recomputed in NumPy -- exactly; the run's state equals the chain's."""
    sc = Scene(h, N, swarms, M, Ks=Ks, Kn=Kn, S=S)
    res = _monte_carlo(h, sc).run_mppi_swarm(sc.d(sc.p0), sc.d(sc.v0), sc.goal_d, cycles, substeps, sim_dt, S, sc.iters, sc.sigma, sc.lam, seed=sc.seed,
                                             spheres=sc.sph_d, obstacle_weight=sc.w_obs, wind=sc.wind_d, shift=1, nominal=sc.d(sc.U0),
                                             sphere_velocities=sc.vel_d, sphere_t0=sc.t0, swarm_size=M, neighbours=Kn, mate_radius=sc.mate_radius)
    st = sc.fresh()
    want = None
    for C in range(cycles):
        want = so.separation(*_host(h, st), M, h.dt, want)
        sc.swarm(st, 1, substeps, sim_dt, 1, cycle_base=C)
    want = so.separation(*_host(h, st), M, h.dt, want)
    for k in ("pos", "vel", "U"):
        assert lc.bits_equal(res[k], st[k]), k
    got = h.to_host(res["separation"])
    assert np.array_equal(got, want), f"{got} vs {want}"
    assert np.all(np.isfinite(got)) and np.all(got > 0)


# ---- 5. clearance ----------------------------------------------------------------------------------------------------------------------
def check_clearance(h, N, swarms=2, M=5, Kn=3, Ks=2, S=64, cycles=6, sim_dt=0.02, seed=8):
    """mppi_moving_checks.check_clearance on the swarm entry: chained calls of one cycle of one simulator step return every position, and the
    oracle's minimum of |pos - centre| - r over the SHARED rows alone meets `clearance` to CLEARANCE_ABS; the one-launch-per-cycle run
    equals the chain bit for bit."""
    sc = Scene(h, N, swarms, M, Ks=Ks, Kn=Kn, S=S, seed=seed)
    st = sc.fresh()
    visited = []
    for c in range(cycles):
        sc.swarm(st, 1, 1, sim_dt, 0, cycle_base=c, iter_base=3)
        visited.append(h.to_host(st["pos"]).astype(float).copy())
    tau = sc.t0 + (np.arange(cycles) + 1.0) * sim_dt
    want = mvo.clearance(np.stack(visited), tau, sc.sph, sc.vel, h.dt)
    got = h.to_host(st["clearance"]).astype(float)
    err = float(np.max(np.abs(got - want)))
    print(f"clearance {got} vs oracle {want}: max abs err {err:.3e} (bound {mv.CLEARANCE_ABS[h.dt]:.0e})")
    assert err <= mv.CLEARANCE_ABS[h.dt], err
    one = sc.fresh()
    sc.swarm(one, cycles, 1, sim_dt, 0, iter_base=3)
    _same(one, st, "one call vs the chain", lc.STATE_KEYS + ("clearance", "separation"))


# ---- 6. continuation and determinism ---------------------------------------------------------------------------------------------------
def check_continuation_and_determinism(h, N=6, S=64, swarms=2, M=5, Kn=3, Ks=2, cycles=3, substeps=3, sim_dt=0.01, shift=1):
    """cycles = 3 in one call == three chained calls (separation and the last neighbours included); two runs give the same bytes; a workspace
    larger than required and full of NaN, and outputs full of NaN, give the same bytes."""
    sc = Scene(h, N, swarms, M, Ks=Ks, Kn=Kn, S=S)
    B = sc.B
    keys = lc.STATE_KEYS + ("clearance", "separation")
    one = sc.fresh()
    o1 = sc.swarm(one, cycles, substeps, sim_dt, shift, iter_base=7)
    many = sc.fresh()
    for c in range(cycles):
        oc = sc.swarm(many, 1, substeps, sim_dt, shift, cycle_base=c, iter_base=7)
        assert lc.bits_equal(oc["trace"][:, 0], o1["trace"][:, c]), f"trace of cycle {c}"
    _same(one, many, "cycles = C vs C calls", keys)
    _same(o1, oc, "cycles = C vs C calls", ("cost", "plan_last", "neighbours"))
    again = sc.fresh()
    o2 = sc.swarm(again, cycles, substeps, sim_dt, shift, iter_base=7)
    _same(one, again, "run to run", keys)
    _same(o1, o2, "run to run", OUT_KEYS + ("neighbours",))
    # garbage everywhere the call only writes, a workspace with room to spare
    import torch
    suf = "f32" if h.dt == np.float32 else "f64"
    be, esz = h.ops.be, np.dtype(h.dt).itemsize
    need = h.ops.lib.mppi_swarm_workspace_bytes(B, esz)
    assert need == 2 * 6 * B * esz
    ws = sc.d(np.full(need // esz + 7, np.nan))
    d = sc.fresh()
    trace = sc.d(np.full((B, cycles, sc.iters), np.nan)); plan = sc.d(np.full((B, 3, N, 3), np.nan)); cost = sc.d(np.full(B, np.nan))
    nb = h.to_dev(np.full((B, Kn), 0x7FC00000, np.int32))
    h.ops.lib.loop_call("mppi_closed_loop_swarm", suf, sc.prm, sc.cp, sc.sp, B, M, Kn, sc.mate_radius, cycles, substeps, sim_dt, 0, shift, S, sc.iters,
                        sc.sigma, sc.lam, sc.seed, 7, 0, be.ptr(sc.goal_d), be.ptr(sc.sph_d), be.ptr(sc.vel_d), sc.t0, Ks, sc.w_obs, be.ptr(sc.wind_d), 3,
                        be.ptr(d["time"]), be.ptr(d["pos"]), be.ptr(d["vel"]), be.ptr(d["att"]), be.ptr(d["omega"]), be.ptr(d["state"]), be.ptr(d["U"]),
                        be.ptr(cost), be.ptr(trace), be.ptr(plan), be.ptr(d["clearance"]), be.ptr(d["separation"]), be.ptr(nb), be.ptr(ws),
                        int(ws.numel()) * esz, be.stream())
    _same(one, d, "dirty buffers", keys)
    assert lc.bits_equal(trace, o1["trace"]) and lc.bits_equal(plan, o1["plan_last"]) and lc.bits_equal(cost, o1["cost"])
    assert torch.equal(nb, o1["neighbours"])


# ---- 7. behaviour ----------------------------------------------------------------------------------------------------------------------
BEHAVIOUR = dict(N=10, S=64, iters=2, sigma=3.0, lam=50.0, cycles=8, substeps=10, sim_dt=0.01, shift=1, w_obs=2000.0, mate_radius=0.5,
                 half=1.0, speed=2.0, seed=1)


def behaviour_scene():
    """Two drones swap places head-on: 2 m apart at 3 m altitude, each one's goal the other's start, each flying at its goal at 2 m/s, so
    they meet 0.5 s into the 1.2 s run, at the start of cycle 5.  (This simulator's thrust acts along world z -- mppi_closed_loop_checks.
    behaviour_scene -- so the crossing is carried by the initial velocities and a drone can only dodge up or down.)"""
    kw = BEHAVIOUR
    prm = Params.reference_defaults(horizon=kw["N"], dt=0.1, mass=1.0, gravity=9.80665, max_thrust=20.0, max_tilt_angle=0.02)
    p0 = np.array([[-kw["half"], 0.0, 3.0], [kw["half"], 0.0, 3.0]])
    v0 = np.array([[kw["speed"], 0.0, 0.0], [-kw["speed"], 0.0, 0.0]])
    return dict(prm=prm, ccfg=co.ControllerConfig(), sim=co.SimulatorConfig(mass=1.0, gravity=9.80665),
                sp=SimulatorParams.reference_defaults(mass=1.0, gravity=9.80665), p0=p0, v0=v0, goal=p0[::-1].copy(),
                U=np.tile([0.0, 0.0, prm.mass * prm.gravity], (2, kw["N"], 1)))


def check_behaviour(h):
    """Two drones swap places head-on at one altitude (behaviour_scene), one swarm of M = 2, mate_radius 0.5 m.  With neighbours_k = 0 they
    fly through each other: the run's separation falls below mate_radius; with neighbours_k = 1 and obstacle_weight = 2000 it stays above.
    Both with more than 20 % margin (< 0.4 m, > 0.6 m).  Measured, float64 and float32 alike to three digits, emulation and MI355X: 0.033 m
    without the mate, 0.960 m with it (one drone climbs to 4.9 m, the other sinks to 2.6 m).  The scene is symmetric: which way a drone dodges
    is its noise's choice, and of six seeds tried two send both the same way; the seed is one that parts them."""
    kw = BEHAVIOUR
    res = {}
    for Kn in (0, 1):
        sc = Scene(h, kw["N"], 1, 2, Ks=0, Kn=Kn, mate_radius=kw["mate_radius"], w_obs=kw["w_obs"], S=kw["S"], iters=kw["iters"], sigma=kw["sigma"],
                   lam=kw["lam"], wind=None, seed=kw["seed"], t0=0.0, **behaviour_scene())
        out = _monte_carlo(h, sc).run_mppi_swarm(sc.d(sc.p0), sc.d(sc.v0), sc.goal_d, kw["cycles"], kw["substeps"], kw["sim_dt"], kw["S"], kw["iters"],
                                                 kw["sigma"], kw["lam"], seed=kw["seed"], obstacle_weight=kw["w_obs"], shift=kw["shift"], swarm_size=2,
                                                 neighbours=Kn, mate_radius=kw["mate_radius"])
        res[Kn] = h.to_host(out["separation"]).astype(float)
        print(f"neighbours_k {Kn}: separation {res[Kn]}, final position {h.to_host(out['pos'])}")
    r = kw["mate_radius"]
    assert np.all(res[0] < 0.8 * r), f"without mates in the table the drones fly through each other: {res[0]}"
    assert np.all(res[1] > 1.2 * r), f"with the mate in the table they keep apart: {res[1]}"


# ---- 8. invalid arguments --------------------------------------------------------------------------------------------------------------
def check_invalid_arguments(h, N=6):
    """Every rule of the header: the code, se3mpc_last_error set, no output touched."""
    nan, inf = float("nan"), float("inf")
    suf = "f32" if h.dt == np.float32 else "f64"
    be, lib = h.ops.be, h.ops.lib
    esz = np.dtype(h.dt).itemsize
    for bad in ((-1, esz), (4, 2), (4, 0), (4, 16)):
        assert lib.mppi_swarm_workspace_bytes(*bad) == 0, bad
    assert lib.mppi_swarm_workspace_bytes(0, esz) == 0 and lib.mppi_swarm_workspace_bytes(6, esz) == 72 * esz
    M, swarms, Ks, Kn = 3, 2, 2, 2
    B = M * swarms
    sc = Scene(h, N, swarms, M, Ks=Ks, Kn=Kn)
    st = sc.fresh()
    cost = sc.d(np.zeros(B))
    nb = h.to_dev(np.full((B, Kn), 7, np.int32))
    ws = sc.d(np.zeros(12 * B))
    keep = {k: v.clone() for k, v in dict(st, cost=cost, nb=nb, ws=ws).items()}
    ok = dict(prm=sc.prm, cp=sc.cp, sp=sc.sp, B=B, M=M, Kn=Kn, radius=0.3, cycles=1, substeps=2, sim_dt=0.01, shift=1, S=64, iters=1, sigma=1.0, lam=1.0,
              goal=be.ptr(sc.goal_d), spheres=be.ptr(sc.sph_d), vel=be.ptr(sc.vel_d), t0=0.5, K=Ks, w=1.0, wind=be.ptr(sc.wind_d), wstride=3,
              time=be.ptr(st["time"]), pos=be.ptr(st["pos"]), state=be.ptr(st["state"]), U=be.ptr(st["U"]), cost=be.ptr(cost),
              sep=be.ptr(st["separation"]), ws=be.ptr(ws), ws_bytes=12 * B * esz)

    def status(**kw):
        a = dict(ok, **kw)
        return lib.loop_status("mppi_closed_loop_swarm", suf, a["prm"], a["cp"], a["sp"], a["B"], a["M"], a["Kn"], a["radius"], a["cycles"], a["substeps"],
                               a["sim_dt"], 0, a["shift"], a["S"], a["iters"], a["sigma"], a["lam"], 0, 0, 0, a["goal"], a["spheres"], a["vel"], a["t0"],
                               a["K"], a["w"], a["wind"], a["wstride"], a["time"], a["pos"], be.ptr(st["vel"]), be.ptr(st["att"]), be.ptr(st["omega"]),
                               a["state"], a["U"], a["cost"], None, None, be.ptr(st["clearance"]), a["sep"], be.ptr(nb), a["ws"], a["ws_bytes"],
                               be.stream())

    bad_cp = ControllerParams.from_config(sc.ccfg); bad_cp.mass = 0.0
    bad_sp = SimulatorParams.reference_defaults(mass=-1.0)
    cases = [  # the swarm's own
             (dict(M=0), -3), (dict(M=-1), -3), (dict(M=1025, B=1025), -3), (dict(M=4), -3), (dict(M=5), -3), (dict(Kn=-1), -3),
             (dict(Kn=255), -3), (dict(K=256, Kn=1), -3), (dict(ws_bytes=12 * B * esz - 1), -3), (dict(ws_bytes=0), -3),
             (dict(radius=-0.1), -4), (dict(radius=nan), -4), (dict(radius=inf), -4), (dict(ws=None), -1), (dict(sep=None), -1),
             # those of se3mpc_mppi_closed_loop_moving_*
             (dict(vel=None), -1), (dict(t0=nan), -4), (dict(t0=inf), -4), (dict(t0=-inf), -4),
             (dict(S=0), -3), (dict(S=63), -3), (dict(S=96), -3), (dict(S=65536 + 64), -3), (dict(S=-64), -3), (dict(lam=0.0), -4),
             (dict(lam=-1.0), -4), (dict(lam=nan), -4), (dict(lam=inf), -4), (dict(sigma=-0.5), -4), (dict(sigma=nan), -4), (dict(sigma=inf), -4),
             (dict(K=-1), -3), (dict(K=257), -3), (dict(prm=sc.prm.copy(horizon=65)), -2), (dict(prm=sc.prm.copy(dt=0.0)), -4), (dict(prm=None), -1),
             (dict(cp=None), -1), (dict(sp=None), -1), (dict(cp=bad_cp), -4), (dict(sp=bad_sp), -4), (dict(B=-3), -3), (dict(cycles=-1), -3),
             (dict(substeps=-1), -3), (dict(iters=-1), -3), (dict(shift=-1), -3), (dict(shift=N + 1), -3), (dict(w=nan), -4), (dict(w=-1.0), -4),
             (dict(w=inf), -4), (dict(sim_dt=nan), -4), (dict(sim_dt=inf), -4), (dict(wstride=2), -3), (dict(U=None), -1), (dict(spheres=None), -1),
             (dict(goal=None), -1), (dict(time=None), -1), (dict(pos=None), -1), (dict(state=None), -1), (dict(cost=None), -1)]

    def untouched(what):
        for k, v in keep.items():
            cur = dict(st, cost=cost, nb=nb, ws=ws)[k]
            assert (v is None and cur is None) or lc.bits_equal(cur, v), f"{what} ({k})"

    for kw, want in cases:
        got = status(**kw)
        assert got == want, f"se3mpc_mppi_closed_loop_swarm {kw}: {got} != {want}"
        assert lib.last_error(), f"{kw}: se3mpc_last_error not set"
    untouched("a rejected call launched")
    assert status(B=0, U=None) == 0 and status(cycles=0, U=None) == 0
    untouched("B = 0 / cycles = 0 are no-ops")
    # what the rules allow: no workspace / separation without mates in the table, a swarm of one, no shared rows
    assert status(Kn=0, ws=None, ws_bytes=0, sep=None) == 0 and status(M=1, ws=None, ws_bytes=0, sep=None) == 0
    assert status(K=0, spheres=None, vel=None) == 0 and status(wind=None, wstride=0) == 0
    assert not lc.bits_equal(st["pos"], keep["pos"])
    # se3mpc_swarm_separation_*
    sep = sc.d(np.full(B, 5.0))
    sstat = lambda **kw: (lambda a: lib.loop_status("swarm_separation", suf, a["B"], a["M"], a["pos"], a["vel"], a["sep"], be.stream()))(
        dict(dict(B=B, M=M, pos=be.ptr(st["pos"]), vel=be.ptr(st["vel"]), sep=be.ptr(sep)), **kw))
    for kw, want in [(dict(B=-3), -3), (dict(M=0), -3), (dict(M=1025), -3), (dict(M=4), -3), (dict(pos=None), -1), (dict(vel=None), -1), (dict(sep=None), -1)]:
        got = sstat(**kw)
        assert got == want, f"se3mpc_swarm_separation {kw}: {got} != {want}"
        assert lib.last_error(), f"{kw}: se3mpc_last_error not set"
    assert np.all(h.to_host(sep) == 5.0), "a rejected call launched"
    assert sstat(B=0, pos=None) == 0 and sstat(M=1) == 0 and np.all(h.to_host(sep) == 5.0)
    assert sstat() == 0 and np.all(h.to_host(sep) < 5.0)


# ---- 9. front end ----------------------------------------------------------------------------------------------------------------------
def check_front_end(h, N=6, swarms=2, M=3, Kn=2, Ks=2):
    """run_mppi_swarm: the documented keys and shapes; smoother= and mixer= are refused; swarm_size = 1 is run_mppi_fused, bit for bit."""
    import pytest
    sc = Scene(h, N, swarms, M, Ks=Ks, Kn=Kn)
    B = sc.B
    mcl = _monte_carlo(h, sc)
    args = (sc.d(sc.p0), sc.d(sc.v0), sc.goal_d, 2, 3, 0.01, 64, 2, 1.0, 50.0)
    kw = dict(seed=9, spheres=sc.sph_d, obstacle_weight=40.0, wind=sc.wind_d)
    res = mcl.run_mppi_swarm(*args, **kw, sphere_velocities=sc.vel_d, sphere_t0=0.7, swarm_size=M, neighbours=Kn, mate_radius=0.3, want_neighbours=True,
                             log=True)
    shapes = dict(pos=(B, 3), vel=(B, 3), att=(B, 3), omega=(B, 3), time=(B,), controller_state=(B, 12), U=(B, N, 3), cost=(B,), trace=(B, 2, 2),
                  clearance=(B,), separation=(B,), neighbours=(B, Kn))
    for k, s in shapes.items():
        assert tuple(res[k].shape) == s, (k, tuple(res[k].shape))
    assert tuple(res["logs"][0]["plan_last"].shape) == (B, 3, N, 3)
    nb = h.to_host(res["neighbours"])
    assert nb.dtype == np.int32 and np.all(nb // M == np.arange(B)[:, None] // M) and np.all(nb != np.arange(B)[:, None])
    assert np.all(np.isfinite(h.to_host(res["separation"])))
    assert mcl.run_mppi_swarm(*args, **kw, swarm_size=M, neighbours=Kn)["neighbours"] is None
    with pytest.raises(ValueError, match="smoother"):
        mcl.run_mppi_swarm(*args, **kw, smoother=h.ops.lib.smoother_default_params(), swarm_size=M)
    with pytest.raises(ValueError, match="mixer"):
        mcl.run_mppi_swarm(*args, **kw, mixer=h.ops.lib.mixer_default_params(), swarm_size=M)
    with pytest.raises(ValueError, match="mixer"):
        mcl.run_mppi_swarm(*args, **kw, motor_health=sc.d(np.ones(4)), swarm_size=M)
    for mv_kw in (dict(), dict(sphere_velocities=sc.vel_d, sphere_t0=0.7)):
        a = mcl.run_mppi_swarm(*args, log=True, **kw, **mv_kw, swarm_size=1, neighbours=Kn, mate_radius=0.3)
        b = mcl.run_mppi_fused(*args, log=True, **kw, **mv_kw)
        for k in ("pos", "vel", "att", "omega", "time", "controller_state", "U", "cost", "trace", "clearance"):
            assert lc.bits_equal(a[k], b[k]), k
        assert lc.bits_equal(a["logs"][0]["plan_last"], b["logs"][0]["plan_last"])
        assert np.all(np.isinf(h.to_host(a["separation"])))
