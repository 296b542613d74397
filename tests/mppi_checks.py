"""Checks of the MPPI planner kernels (se3mpc_mppi_*, se3mpc_mppi_samples_*) shared by the host-emulation suite
(tests/test_emu_mppi.py) and the MI355X suite (tests/test_gpu_mppi.py).  Every check takes a parity_checks.Harness."""
import numpy as np

import mppi_oracle as mo
import parity_checks as pc
from dart_planner_amd.capi import Params

# f32 kernels draw their uniforms, normals and samples in float32 and roll out in float32: the oracle (float64 on the same float32
# uniforms) is met to these bounds
F32_NORMAL_ABS = 2e-5           # normals (|n| <= 6.7): the float32 angle 2 pi u and the float32 log / sin / cos
F32_U_ABS = 2e-3                # nominal thrusts, newtons (float32 costs through the weights)
F32_COST_REL = 2e-5
F32_TRACE_REL = 1e-3            # the minimum sample cost of iterations after the first: float32 nominals within F32_U_ABS
F64_REL = 1e-9


def problem(N, nprob, seed, dt=0.1, K=0, params=None):
    """A batch of small problems at dt = 0.1 s (the horizon covers metres), nominals inside the thrust box around hover.
    params: overrides (e.g. a set of tests/param_sets.py) merged over the reference defaults at this horizon and dt."""
    rng = np.random.default_rng(seed)
    prm = pc.make_params(N, params, dt=dt)
    cfg = pc.oracle_cfg(prm)
    p0 = rng.uniform(-1, 1, (nprob, 3)) + [0, 0, 2]
    v0 = rng.uniform(-1, 1, (nprob, 3))
    goal = rng.uniform(-4, 4, (nprob, 3)) + [0, 0, 2]
    U = np.clip(rng.normal(0, 1.5, (nprob, N, 3)) + [0, 0, cfg.hover_thrust], *mo.thrust_box(cfg))
    sph = np.concatenate([rng.uniform(-3, 3, (K, 3)) + [0, 0, 2], rng.uniform(0.3, 1.0, (K, 1))], axis=1)
    return prm, cfg, p0, v0, goal, U, sph


def _round(h, a):
    return np.asarray(a).astype(h.dt).astype(float)


class Run:
    """Device operands of one batch and a launcher."""

    def __init__(self, h, prm, p0, v0, goal, U, sph=None, w_obs=0.0):
        B = len(p0)
        self.h, self.prm, self.B, self.w_obs = h, prm, B, w_obs
        self.p0, self.v0, self.goal, self.U = h.lane(p0, B), h.lane(v0, B), h.lane(goal, B), h.lane(U, B)
        self.sph = None if sph is None or len(sph) == 0 else h.to_dev(np.ascontiguousarray(np.asarray(sph).astype(h.dt)))

    def __call__(self, S, iters, sigma, lam, seed=0, iter_base=0, index_base=0, U=None, **kw):
        return self.h.ops.mppi(self.prm, self.p0, self.v0, self.goal, self.U if U is None else U, S, iters, sigma, lam, seed=seed,
                               iter_base=iter_base, index_base=index_base, spheres=self.sph, obstacle_weight=self.w_obs, **kw)

    def host(self, out):
        h, N = self.h, self.prm.horizon
        return (h.unlane(out["U"], (self.B, N, 3)), h.to_host(out["cost"]).astype(float),
                None if out["trace"] is None else h.to_host(out["trace"]).astype(float), None if out["keys"] is None else h.to_host(out["keys"]).copy())


def check_noise(h, N, S, nprob, seed=3, iter_base=7, index_base=11, sigma=1.5):
    """mppi_samples: the Philox words bit for bit, the normals to a few ulp (f64) / F32_NORMAL_ABS, the samples = clip(U + sigma n)."""
    prm, cfg, p0, v0, goal, U, _ = problem(N, nprob, seed)
    U = _round(h, U)
    seed64 = 0x0123456789ABCDEF + seed
    out = h.ops.mppi_samples(prm, h.lane(U, nprob), S, sigma, seed=seed64, iter_base=iter_base, index_base=index_base, want_noise=True, want_raw=True)
    raw = h.to_host(out["raw"]).view(np.uint32).reshape(N, 4, nprob, S)
    nrm = h.to_host(out["noise"]).astype(float).reshape(N, 3, nprob, S)
    T = h.to_host(out["T"]).astype(float).reshape(N, 3, nprob, S)
    for p in range(nprob):
        Tr, xr, nr = mo.samples(U[p], index_base + p, iter_base, S, sigma, seed64, cfg, h.dt)
        assert np.array_equal(raw[:, :, p, :].transpose(1, 2, 0), xr), f"Philox words of problem {p}"
        got_n = nrm[:, :, p, :].transpose(2, 0, 1)
        tol_n = F32_NORMAL_ABS if h.dt == np.float32 else 4e-15 * max(1.0, float(np.max(np.abs(nr))))
        assert np.max(np.abs(got_n - nr)) <= tol_n, f"normals of problem {p}: {np.max(np.abs(got_n - nr))}"
        tol_T = F32_NORMAL_ABS * sigma * 2 + 4e-6 * 25 if h.dt == np.float32 else 1e-12
        assert np.max(np.abs(T[:, :, p, :].transpose(2, 0, 1) - Tr)) <= tol_T, f"samples of problem {p}"
        assert np.array_equal(T[:, :, p, 0], np.clip(U[p], *mo.thrust_box(cfg)).astype(h.dt).astype(float)), "sample 0 is the nominal"
    return out


def temperature_for(cfg, p0, v0, goal, U, S, sigma, seed, sph=None, w_obs=0.0):
    """A temperature on the scale of the first iteration's sample costs (their median spread above the minimum, problem 0)."""
    T, _, _ = mo.samples(U[0], 0, 0, S, sigma, seed, cfg)
    c = mo.cost(p0[0], v0[0], goal[0], T, cfg, sph, w_obs)
    return float(np.median(c) - np.min(c))


def check_against_oracle(h, N, S, nprob, iters, K=0, seed=5, sigma=1.0, w_obs=40.0, params=None):
    """U, cost, trace of the fused kernel against the float64 oracle (iters = 0 included: evaluate and copy)."""
    prm, cfg, p0, v0, goal, U, sph = problem(N, nprob, seed, K=K, params=params)
    p0, v0, goal, U, sph = (_round(h, a) for a in (p0, v0, goal, U, sph))
    run = Run(h, prm, p0, v0, goal, U, sph, w_obs)
    lam = temperature_for(cfg, p0, v0, goal, U, S, sigma, seed, sph, w_obs)
    if K:
        pen = mo.orc.obstacle_penalty_grad(p0[:, None], v0[:, None], U[:, None], sph, cfg, w_obs)[0]
        assert np.any(pen > 0), "the check wants nominals inside the spheres' margins"
    for it in (iters, 0):
        Ud, cd, trd, keys = run.host(run(S, it, sigma, lam, seed=seed, iter_base=2, index_base=0))
        for p in range(nprob):
            Ur, cr, trr = mo.mppi(p0[p], v0[p], goal[p], U[p], p, S, it, sigma, lam, seed, cfg, iter_base=2, spheres=sph, obstacle_weight=w_obs,
                                  dtype=h.dt)
            if h.dt == np.float32:
                assert np.max(np.abs(Ud[p] - Ur)) <= F32_U_ABS, f"U of problem {p}: {np.max(np.abs(Ud[p] - Ur))}"
                c_at = mo.cost(p0[p], v0[p], goal[p], Ud[p], cfg, sph, w_obs)          # the cost of the nominal the kernel returned
                assert abs(cd[p] - c_at) <= F32_COST_REL * abs(c_at), f"cost of problem {p}"
                assert np.all(np.abs(trd[:it, p] - trr) <= F32_TRACE_REL * np.abs(trr)), f"trace of problem {p}: {trd[:it, p]} vs {trr}"
            else:
                assert np.max(np.abs(Ud[p] - Ur)) <= F64_REL * 25, f"U of problem {p}: {np.max(np.abs(Ud[p] - Ur))}"
                assert abs(cd[p] - cr) <= F64_REL * abs(cr), f"cost of problem {p}"
                assert np.all(np.abs(trd[:it, p] - trr) <= F64_REL * np.abs(trr)), f"trace of problem {p}"
            k = int(keys[p]) & 0xFFFFFFFFFFFFFFFF
            assert h.ops.lib.key_index(k) == p and h.ops.lib.key_cost(k) == np.float32(cd[p]), "key = orderable(cost) << 32 | q"
        if it == 0:
            assert np.array_equal(Ud, U), "iters = 0 copies U_in"


def check_limits(h, N, S, nprob, iters=3, K=0, seed=9, sigma=2.0, params=None):
    """lambda -> 0: the update is the best sample and the trace never increases; lambda -> inf: the update is the plain mean of the samples
    (se3mpc_population_sums_* with cost = NULL)."""
    prm, cfg, p0, v0, goal, U, sph = problem(N, nprob, seed, K=K, params=params)
    run = Run(h, prm, p0, v0, goal, U, sph, 40.0)
    Ud, cd, trd, _ = run.host(run(S, iters, sigma, 1e-300, seed=seed, iter_base=5))
    assert np.all(np.diff(trd, axis=0) <= 0), "lambda -> 0: the trace is non-increasing"
    assert np.array_equal(trd[-1], cd) or iters == 0 or np.all(cd <= trd[-1] * (1 + 1e-6)), "final cost at the best sample"
    one = run(S, 1, sigma, 1e-300, seed=seed, iter_base=5)
    U1, c1, tr1, _ = run.host(one)
    sm = h.ops.mppi_samples(prm, run.U, S, sigma, seed=seed, iter_base=5)
    Ts = h.to_host(sm["T"]).astype(float).reshape(N, 3, nprob, S)
    inf = run(S, 1, sigma, 1e300, seed=seed, iter_base=5)
    Uinf = run.host(inf)[0]
    for p in range(nprob):
        Tp = Ts[:, :, p, :].transpose(2, 0, 1)                        # (S, N, 3)
        if K == 0:
            c = mo.cost(p0[p], v0[p], goal[p], Tp, cfg)
            best = int(np.argmin(c))
            assert np.array_equal(U1[p], Tp[best]), f"lambda -> 0: problem {p} takes its best sample {best}"
        else:
            assert any(np.array_equal(U1[p], Tp[s]) for s in range(S)), f"lambda -> 0: problem {p} takes one of its samples"
        col = h.to_dev(np.ascontiguousarray(Ts[:, :, p, :].reshape(3 * N, S).astype(h.dt)))
        sums = h.to_host(h.ops.population_sums(col)).astype(float)
        mean = sums[:-1] / sums[-1]
        tol = 1e-6 * 25 if h.dt == np.float32 else 1e-13 * 25
        assert np.max(np.abs(Uinf[p].reshape(-1) - mean)) <= tol, f"lambda -> inf: problem {p} moves to the plain mean"


def check_composition(h, N, S, iters_seed=4, sigma=1.5, params=None):
    """Bit-level decomposition of one iteration (K = 0): mppi_samples -> rollout_cost_grad -> argmin -> population_sums(ref_key): the
    weighted mean equals one mppi iteration (f64: 1e-12, f32: 1e-6 relative to the box)."""
    prm, cfg, p0, v0, goal, U, _ = problem(N, 1, iters_seed, params=params)
    run = Run(h, prm, p0, v0, goal, U)
    lam = temperature_for(cfg, p0, v0, goal, U, S, sigma, iters_seed)
    U1 = run.host(run(S, 1, sigma, lam, seed=iters_seed, iter_base=9))[0][0]
    T = h.ops.mppi_samples(prm, run.U, S, sigma, seed=iters_seed, iter_base=9)["T"]
    wide = lambda a: h.to_dev(np.ascontiguousarray(np.repeat(h.to_host(a).astype(float), S, axis=1).astype(h.dt)))
    cost, _, _, _ = h.ops.rollout_cost_grad(prm, wide(run.p0), wide(run.v0), wide(run.goal), T, want_grad=False)
    key = h.ops.argmin(cost)
    sums = h.to_host(h.ops.population_sums(T, cost=cost, temperature=lam, ref_key=key)).astype(float)
    mean = (sums[:-1] / sums[-1]).reshape(N, 3)
    tol = 1e-6 * 25 if h.dt == np.float32 else 1e-12 * 25
    assert np.max(np.abs(U1 - mean)) <= tol, f"composed iteration: {np.max(np.abs(U1 - mean))}"


def check_chunking_and_slices(h, N, S, nprob, iters=3, K=0, seed=13, sigma=1.0):
    """iters = K in one call == K calls with iter_base stepping; problems [lo, hi) with index_base = lo == that slice of the batch;
    a second launch == the first (all bit for bit)."""
    prm, cfg, p0, v0, goal, U, sph = problem(N, nprob, seed, K=K)
    run = Run(h, prm, p0, v0, goal, U, sph, 40.0)
    lam = 50.0
    full = run.host(run(S, iters, sigma, lam, seed=seed, iter_base=100))
    again = run.host(run(S, iters, sigma, lam, seed=seed, iter_base=100))
    for a, b in zip(full, again):
        assert np.array_equal(a, b), "run-to-run identity"
    Ucur = run.U
    for i in range(iters):
        o = run(S, 1, sigma, lam, seed=seed, iter_base=100 + i, U=Ucur)
        Ucur = o["U"]
        step = run.host(o)
        assert np.array_equal(step[2][0], full[2][i]), f"trace row {i} from one-iteration calls"
    assert np.array_equal(step[0], full[0]) and np.array_equal(step[1], full[1]), "iters = K == K calls"
    lo, hi = 1, nprob - 1
    sub = Run(h, prm, p0[lo:hi], v0[lo:hi], goal[lo:hi], U[lo:hi], sph, 40.0)
    part = sub.host(sub(S, iters, sigma, lam, seed=seed, iter_base=100, index_base=lo))
    assert np.array_equal(part[0], full[0][lo:hi]) and np.array_equal(part[1], full[1][lo:hi]), "slice [lo, hi) == the batch's"
    assert np.array_equal(part[2], full[2][:, lo:hi]) and np.array_equal(part[3], full[3][lo:hi]), "slice trace / keys"
    return full


def check_invalid_arguments(h, N=6):
    """Every invalid argument returns its status, sets se3mpc_last_error and launches nothing (U_out untouched)."""
    prm, cfg, p0, v0, goal, U, sph = problem(N, 2, 1, K=2)
    run = Run(h, prm, p0, v0, goal, U, sph, 1.0)
    ops, be = h.ops, h.ops.be
    suf = "f32" if h.dt == np.float32 else "f64"
    Uo = h.to_dev(np.zeros((3 * N, 2), h.dt))
    cost = h.to_dev(np.zeros(2, h.dt))
    ok = dict(prm=prm, nprob=2, ld=2, S=64, iters=1, sigma=1.0, lam=1.0, K=2, w=1.0, U=be.ptr(run.U), spheres=be.ptr(run.sph))

    def status(**kw):
        a = dict(ok, **kw)
        return ops.lib.call_status("mppi", suf, a["nprob"], a["ld"], a["S"], a["iters"], a["sigma"], a["lam"], 0, 0, None, 0, be.ptr(run.p0),
                                   be.ptr(run.v0), be.ptr(run.goal), a["U"], be.ptr(Uo), a["spheres"], a["K"], a["w"], be.ptr(cost), None, None,
                                   be.stream(), params=a["prm"])

    cases = [(dict(S=0), -3), (dict(S=63), -3), (dict(S=96), -3), (dict(S=65536 + 64), -3), (dict(S=-64), -3), (dict(lam=0.0), -4),
             (dict(lam=-1.0), -4), (dict(lam=float("nan")), -4), (dict(lam=float("inf")), -4), (dict(sigma=-0.5), -4),
             (dict(sigma=float("nan")), -4), (dict(K=-1), -3), (dict(K=257), -3), (dict(prm=prm.copy(horizon=65)), -2),
             (dict(prm=prm.copy(dt=0.0)), -4), (dict(prm=None), -1), (dict(nprob=-1), -3), (dict(ld=1), -3), (dict(iters=-1), -3),
             (dict(w=float("nan")), -4), (dict(w=-1.0), -4), (dict(U=None), -1), (dict(spheres=None), -1)]
    for kw, want in cases:
        got = status(**kw)
        assert got == want, f"{kw}: {got} != {want}"
        assert ops.lib.last_error(), f"{kw}: se3mpc_last_error not set"
    assert np.all(h.to_host(Uo) == 0), "a rejected call launched"
    assert status() == 0 and status(nprob=0, U=None) == 0
    T = h.to_dev(np.zeros((3 * N, 128), h.dt))
    s_status = lambda S=64, ld_out=128, sigma=1.0, U=be.ptr(run.U): ops.lib.call_status("mppi_samples", suf, 2, 2, S, sigma, 0, 0, 0, U, be.ptr(T), ld_out,
                                                                                            None, None, be.stream(), params=prm)
    assert s_status() == 0 and s_status(ld_out=127) == -3 and s_status(S=65) == -3 and s_status(sigma=-1.0) == -4 and s_status(U=None) == -1
