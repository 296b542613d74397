"""Checks of the split-sample MPPI entry points (se3mpc_mppi_split_*, Ops.mppi_split: one problem's samples over several workgroups, one
launch per iteration) shared by the host-emulation suite (tests/test_emu_mppi_split.py) and the MI355X suite
(tests/test_gpu_mppi_split.py).  Built on mppi_checks.problem / Run and mppi_oracle.mppi; every check takes a parity_checks.Harness."""
import numpy as np

import mppi_checks as mc
import mppi_oracle as mo
from mppi_checks import F32_COST_REL, F32_TRACE_REL, F32_U_ABS, F64_REL


class Run(mc.Run):
    """mppi_checks.Run with a `splits` argument: None launches se3mpc_mppi_*, an integer se3mpc_mppi_split_*."""

    def __call__(self, S, iters, sigma, lam, splits=None, seed=0, iter_base=0, index_base=0, U=None, **kw):
        if splits is None:
            return super().__call__(S, iters, sigma, lam, seed=seed, iter_base=iter_base, index_base=index_base, U=U, **kw)
        return self.h.ops.mppi_split(self.prm, self.p0, self.v0, self.goal, self.U if U is None else U, S, iters, sigma, lam, splits, seed=seed,
                                     iter_base=iter_base, index_base=index_base, spheres=self.sph, obstacle_weight=self.w_obs, **kw)


def _same(a, b, what):
    for x, y, name in zip(a, b, ("U", "cost", "trace", "keys")):
        assert np.array_equal(x, y), f"{what}: {name} differs"


def check_against_oracle(h, N, S, splits, nprob, iters, K=0, seed=5, sigma=1.0, w_obs=40.0, params=None):
    """U, cost, trace and keys of the split kernels against the float64 oracle, with the bounds of mppi_checks.check_against_oracle: they
    were set for float64 sums in a fixed order over the same samples, and another fixed order moves those sums in their last bits only."""
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, nprob, seed, K=K, params=params)
    p0, v0, goal, U, sph = (mc._round(h, a) for a in (p0, v0, goal, U, sph))
    run = Run(h, prm, p0, v0, goal, U, sph, w_obs)
    lam = mc.temperature_for(cfg, p0, v0, goal, U, S, sigma, seed, sph, w_obs)
    for it in iters:
        Ud, cd, trd, keys = run.host(run(S, it, sigma, lam, splits, seed=seed, iter_base=2))
        assert trd.shape[0] == it
        for p in range(nprob):
            Ur, cr, trr = mo.mppi(p0[p], v0[p], goal[p], U[p], p, S, it, sigma, lam, seed, cfg, iter_base=2, spheres=sph, obstacle_weight=w_obs,
                                  dtype=h.dt)
            dU = np.max(np.abs(Ud[p] - Ur))
            if h.dt == np.float32:
                c_at = mo.cost(p0[p], v0[p], goal[p], Ud[p], cfg, sph, w_obs)          # the cost of the nominal the kernel returned
                print(f"S={S} splits={splits} iters={it} problem {p}: |dU| {dU:.3g}, cost rel {abs(cd[p] - c_at) / abs(c_at):.3g}")
                assert dU <= F32_U_ABS, f"U of problem {p}: {dU}"
                assert abs(cd[p] - c_at) <= F32_COST_REL * abs(c_at), f"cost of problem {p}"
                assert np.all(np.abs(trd[:it, p] - trr) <= F32_TRACE_REL * np.abs(trr)), f"trace of problem {p}: {trd[:it, p]} vs {trr}"
            else:
                print(f"S={S} splits={splits} iters={it} problem {p}: |dU| {dU:.3g}, cost rel {abs(cd[p] - cr) / abs(cr):.3g}")
                assert dU <= F64_REL * 25, f"U of problem {p}: {dU}"
                assert abs(cd[p] - cr) <= F64_REL * abs(cr), f"cost of problem {p}"
                assert np.all(np.abs(trd[:it, p] - trr) <= F64_REL * np.abs(trr)), f"trace of problem {p}"
            k = int(keys[p]) & 0xFFFFFFFFFFFFFFFF
            assert h.ops.lib.key_index(k) == p and h.ops.lib.key_cost(k) == np.float32(cd[p]), "key = orderable(cost) << 32 | q"
        if it == 0:
            assert np.array_equal(Ud, U), "iters = 0 copies U_in"


def check_one_split_is_the_unsplit_kernel(h, N, S, nprob, iters=3, K=0, seed=7, sigma=1.5):
    """splits = 1: the fold over one partial is the identity and the pass over the samples is shared code, so U, cost, trace and keys are
    the bytes of se3mpc_mppi_* (at a finite temperature and at lambda -> 0, iters = 0 included)."""
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, nprob, seed, K=K)
    run = Run(h, prm, p0, v0, goal, U, sph, 40.0)
    for lam, its in ((50.0, (iters, 0)), (1e-300, (1,))):
        for it in its:
            kw = dict(seed=seed, iter_base=3, index_base=4)
            _same(run.host(run(S, it, sigma, lam, 1, **kw)), run.host(run(S, it, sigma, lam, None, **kw)), f"S={S} iters={it} lambda={lam}")


def check_one_iteration_any_split(h, N, S, splits, nprob, K=0, seed=11, sigma=1.5):
    """One iteration from the same nominal: the split and the unsplit kernel draw the same samples and give them the same costs, so their
    weights have the same arguments; what differs is the order of the float64 sums and the minimum a partial sum is first expressed
    against.  With box = the largest thrust magnitude of the box and u = 2^-53:
      * a float64 sum of S products w_s T_s in any order is within S u sum_s w_s |T_s| <= S u box sum_s w_s of the exact sum, the weight sum
        within S u sum_s w_s, so each mean is within 2 S u box of the exact mean;
      * re-expressing a partial against another minimum multiplies its rows AND its weight sum by the same exp((m_new - m_old) / lambda), whose
        argument is rounded to u relative: |argument| < 745 (beyond, the factor is 0), so the factor is off by < 745 * 2 u relative -- a
        common perturbation of the weights of that partial, which moves a weighted mean by at most twice itself times box: 2980 u box;
      * two kernels, each with both errors: |dU| <= 2 (2 S + 2980) u box, = 3.9e-11 N for S = 2048 (the largest here) and box = 25 N.
    float64: that is far inside F64_REL * 25 = 2.5e-8, the bound the issue sets.  float32: both kernels round their float64 mean to
    float32, and two float64 values 3.9e-11 apart round to the same float32 or to neighbours: at most one unit in the last place of
    float32 at the box's scale, spacing(float32(box)) = 2^-19 = 1.9e-6 N (the clip that follows does not widen a difference)."""
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, nprob, seed, K=K)
    run = Run(h, prm, p0, v0, goal, U, sph, 40.0)
    lam = mc.temperature_for(cfg, p0, v0, goal, U, S, sigma, seed, sph if K else None, 40.0)
    box = float(np.max(np.abs(mo.thrust_box(cfg))))
    assert 2 * (2 * S + 2980) * 2.0 ** -53 * box <= 1e-10
    tol = F64_REL * 25 if h.dt == np.float64 else float(np.spacing(np.float32(box)))
    a = run.host(run(S, 1, sigma, lam, splits, seed=seed, iter_base=6))
    b = run.host(run(S, 1, sigma, lam, None, seed=seed, iter_base=6))
    d = float(np.max(np.abs(a[0] - b[0])))
    print(f"S={S} splits={splits} {np.dtype(h.dt).name}: max |U_split - U_unsplit| = {d:.3g} (bound {tol:.3g})")
    assert d <= tol, f"one iteration, {splits} splits against the unsplit kernel: {d} > {tol}"


def check_nan_costs_weigh_nothing(h, N, S, splits, iters=2):
    """A problem whose every sample costs NaN (a NaN start state) keeps its nominal through every iteration, as se3mpc_mppi_* leaves it:
    each split contributes minimum +inf and zero sums, the trace is +inf, the cost NaN; the problem next to it is not disturbed."""
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, 2, 17)
    U = mc._round(h, U)
    bad = p0.copy()
    bad[0, 0] = np.nan
    a = Run(h, prm, bad, v0, goal, U)
    got, ref = a.host(a(S, iters, 1.0, 50.0, splits, seed=1)), a.host(a(S, iters, 1.0, 50.0, None, seed=1))
    clean = Run(h, prm, p0, v0, goal, U)
    ok = clean.host(clean(S, iters, 1.0, 50.0, splits, seed=1))
    assert np.array_equal(got[0][0], U[0]) and np.array_equal(ref[0][0], U[0]), "no finite cost: the nominal stays"
    assert np.all(np.isposinf(got[2][:, 0])) and np.isnan(got[1][0]) and got[3][0] == ref[3][0]
    assert np.array_equal(got[0][1], ok[0][1]) and got[1][1] == ok[1][1] and np.array_equal(got[2][:, 1], ok[2][:, 1]) and np.all(np.isfinite(got[0][1]))


def check_chunking_and_slices(h, N, S, splits, nprob, iters=3, K=0, seed=13, sigma=1.0):
    """mppi_checks.check_chunking_and_slices for the split entry point: iters = K in one call == K calls of one iteration chained through
    iter_base; problems [lo, hi) with index_base = lo == those rows of the batch; a second launch == the first (all bit for bit)."""
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, nprob, seed, K=K)
    run = Run(h, prm, p0, v0, goal, U, sph, 40.0)
    lam = 50.0
    full = run.host(run(S, iters, sigma, lam, splits, seed=seed, iter_base=100))
    _same(run.host(run(S, iters, sigma, lam, splits, seed=seed, iter_base=100)), full, "run-to-run identity")
    Ucur = run.U
    for i in range(iters):
        o = run(S, 1, sigma, lam, splits, seed=seed, iter_base=100 + i, U=Ucur)
        Ucur = o["U"]
        step = run.host(o)
        assert np.array_equal(step[2][0], full[2][i]), f"trace row {i} from one-iteration calls"
    assert np.array_equal(step[0], full[0]) and np.array_equal(step[1], full[1]) and np.array_equal(step[3], full[3]), "iters = K == K calls"
    lo, hi = 1, nprob - 1
    sub = Run(h, prm, p0[lo:hi], v0[lo:hi], goal[lo:hi], U[lo:hi], sph, 40.0)
    part = sub.host(sub(S, iters, sigma, lam, splits, seed=seed, iter_base=100, index_base=lo))
    assert np.array_equal(part[0], full[0][lo:hi]) and np.array_equal(part[1], full[1][lo:hi]), "slice [lo, hi) == the batch's"
    assert np.array_equal(part[2], full[2][:, lo:hi]) and np.array_equal(part[3], full[3][lo:hi]), "slice trace / keys"
    # a preallocated workspace holding another call's leftovers gives the same bytes: it needs no initialisation
    ws = h.ops.mppi_split_workspace(prm, nprob, splits)
    run(S, 2, sigma, 7.0, splits, seed=seed + 1, iter_base=3, workspace=ws)
    _same(run.host(run(S, iters, sigma, lam, splits, seed=seed, iter_base=100, workspace=ws)), full, "a reused workspace")
    return full


def check_limits(h, N, S, splits, nprob, iters=3, seed=9, sigma=2.0):
    """mppi_checks.check_limits (K = 0) for the split entry point: lambda -> 0 returns exactly the best sample of the WHOLE S, whichever split
    holds it, and a non-increasing trace; lambda -> inf returns the plain mean.  -> the split that held each problem's winner, computed
    from the oracle's costs of the samples."""
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, nprob, seed)
    run = Run(h, prm, p0, v0, goal, U, None, 0.0)
    Ud, cd, trd, _ = run.host(run(S, iters, sigma, 1e-300, splits, seed=seed, iter_base=5))
    assert np.all(np.diff(trd, axis=0) <= 0), "lambda -> 0: the trace is non-increasing"
    assert np.all(cd <= trd[-1] * (1 + 1e-6)), "final cost at the best sample"
    U1 = run.host(run(S, 1, sigma, 1e-300, splits, seed=seed, iter_base=5))[0]
    Ts = h.to_host(h.ops.mppi_samples(prm, run.U, S, sigma, seed=seed, iter_base=5)["T"]).astype(float).reshape(N, 3, nprob, S)
    Uinf = run.host(run(S, 1, sigma, 1e300, splits, seed=seed, iter_base=5))[0]
    winners = []
    for p in range(nprob):
        Tp = Ts[:, :, p, :].transpose(2, 0, 1)                        # (S, N, 3)
        best = int(np.argmin(mo.cost(p0[p], v0[p], goal[p], Tp, cfg)))
        winners.append(best // (S // splits))
        assert np.array_equal(U1[p], Tp[best]), f"lambda -> 0: problem {p} takes its best sample {best} (split {winners[-1]})"
        col = h.to_dev(np.ascontiguousarray(Ts[:, :, p, :].reshape(3 * N, S).astype(h.dt)))
        sums = h.to_host(h.ops.population_sums(col)).astype(float)
        mean = sums[:-1] / sums[-1]
        tol = 1e-6 * 25 if h.dt == np.float32 else 1e-13 * 25
        assert np.max(np.abs(Uinf[p].reshape(-1) - mean)) <= tol, f"lambda -> inf: problem {p} moves to the plain mean"
    return winners


def assert_winners_spread(winners):
    assert len(set(winners)) >= 2 and any(w != 0 for w in winners), f"the winners sat in splits {sorted(set(winners))}: the cases do not reach past one split"


def check_invalid_arguments(h, N=6):
    """Every rule of se3mpc_mppi_split_* returns its status, sets se3mpc_last_error and launches nothing (U_out, cost and the workspace
    untouched): the rules of se3mpc_mppi_*, splits, S against splits, the workspace (NULL, one byte short)."""
    prm, cfg, p0, v0, goal, U, sph = mc.problem(N, 2, 1, K=2)
    run = Run(h, prm, p0, v0, goal, U, sph, 1.0)
    ops, be = h.ops, h.ops.be
    suf = "f32" if h.dt == np.float32 else "f64"
    Uo = h.to_dev(np.zeros((3 * N, 2), h.dt))
    cost = h.to_dev(np.zeros(2, h.dt))
    need = ops.lib.mppi_split_workspace_bytes(N, 2, 2)
    assert need == 2 * 2 * (2 * (3 * N + 2) + 3 * N) * 8 and ops.lib.mppi_split_workspace_bytes(N, 2, 0) == 0
    assert ops.lib.mppi_split_workspace_bytes(N, 2, 4) > need > ops.lib.mppi_split_workspace_bytes(N, 1, 2) > 0
    ws = h.to_dev(np.zeros(need // 8, np.float64))
    ok = dict(prm=prm, nprob=2, ld=2, S=128, iters=1, sigma=1.0, lam=1.0, K=2, w=1.0, U=be.ptr(run.U), spheres=be.ptr(run.sph), splits=2,
              ws=be.ptr(ws), ws_bytes=need)

    def status(**kw):
        a = dict(ok, **kw)
        return ops.lib.call_status("mppi_split", suf, a["nprob"], a["ld"], a["S"], a["iters"], a["sigma"], a["lam"], 0, 0, None, 0, be.ptr(run.p0),
                                   be.ptr(run.v0), be.ptr(run.goal), a["U"], be.ptr(Uo), a["spheres"], a["K"], a["w"], be.ptr(cost), None, None,
                                   a["splits"], a["ws"], a["ws_bytes"], be.stream(), params=a["prm"])

    cases = [  # what se3mpc_mppi_* rejects
             (dict(S=0), -3), (dict(S=63), -3), (dict(S=96), -3), (dict(S=65536 + 64), -3), (dict(S=-64), -3), (dict(lam=0.0), -4),
             (dict(lam=-1.0), -4), (dict(lam=float("nan")), -4), (dict(lam=float("inf")), -4), (dict(sigma=-0.5), -4),
             (dict(sigma=float("nan")), -4), (dict(K=-1), -3), (dict(K=257), -3), (dict(prm=prm.copy(horizon=65)), -2),
             (dict(prm=prm.copy(dt=0.0)), -4), (dict(prm=None), -1), (dict(nprob=-1), -3), (dict(ld=1), -3), (dict(iters=-1), -3),
             (dict(w=float("nan")), -4), (dict(w=-1.0), -4), (dict(U=None), -1), (dict(spheres=None), -1),
             # the split's own: splits >= 1, S a multiple of 64 * splits, S / splits >= 64, the workspace
             (dict(splits=0), -3), (dict(splits=-2), -3), (dict(S=192, splits=2), -3), (dict(S=320, splits=4), -3), (dict(S=64, splits=2), -3),
             (dict(S=128, splits=4), -3), (dict(ws=None), -1), (dict(ws_bytes=need - 1), -3), (dict(ws_bytes=0), -3),
             (dict(splits=1, S=64, ws_bytes=ops.lib.mppi_split_workspace_bytes(N, 2, 1) - 1), -3)]
    for kw, want in cases:
        got = status(**kw)
        assert got == want, f"{kw}: {got} != {want}"
        assert ops.lib.last_error(), f"{kw}: se3mpc_last_error not set"
    assert np.all(h.to_host(Uo) == 0) and np.all(h.to_host(cost) == 0) and np.all(h.to_host(ws) == 0), "a rejected call launched"
    assert status(nprob=0, U=None, ws=None, ws_bytes=0) == 0 and np.all(h.to_host(Uo) == 0)
    assert status(iters=0, ws=None, ws_bytes=0) == 0, "iters = 0 needs no workspace"
    assert status() == 0 and status(S=192, splits=3, ws_bytes=ops.lib.mppi_split_workspace_bytes(N, 2, 3) - 8) == -3
    assert np.any(h.to_host(Uo) != 0)
