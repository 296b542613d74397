"""MPPI probe: the batched launch (4096 problems x 256 samples x 8 iterations, N = 30, K = 0 / 16, f32 / f64; and N = 50,
K = 16 next to the obstacle-aware gradient loop's yardstick), plan_mppi latency next to plan_shooting and plan_trajectory in the same
process, and the (sigma, temperature, iters) tuning sweep on the obstacle scene and the cfg-2 distribution.  HIP events, warm-up as bench.py.
The split part: one problem, N = 30, f32 / f64, K = 0 / 16, S in {1024, 4096, 16384} x splits in {unsplit, 1 .. 64}: the
captured plan (wall clock to the synchronise, as the plan part) and the bare launches (HIP events); then B in {1, 16, 256} x S = 1024.
  python tools/gpu_probe_mppi.py launch|plan|tune|split [--out FILE]      (one part per process: each GPU step under its own time limit)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def launch_part(ops, reps=20, warmup=5):
    import torch
    import mppi_checks as mc
    from dart_planner_amd.capi import Params
    rows = []
    for N, K, dts in ((30, 0, (np.float32, np.float64)), (30, 16, (np.float32, np.float64)), (50, 16, (np.float32,))):
        for dt in dts:
            tdt = torch.float32 if dt == np.float32 else torch.float64
            B, S, iters = 4096, 256, 8
            prm = Params.reference_defaults(horizon=N, dt=0.1)
            rng = np.random.default_rng(2)
            lane = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a, float).reshape(B, -1).T), dtype=tdt, device="cuda:0")
            p0, v0, goal = lane(rng.uniform(-20, 20, (B, 3))), lane(rng.uniform(-5, 5, (B, 3))), lane(rng.uniform(-20, 20, (B, 3)))
            U = lane(np.clip(rng.normal(0, 2, (B, N, 3)) + [0, 0, 14.715], [-17.67, -17.67, 2.0], [17.67, 17.67, 25.0]))
            sph = None
            if K:
                c = np.round(rng.uniform(0, 15, (K, 3)) * 2) / 2
                sph = torch.tensor(np.concatenate([c, np.ones((K, 1))], 1), dtype=tdt, device="cuda:0")
            out = (torch.empty_like(U), torch.empty(B, dtype=tdt, device="cuda:0"), torch.empty((iters, B), dtype=tdt, device="cuda:0"),
                   torch.empty(B, dtype=torch.int64, device="cuda:0"))
            go = lambda: ops.mppi(prm, p0, v0, goal, U, S, iters, 4.0, 1000.0, seed=1, spheres=sph, obstacle_weight=1000.0, out=out)
            for _ in range(warmup):
                go()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); go(); e1.record(); e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            us = float(np.median(ts))
            evals = B * S * iters
            rows.append(dict(N=N, K=K, dtype=np.dtype(dt).name, problems=B, samples=S, iters=iters, kernel_us_median=us, kernel_us_min=float(np.min(ts)),
                             sample_rollouts_per_s=evals / (us * 1e-6)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def plan_part(reps=200, warmup=20):
    import torch
    from dart_planner_amd.common.types import DroneState
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=30), precision="f32")
    st = DroneState(timestamp=0.0, position=np.array([0.0, 0.0, 1.0]), velocity=np.zeros(3))
    goal = np.array([4.0, 2.0, 2.0])
    rows = []

    def timed(name, fn):
        ts = []
        for i in range(warmup + reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            if i >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        rows.append(dict(plan=name, p50_ms=float(np.percentile(ts, 50)), p95_ms=float(np.percentile(ts, 95))))
        print(json.dumps(rows[-1]), flush=True)

    for iters in (1, 4, 8):
        timed(f"plan_mppi S=1024 iters={iters} (warm, captured)", lambda: pl.plan_mppi(st, goal, n_samples=1024, iters=iters))
    timed("plan_shooting 8192 x 16 (captured)", lambda: pl.plan_shooting(st, goal, n_samples=8192, iters=16))
    timed("plan_trajectory (L-BFGS-B)", lambda: pl.plan_trajectory(st, goal))
    return rows


def tune_part(ops):
    import torch
    import mppi_oracle as mo
    from dart_planner_amd.capi import Params
    from dart_planner_amd.common.timing_alignment import TimingConfig, get_timing_manager, reset_timing_manager
    from dart_planner_amd.common.types import DroneState
    from dart_planner_amd.perception.explicit_geometric_mapper import ExplicitGeometricMapper
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    rows = []
    reset_timing_manager()
    get_timing_manager(TimingConfig(control_frequency=10.0))
    pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=30), device="cuda:0")
    mapper = ExplicitGeometricMapper(resolution=0.5, max_range=20.0, ops=ops)
    mapper.add_obstacle(np.array([3.0, 0.0, 2.0]), 1.0)
    st = DroneState(timestamp=0.0, position=np.array([0.0, 0.0, 2.0]), velocity=np.zeros(3))
    for c in mapper.local_obstacle_spheres(st.position, 20.0, 0.6, 20, 1.0):
        pl.add_obstacle(c[:3], float(c[3]))
    goal = np.array([8.0, 0.5, 2.0])
    grid = [(s, l, i) for s in (1.0, 2.0, 4.0) for l in (10.0, 100.0, 1000.0, 10000.0) for i in (4, 8, 16)]
    for sigma, lam, iters in grid:
        tr = pl.plan_mppi(st, goal, n_samples=1024, iters=iters, sigma=sigma, temperature=lam, warm_start=False)
        safe, _ = mapper.is_trajectory_safe(tr.positions, safety_margin=1.0)
        r = pl.last_result
        rows.append(dict(scene="obstacle", sigma=sigma, temperature=lam, iters=iters, cost_with_penalty=r["cost_with_penalty"], penalty=r["penalty"],
                         safe=bool(safe), goal_distance=float(np.linalg.norm(tr.positions[-1] - goal))))
        print(json.dumps(rows[-1]), flush=True)
    reset_timing_manager()
    # cfg-2 distribution: 1024 problems, N = 30, at the planner's default dt and at dt = 0.1
    B, N = 1024, 30
    rng = np.random.default_rng(1)
    p0, v0, goal = rng.uniform(-20, 20, (B, 3)), rng.uniform(-5, 5, (B, 3)), rng.uniform(-20, 20, (B, 3))
    lane = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a, float).reshape(B, -1).T), dtype=torch.float32, device="cuda:0")
    hover = lane(np.tile([0, 0, 14.715], (B, N, 1)))
    for dtp in (1.0 / 400.0, 0.1):
        prm = Params.reference_defaults(horizon=N, dt=dtp)
        c0 = ops.mppi(prm, lane(p0), lane(v0), lane(goal), hover, 64, 0, 1.0, 1.0)["cost"].cpu().numpy().astype(float)
        for sigma, lam, iters in grid:
            c = ops.mppi(prm, lane(p0), lane(v0), lane(goal), hover, 1024, iters, sigma, lam, seed=0)["cost"].cpu().numpy().astype(float)
            rows.append(dict(scene="cfg-2", dt=dtp, sigma=sigma, temperature=lam, iters=iters, median_cost_ratio_vs_hover=float(np.median(c / c0)),
                             mean_cost_ratio_vs_hover=float(np.mean(c / c0))))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def split_part(ops, reps=200, warmup=20, iters=8):
    """Split-sample MPPI against the one-workgroup path, same process, warm: rows of kind "plan" (plan_mppi through its captured graph, host
    clock around the call, which ends in a synchronise), "launch" (the iters + 1 launches of Ops.mppi_split / the one of Ops.mppi between HIP
    events) and "batch" (the launches over B problems).  splits = None is the unsplit path."""
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.common.types import DroneState
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    N = 30
    rng = np.random.default_rng(4)
    spheres16 = np.concatenate([np.round(rng.uniform(0, 15, (16, 3)) * 2) / 2, np.ones((16, 1))], axis=1)
    st = DroneState(timestamp=0.0, position=np.array([0.0, 0.0, 1.0]), velocity=np.zeros(3))
    goal = np.array([4.0, 2.0, 2.0])
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def pcts(ts, unit):
        return {f"p50_{unit}": float(np.percentile(ts, 50)), f"p95_{unit}": float(np.percentile(ts, 95))}

    def event_times(go):
        for _ in range(warmup):
            go()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); go(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return ts

    def operands(B, S, tdt, K):
        prm = Params.reference_defaults(horizon=N, dt=0.1)
        r = np.random.default_rng(2)
        lane = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a, float).reshape(B, -1).T), dtype=tdt, device="cuda:0")
        p0, v0, gl = lane(r.uniform(-2, 2, (B, 3)) + [0, 0, 2]), lane(r.uniform(-1, 1, (B, 3))), lane(r.uniform(-4, 4, (B, 3)) + [0, 0, 2])
        U = lane(np.tile([0.0, 0.0, 14.715], (B, N, 1)))
        sph = torch.tensor(spheres16, dtype=tdt, device="cuda:0") if K else None
        out = (torch.empty_like(U), torch.empty(B, dtype=tdt, device="cuda:0"), torch.empty((iters, B), dtype=tdt, device="cuda:0"),
               torch.empty(B, dtype=torch.int64, device="cuda:0"))
        return prm, p0, v0, gl, U, sph, out

    def launcher(B, S, tdt, K, g):
        prm, p0, v0, gl, U, sph, out = operands(B, S, tdt, K)
        kw = dict(seed=1, spheres=sph, obstacle_weight=1000.0, out=out)
        if g is None:
            return lambda: ops.mppi(prm, p0, v0, gl, U, S, iters, 4.0, 100.0, **kw)
        ws = ops.mppi_split_workspace(prm, B, g)
        return lambda: ops.mppi_split(prm, p0, v0, gl, U, S, iters, 4.0, 100.0, g, workspace=ws, **kw)

    valid = lambda S, g: g is None or (S % (64 * g) == 0 and S // g >= 64)
    for precision in ("f32", "f64"):
        tdt = torch.float32 if precision == "f32" else torch.float64
        for K in (0, 16):
            pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=N), device="cuda:0")
            for c in spheres16[:K]:
                pl.add_obstacle(c[:3], float(c[3]))
            for S in (1024, 4096, 16384):
                for g in (None, 1, 2, 4, 8, 16, 32, 64):
                    if not valid(S, g):
                        continue
                    ts = []
                    for i in range(warmup + reps):
                        t0 = time.perf_counter()
                        pl.plan_mppi(st, goal, n_samples=S, iters=iters, precision=precision, splits=g)
                        torch.cuda.synchronize()
                        if i >= warmup:
                            ts.append((time.perf_counter() - t0) * 1e3)
                    emit(kind="plan", dtype=precision, K=K, N=N, samples=S, iters=iters, splits=g, auto=pl._mppi_splits("auto", S), **pcts(ts, "ms"))
                    emit(kind="launch", dtype=precision, K=K, N=N, samples=S, iters=iters, splits=g, problems=1,
                         **pcts(event_times(launcher(1, S, tdt, K, g)), "us"))
    for B in (1, 16, 256):
        for g in (None, 1, 2, 4, 8, 16):
            emit(kind="batch", dtype="f32", K=0, N=N, samples=1024, iters=iters, splits=g, problems=B, auto=SE3MPCPlanner._mppi_splits("auto", 1024, B),
                 **pcts(event_times(launcher(B, 1024, torch.float32, 0, g)), "us"))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["launch", "plan", "tune", "split"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend("cuda:0"))
    rows = {"launch": lambda: launch_part(ops), "plan": plan_part, "tune": lambda: tune_part(ops), "split": lambda: split_part(ops)}[a.part]()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
