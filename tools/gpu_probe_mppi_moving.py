"""Probe of MPPI around moving spheres: what the per-step centres cost.  HIP events, the card warmed first, 5 warm-up
launches per shape, median of 20; the static and the moving entry alternate launch by launch in the same process on the same centres.
  planner      4096 problems x 256 samples x 8 iterations, K = 16, N = 30 and N = 50, f32 and f64: se3mpc_mppi_moving_* (random velocities up
               to 3 m/s) against se3mpc_mppi_*
  closed loop  256 drones x 33 cycles x 15 steps (256 samples, 8 iterations, N = 30, K = 16), f32 and f64: se3mpc_mppi_closed_loop_moving_*
               against se3mpc_mppi_closed_loop_*
  python tools/gpu_probe_mppi_moving.py [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 20, 5


def timed_pair(torch, static, moving, reps=REPS, warmup=WARMUP):
    """Median / min of `reps` launches of each form, alternating, after `warmup` launches of each."""
    for _ in range(warmup):
        static(); moving()
    torch.cuda.synchronize()
    ts = {"static": [], "moving": []}
    for _ in range(reps):
        for name, go in (("static", static), ("moving", moving)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); go(); e1.record(); e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    return dict(static_us_median=med["static"], moving_us_median=med["moving"], static_us_min=float(np.min(ts["static"])),
                moving_us_min=float(np.min(ts["moving"])), ratio=med["moving"] / med["static"])


def table(torch, rng, K, tdt):
    c = np.round(rng.uniform(0, 15, (K, 3)) * 2) / 2
    d = rng.normal(0, 1, (K, 3))
    vel = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, (K, 1))
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=tdt, device="cuda:0")
    return dev(np.concatenate([c, np.ones((K, 1))], 1)), dev(vel)


def planner_part(torch, ops):
    from dart_planner_amd.capi import Params
    rows = []
    B, S, iters, K = 4096, 256, 8, 16
    for N in (30, 50):
        for dt in (np.float32, np.float64):
            tdt = torch.float32 if dt == np.float32 else torch.float64
            prm = Params.reference_defaults(horizon=N, dt=0.1)
            rng = np.random.default_rng(2)
            lane = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a, float).reshape(B, -1).T), dtype=tdt, device="cuda:0")
            p0, v0, goal = lane(rng.uniform(-20, 20, (B, 3))), lane(rng.uniform(-5, 5, (B, 3))), lane(rng.uniform(-20, 20, (B, 3)))
            U = lane(np.clip(rng.normal(0, 2, (B, N, 3)) + [0, 0, 14.715], [-17.67, -17.67, 2.0], [17.67, 17.67, 25.0]))
            sph, vel = table(torch, rng, K, tdt)
            out = (torch.empty_like(U), torch.empty(B, dtype=tdt, device="cuda:0"), torch.empty((iters, B), dtype=tdt, device="cuda:0"),
                   torch.empty(B, dtype=torch.int64, device="cuda:0"))
            kw = dict(seed=1, spheres=sph, obstacle_weight=1000.0, out=out)
            static = lambda: ops.mppi(prm, p0, v0, goal, U, S, iters, 4.0, 1000.0, **kw)
            moving = lambda: ops.mppi(prm, p0, v0, goal, U, S, iters, 4.0, 1000.0, sphere_vel=vel, sphere_t0=0.5, **kw)
            rows.append(dict(part="planner", N=N, K=K, dtype=np.dtype(dt).name, problems=B, samples=S, iters=iters, **timed_pair(torch, static, moving)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def closed_loop_part(torch, ops):
    from dart_planner_amd.capi import Params
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    rows = []
    B, S, iters, K, N, cycles, substeps, sim_dt = 256, 256, 8, 16, 30, 33, 15, 0.01
    for dt in (np.float32, np.float64):
        tdt = torch.float32 if dt == np.float32 else torch.float64
        prm = Params.reference_defaults(horizon=N, dt=0.1)
        rng = np.random.default_rng(3)
        dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=tdt, device="cuda:0")
        p0, v0 = dev(rng.uniform(-1, 1, (B, 3)) + [0, 0, 2]), dev(rng.uniform(-1, 1, (B, 3)))
        goal = dev(rng.uniform(0, 15, (B, 3)))
        sph, vel = table(torch, rng, K, tdt)
        mcl = ClosedLoopMonteCarlo(ops, prm)
        args = (p0, v0, goal, cycles, substeps, sim_dt, S, iters, 4.0, 1000.0)
        kw = dict(seed=1, spheres=sph, obstacle_weight=1000.0)
        static = lambda: mcl.run_mppi_fused(*args, **kw)
        moving = lambda: mcl.run_mppi_fused(*args, sphere_velocities=vel, sphere_t0=0.5, **kw)
        rows.append(dict(part="closed_loop", N=N, K=K, dtype=np.dtype(dt).name, drones=B, samples=S, iters=iters, cycles=cycles, substeps=substeps,
                         **timed_pair(torch, static, moving)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mppi_moving_launch.json"))
    a = ap.parse_args()
    import torch
    from dart_planner_amd.ops import Ops, TorchBackend
    assert torch.cuda.is_available(), "the probe needs an MI355X"
    ops = Ops(TorchBackend("cuda:0"))
    x = torch.randn(4096, 4096, device="cuda:0")
    for _ in range(200):                                            # bring the card to its working clocks before anything is timed
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    rows = planner_part(torch, ops) + closed_loop_part(torch, ops)
    doc = dict(probe="tools/gpu_probe_mppi_moving.py", device=torch.cuda.get_device_name(0), reps=REPS, warmup=WARMUP,
               expectation="planner, N = 30, K = 16, f32: (482 + 16 x 12.25) / 630 = 1.08 from the VALU count of DESIGN.md 5.8", rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
