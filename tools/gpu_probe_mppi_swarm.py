"""Probe of the swarm MPPI closed loop: what the prologue and the launch per cycle cost over one launch around a table of
the same size.  HIP events, the card warmed first, 5 warm-up runs per form, median of 20; the two forms alternate run by run in the same
process on the same drones.
  64 swarms x 16 drones, N = 30, 256 samples, 8 iterations, 33 cycles x 15 steps, f32 and f64:
  swarm   se3mpc_mppi_closed_loop_swarm_* with Ks = 16 shared moving spheres and Kn = 4 mates per table, then se3mpc_swarm_separation_*
          (33 + 2 launches)
  moving  se3mpc_mppi_closed_loop_moving_* on the same 1024 drones around K = 20 shared moving spheres (one launch)
  python tools/gpu_probe_mppi_swarm.py [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 20, 5


def timed_pair(torch, moving, swarm, reps=REPS, warmup=WARMUP):
    """Median / min of `reps` runs of each form, alternating, after `warmup` runs of each."""
    for _ in range(warmup):
        moving(); swarm()
    torch.cuda.synchronize()
    ts = {"moving": [], "swarm": []}
    for _ in range(reps):
        for name, go in (("moving", moving), ("swarm", swarm)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); go(); e1.record(); e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    return dict(moving_us_median=med["moving"], swarm_us_median=med["swarm"], moving_us_min=float(np.min(ts["moving"])),
                swarm_us_min=float(np.min(ts["swarm"])), timed_runs_each=len(ts["swarm"]), ratio=med["swarm"] / med["moving"])


def table(torch, rng, K, tdt):
    c = np.round(rng.uniform(0, 15, (K, 3)) * 2) / 2
    d = rng.normal(0, 1, (K, 3))
    vel = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, (K, 1))
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=tdt, device="cuda:0")
    return dev(np.concatenate([c, np.ones((K, 1))], 1)), dev(vel)


def rows_of(torch, ops):
    from dart_planner_amd.capi import Params
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    rows = []
    swarms, M, S, iters, Ks, Kn, N, cycles, substeps, sim_dt = 64, 16, 256, 8, 16, 4, 30, 33, 15, 0.01
    B = swarms * M
    for dt in (np.float32, np.float64):
        tdt = torch.float32 if dt == np.float32 else torch.float64
        prm = Params.reference_defaults(horizon=N, dt=0.1)
        rng = np.random.default_rng(3)
        dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=tdt, device="cuda:0")
        centre = np.repeat(rng.uniform(0, 15, (swarms, 3)), M, axis=0)
        p0, v0 = dev(centre + rng.uniform(-2, 2, (B, 3))), dev(rng.uniform(-1, 1, (B, 3)))
        goal = dev(rng.uniform(0, 15, (B, 3)))
        sph, vel = table(torch, rng, Ks + Kn, tdt)
        mcl = ClosedLoopMonteCarlo(ops, prm)
        args = (p0, v0, goal, cycles, substeps, sim_dt, S, iters, 4.0, 1000.0)
        kw = dict(seed=1, obstacle_weight=1000.0, sphere_t0=0.5)
        moving = lambda: mcl.run_mppi_fused(*args, spheres=sph, sphere_velocities=vel, **kw)
        swarm = lambda: mcl.run_mppi_swarm(*args, spheres=sph[:Ks].contiguous(), sphere_velocities=vel[:Ks].contiguous(), swarm_size=M, neighbours=Kn,
                                           mate_radius=0.3, **kw)
        sep = swarm()["separation"]
        rows.append(dict(dtype=np.dtype(dt).name, swarms=swarms, swarm_size=M, drones=B, N=N, samples=S, iters=iters, cycles=cycles, substeps=substeps,
                         Ks=Ks, Kn=Kn, K_moving=Ks + Kn, min_separation_m=float(sep.min()), **timed_pair(torch, moving, swarm)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mppi_swarm_launch.json"))
    a = ap.parse_args()
    import torch
    from dart_planner_amd.ops import Ops, TorchBackend
    assert torch.cuda.is_available(), "the probe needs an MI355X"
    ops = Ops(TorchBackend("cuda:0"))
    x = torch.randn(4096, 4096, device="cuda:0")
    for _ in range(200):                                            # bring the card to its working clocks before anything is timed
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    rows = rows_of(torch, ops)
    doc = dict(probe="tools/gpu_probe_mppi_swarm.py", device=torch.cuda.get_device_name(0), reps=REPS, warmup=WARMUP,
               expectation="none fixed in advance: the ratio prices the prologue and 34 more launches over one launch around a table of the same size",
               rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
