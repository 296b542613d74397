"""Probe of the swarm's shared plans and of the tracked-sphere planner: what the tracked walk, the slab copy and the
intent rollout cost against the forms they stand beside.  HIP events, the card warmed first, 5 warm-up runs per form, median of 20; the two
forms alternate run by run in the same process on the same operands.
  swarm    64 swarms x 16 drones, N = 30, 256 samples, 8 iterations, 33 cycles x 15 steps, Ks = 16 shared moving spheres, Kn = 4 mates, f32 and
           f64: se3mpc_mppi_closed_loop_swarm_intent_* (share_plans=True) against se3mpc_mppi_closed_loop_swarm_* (5.8g's call), each followed by
           se3mpc_swarm_separation_*
  planner  4096 problems x 256 samples x 8 iterations, N = 30 and N = 50, f32 and f64: se3mpc_mppi_tracks_* on K = 12 moving rows + Kt = 4 tracks
           (one slab for all problems) against se3mpc_mppi_moving_* on K = 16 moving rows
  python tools/gpu_probe_mppi_swarm_intent.py [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 20, 5


def timed_pair(torch, base, new, reps=REPS, warmup=WARMUP):
    """Median / min of `reps` runs of each form, alternating, after `warmup` runs of each."""
    for _ in range(warmup):
        base(); new()
    torch.cuda.synchronize()
    ts = {"base": [], "new": []}
    for _ in range(reps):
        for name, go in (("base", base), ("new", new)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); go(); e1.record(); e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    return dict(base_us_median=med["base"], new_us_median=med["new"], base_us_min=float(np.min(ts["base"])), new_us_min=float(np.min(ts["new"])),
                timed_runs_each=len(ts["new"]), ratio=med["new"] / med["base"])


def table(torch, rng, K, tdt):
    c = np.round(rng.uniform(0, 15, (K, 3)) * 2) / 2
    d = rng.normal(0, 1, (K, 3))
    vel = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, (K, 1))
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=tdt, device="cuda:0")
    return dev(np.concatenate([c, np.ones((K, 1))], 1)), dev(vel), c, vel


def swarm_part(torch, ops):
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
        sph, vel, _, _ = table(torch, rng, Ks, tdt)
        mcl = ClosedLoopMonteCarlo(ops, prm)
        args = (p0, v0, goal, cycles, substeps, sim_dt, S, iters, 4.0, 1000.0)
        kw = dict(seed=1, obstacle_weight=1000.0, sphere_t0=0.5, spheres=sph, sphere_velocities=vel, swarm_size=M, neighbours=Kn, mate_radius=0.3)
        base = lambda: mcl.run_mppi_swarm(*args, **kw)
        new = lambda: mcl.run_mppi_swarm(*args, share_plans=True, **kw)
        rows.append(dict(part="swarm", dtype=np.dtype(dt).name, swarms=swarms, swarm_size=M, drones=B, N=N, samples=S, iters=iters, cycles=cycles,
                         substeps=substeps, Ks=Ks, Kn=Kn, base="se3mpc_mppi_closed_loop_swarm", new="se3mpc_mppi_closed_loop_swarm_intent",
                         min_separation_m=dict(base=float(base()["separation"].min()), new=float(new()["separation"].min())),
                         **timed_pair(torch, base, new)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def planner_part(torch, ops):
    from dart_planner_amd.capi import Params
    rows = []
    B, S, iters, K, Kt = 4096, 256, 8, 12, 4
    for N in (30, 50):
        for dt in (np.float32, np.float64):
            tdt = torch.float32 if dt == np.float32 else torch.float64
            prm = Params.reference_defaults(horizon=N, dt=0.1)
            rng = np.random.default_rng(2)
            lane = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a, float).reshape(B, -1).T), dtype=tdt, device="cuda:0")
            dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=tdt, device="cuda:0")
            p0, v0, goal = lane(rng.uniform(-20, 20, (B, 3))), lane(rng.uniform(-5, 5, (B, 3))), lane(rng.uniform(-20, 20, (B, 3)))
            U = lane(np.clip(rng.normal(0, 2, (B, N, 3)) + [0, 0, 14.715], [-17.67, -17.67, 2.0], [17.67, 17.67, 25.0]))
            sph, vel, c, v = table(torch, rng, K + Kt, tdt)
            tau = 0.5 + np.arange(N) * 0.1                                    # the last Kt rows' own paths, sampled at the plan's step times
            slab = dev(np.concatenate([c[None, K:] + v[None, K:] * tau[:, None, None], np.ones((N, Kt, 1))], axis=2))
            out = (torch.empty_like(U), torch.empty(B, dtype=tdt, device="cuda:0"), torch.empty((iters, B), dtype=tdt, device="cuda:0"),
                   torch.empty(B, dtype=torch.int64, device="cuda:0"))
            kw = dict(seed=1, obstacle_weight=1000.0, out=out, sphere_t0=0.5)
            base = lambda: ops.mppi(prm, p0, v0, goal, U, S, iters, 4.0, 1000.0, spheres=sph, sphere_vel=vel, **kw)
            new = lambda: ops.mppi_tracks(prm, p0, v0, goal, U, S, iters, 4.0, 1000.0, slab, spheres=sph[:K].contiguous(), sphere_vel=vel[:K].contiguous(),
                                          **kw)
            rows.append(dict(part="planner", N=N, K_moving=K, Kt=Kt, dtype=np.dtype(dt).name, problems=B, samples=S, iters=iters,
                             base=f"se3mpc_mppi_moving, K = {K + Kt}", new=f"se3mpc_mppi_tracks, K = {K} + Kt = {Kt}", **timed_pair(torch, base, new)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mppi_swarm_intent_launch.json"))
    a = ap.parse_args()
    import torch
    from dart_planner_amd.ops import Ops, TorchBackend
    assert torch.cuda.is_available(), "the probe needs an MI355X"
    ops = Ops(TorchBackend("cuda:0"))
    x = torch.randn(4096, 4096, device="cuda:0")
    for _ in range(200):                                            # bring the card to its working clocks before anything is timed
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    rows = swarm_part(torch, ops) + planner_part(torch, ops)
    doc = dict(probe="tools/gpu_probe_mppi_swarm_intent.py", device=torch.cuda.get_device_name(0), reps=REPS, warmup=WARMUP,
               expectation="none fixed in advance.  VALU count per sphere and step (DESIGN.md 5.8f's listing): 11 for a moving row, 8 for a tracked "
                           "row, on ~630 per sample-step at K = 16: planner (630 - 4 x 3) / 630 = 0.98; swarm: the same four rows, plus per drone and "
                           "cycle a slab copy of N x Kn rows by the workgroup and an N-step serial rollout on one lane",
               rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
