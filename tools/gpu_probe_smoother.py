"""Developer probe (GPU box): what the TrajectorySmoother costs per control step.

* se3mpc_closed_loop_smoothed_* against the unchanged se3mpc_closed_loop_* of the same build: 4096 drones x 100 steps on one plan per drone
  (30 rows), float32 and float64, HIP events around one launch, warm, the two alternating, median and minimum of 20.  Measured twice: in
  normal following, and with every drone inside a transition (the branch with the quintic and its two norm clamps).
* ClosedLoopMonteCarlo.run(smoother=...) against run() at the README's shape (4096 runs x 33 cycles x 15 steps at 10 ms), host clock around a
  synchronised run, median of 5.

`python tools/gpu_probe_smoother.py [out.json]` (default profiles/smoother_launch.json)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dart_planner_amd.capi import Params, SmootherParams  # noqa: E402
from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "smoother_launch.json")
ops = Ops(); dev = ops.be.device
B, NSTEPS, N, SIM_DT, REPS = 4096, 100, 30, 0.001, 20
cp, sp, mp = ops.lib.controller_default_params(), ops.lib.simulator_default_params(), SmootherParams.reference_defaults()
results = []


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3


for name, dtype in (("float32", torch.float32), ("float64", torch.float64)):
    g = torch.Generator(device=dev); g.manual_seed(7)
    k = torch.arange(N, dtype=torch.float64, device=dev)
    ts = 5.0 + k * 0.01
    start = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev) + 0.2 * torch.randn(B, 1, 3, dtype=dtype, device=dev, generator=g)
    V = (0.5 * torch.randn(B, 1, 3, dtype=dtype, device=dev, generator=g)).expand(B, N, 3).contiguous()
    P = (start + V * (k * 0.01).to(dtype)[None, :, None]).contiguous()
    A = torch.zeros(B, N, 3, dtype=dtype, device=dev)
    P_far = (P + torch.tensor([2.0, 1.0, 0.0], dtype=dtype, device=dev)).contiguous()
    pos0, vel0 = P[:, 0].contiguous(), V[:, 0].contiguous()
    zeros = torch.zeros(B, 3, dtype=dtype, device=dev)

    for scene in ("following", "transition"):
        def fresh():
            s = dict(st=ops.controller_state(cp, B), sm=ops.smoother_state(B), time=torch.full((B,), 5.0, dtype=torch.float64, device=dev), pos=pos0.clone(),
                     vel=vel0.clone(), att=zeros.clone(), om=zeros.clone())
            ops.smoother_update(mp, s["sm"], s["time"], ts, P, V, A)
            if scene == "transition":
                ops.smoother_update(mp, s["sm"], s["time"], ts, P_far, V, A, old=(ts, P, V, A))
            return s
        plan = (ts, P_far if scene == "transition" else P, V, A)
        smoothed = lambda s: ops.closed_loop_smoothed(mp, cp, sp, s["st"], s["sm"], s["time"], s["pos"], s["vel"], s["att"], s["om"], *plan, nsteps=NSTEPS, sim_dt=SIM_DT)
        plain = lambda s: ops.closed_loop(cp, sp, s["st"], s["time"], s["pos"], s["vel"], s["att"], s["om"], *plan, nsteps=NSTEPS, sim_dt=SIM_DT, stop_at_plan_end=False)
        for fn in (smoothed, plain):                             # warm: code objects, allocator pools
            fn(fresh())
        torch.cuda.synchronize()
        t_s, t_p = [], []
        for _ in range(REPS):                                    # alternating, every launch from the same fresh state
            s = fresh(); torch.cuda.synchronize(); t_s.append(event_us(lambda: smoothed(s)))
            s = fresh(); torch.cuda.synchronize(); t_p.append(event_us(lambda: plain(s)))
        row = dict(what="se3mpc_closed_loop_smoothed vs se3mpc_closed_loop, one launch", scene=scene, dtype=name, drones=B, steps=NSTEPS, plan_rows=N,
                   smoothed_us_median=float(np.median(t_s)), smoothed_us_min=float(np.min(t_s)), plain_us_median=float(np.median(t_p)),
                   plain_us_min=float(np.min(t_p)), ratio_median=float(np.median(t_s) / np.median(t_p)),
                   smoothed_ns_per_drone_step=float(np.median(t_s) * 1e3 / (B * NSTEPS)))
        results.append(row); print(json.dumps(row), flush=True)

    # the README's Monte-Carlo shape
    S, cycles, substeps, sim_dt = 4096, 33, 15, 0.01
    p0 = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev).repeat(S, 1) + 0.2 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    v0 = 0.3 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    goal = torch.tensor([8.0, 0.0, 5.0], dtype=dtype, device=dev).repeat(S, 1).contiguous()
    wind = torch.randn(S, 3, dtype=dtype, device=dev, generator=g).contiguous()
    mc = ClosedLoopMonteCarlo(ops, Params.reference_defaults(), cp, sp)
    runs = dict(smoothed=lambda: mc.run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind, smoother=mp), plain=lambda: mc.run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind))
    times = {k_: [] for k_ in runs}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(5):
        for k_, fn in runs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times[k_].append(time.perf_counter() - t0)
    row = dict(what="ClosedLoopMonteCarlo.run(smoother=...) vs run()", dtype=name, runs=S, cycles=cycles, substeps=substeps, sim_dt=sim_dt,
               smoothed_ms_median=float(np.median(times["smoothed"]) * 1e3), plain_ms_median=float(np.median(times["plain"]) * 1e3),
               ratio_median=float(np.median(times["smoothed"]) / np.median(times["plain"])))
    results.append(row); print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
print("wrote", OUT)
