"""Developer probe (GPU box): what flying the edge loop (latency buffer -> OnboardController -> simulator) inside the one-launch Monte-Carlo gains
or costs against the chain of launches it fuses.

The shape of bench.py's Monte-Carlo leg -- 4096 drones x 33 planning cycles x 15 steps at sim_dt 0.01, horizon-6 plans, the leg's scene -- at latency
depth 0 (no buffer) and 5, float32 and float64, HIP events, warm (60 ms of untimed load first, as bench.py's warm_device), the two forms
alternating from the same fresh state, median and minimum of 10:

* ClosedLoopMonteCarlo.run_edge_fused (one se3mpc_monte_carlo_edge_* launch) against ClosedLoopMonteCarlo.run_edge (se3mpc_solve_* +
  se3mpc_edge_loop_* per cycle: 66 launches; the kernels of that chain compute what the parent commit's do).

Then the same pair once at 64 drones, depth 5: the launch-bound end.  Each row carries a position checksum of both forms of its first pair, which
must agree to the bit; a row that does not ends the probe with status 1.

`python tools/gpu_probe_monte_carlo_edge.py [out.json]` (default profiles/monte_carlo_edge.json)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dart_planner_amd.capi import Params  # noqa: E402
from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "monte_carlo_edge.json")
ops = Ops(); dev = ops.be.device
CYCLES, SUBSTEPS, SIM_DT, REPS, WARM_MS = 33, 15, 0.01, 10, 60.0
prm = Params.reference_defaults()
mc = ClosedLoopMonteCarlo(ops, prm, ops.lib.controller_default_params(), ops.lib.simulator_default_params())
results = []


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def warm(fn):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < WARM_MS:
        fn(); torch.cuda.synchronize()


def measure(S, depth, name, dtype, g):
    p0 = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev).repeat(S, 1) + 0.2 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    v0 = 0.3 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    goal = torch.tensor([8.0, 0.0, 5.0], dtype=dtype, device=dev).repeat(S, 1).contiguous()
    wind = torch.randn(S, 3, dtype=dtype, device=dev, generator=g).contiguous()
    fused = lambda: mc.run_edge_fused(p0, v0, goal, CYCLES, SUBSTEPS, SIM_DT, latency_depth=depth, wind=wind)["pos"]
    chain = lambda: mc.run_edge(p0, v0, goal, CYCLES, SUBSTEPS, SIM_DT, latency_depth=depth, wind=wind)["pos"]
    warm(chain)
    fused(); torch.cuda.synchronize()
    t_n, t_o, first = [], [], None
    for _ in range(REPS):
        torch.cuda.synchronize(); us, pos_n = event_us(fused); t_n.append(us)
        torch.cuda.synchronize(); us, pos_o = event_us(chain); t_o.append(us)
        if first is None:
            first = (float(pos_n.double().sum()), float(pos_o.double().sum()), bool(torch.equal(pos_n, pos_o)))
    row = dict(what=f"run_edge_fused (1 launch) vs run_edge ({2 * CYCLES} launches)", dtype=name, drones=S, latency_depth=depth, cycles=CYCLES,
               substeps=SUBSTEPS, horizon=prm.horizon, new_ms_median=float(np.median(t_n)) * 1e-3, new_ms_min=float(np.min(t_n)) * 1e-3,
               old_ms_median=float(np.median(t_o)) * 1e-3, old_ms_min=float(np.min(t_o)) * 1e-3, ratio_median=float(np.median(t_n) / np.median(t_o)),
               new_pos_checksum=first[0], old_pos_checksum=first[1], same_bits=first[2])
    results.append(row); print(json.dumps(row), flush=True)
    return first[2]


g = torch.Generator(device=dev); g.manual_seed(5)
ok = True
for S, depths in ((4096, (0, 5)), (64, (5,))):
    for name, dtype in (("float32", torch.float32), ("float64", torch.float64)):
        for depth in depths:
            ok = ok and measure(S, depth, name, dtype, g)
            if not ok:
                break
        if not ok:
            break
    if not ok:
        break

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
print("wrote", OUT)
sys.exit(0 if ok else 1)
