"""Developer probe (GPU box): what flying the edge loop (latency buffer -> OnboardController -> simulator) inside the one-launch closed-loop MPPI
Monte-Carlo gains or costs against the chain of launches it fuses.

Scene and shape of tools/gpu_probe_mppi_closed_loop.py: N = 30 at a plan step of 0.1 s, S = 256 samples, 8 iterations, 33 cycles
x 15 simulator steps of 0.01 s; 256 and 4096 drones, K = 0 and K = 16 spheres, latency depth 0 (no buffer) and 5, float32 and float64.

* ClosedLoopMonteCarlo.run_mppi_edge_fused (one se3mpc_mppi_closed_loop_edge_* launch, with the clearance) against
* ClosedLoopMonteCarlo.run_mppi_edge (se3mpc_mppi_closed_loop_* with no steps + se3mpc_edge_loop_* per cycle: 66 launches, no clearance; the
  kernels of that chain compute what the parent commit's do).

HIP events, warm (60 ms of untimed load first, as bench.py's warm_device), the two forms alternating from the same fresh state, median and
minimum of 10.  Each row carries a position checksum of both forms of its first pair, which must agree to the bit; a row that does not ends the
probe with status 1.

`python tools/gpu_probe_mppi_closed_loop_edge.py [out.json]` (default profiles/mppi_closed_loop_edge.json)."""
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
from tools.gpu_probe_mppi_closed_loop import CYCLES, ITERS, LAM, N, PLAN_DT, S, SIGMA, SIM_DT, SUBSTEPS, W_OBS, scene  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mppi_closed_loop_edge.json")
REPS, WARM_MS = 10, 60.0
ops = Ops()
mc = ClosedLoopMonteCarlo(ops, Params.reference_defaults(horizon=N, dt=PLAN_DT), ops.lib.controller_default_params(), ops.lib.simulator_default_params())
results = []


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); b.synchronize()
    return a.elapsed_time(b), out


def warm(fn):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < WARM_MS:
        fn(); torch.cuda.synchronize()


def measure(B, K, depth, dtype):
    p0, v0, goal, sph, wind = scene(torch, B, K, dtype)
    kw = dict(seed=1, spheres=sph, obstacle_weight=W_OBS if K else 0.0, wind=wind, latency_depth=depth)
    args = (p0, v0, goal, CYCLES, SUBSTEPS, SIM_DT, S, ITERS, SIGMA, LAM)
    fused = lambda: mc.run_mppi_edge_fused(*args, **kw)
    chain = lambda: mc.run_mppi_edge(*args, **kw)
    warm(chain)
    fused(); torch.cuda.synchronize()
    t_f, t_c, first = [], [], None
    for _ in range(REPS):
        torch.cuda.synchronize(); ms, out_f = event_ms(fused); t_f.append(ms)
        torch.cuda.synchronize(); ms, out_c = event_ms(chain); t_c.append(ms)
        if first is None:
            pf, pc = out_f["pos"], out_c["pos"]
            clr = out_f["clearance"].double() if K else None
            first = dict(fused_pos_checksum=float(pf.double().sum()), chain_pos_checksum=float(pc.double().sum()),
                         same_bits=bool(torch.equal(pf.view(torch.uint8), pc.view(torch.uint8))),
                         zero_thrust_steps_max=int(out_f["zero_thrust_steps"].max()),
                         clearance_min=None if clr is None else float(clr.min()), clearance_median=None if clr is None else float(clr.median()),
                         drones_inside_a_sphere=None if clr is None else int((clr < 0).sum()))
    spread = lambda t: float((np.max(t) - np.min(t)) / np.median(t))
    row = dict(what=f"run_mppi_edge_fused (1 launch) vs run_mppi_edge ({2 * CYCLES} launches)", dtype=dtype, drones=B, samples=S, iters=ITERS, horizon=N,
               spheres=K, latency_depth=depth, cycles=CYCLES, substeps=SUBSTEPS, reps=REPS, fused_ms_median=float(np.median(t_f)),
               fused_ms_min=float(np.min(t_f)), fused_spread=spread(t_f), chain_ms_median=float(np.median(t_c)), chain_ms_min=float(np.min(t_c)),
               chain_spread=spread(t_c), ratio_median=float(np.median(t_f) / np.median(t_c)), **first)
    results.append(row); print(json.dumps(row), flush=True)
    return first["same_bits"]


ok = True
for B, K, depth, dtype in [(B, K, depth, dtype) for B in (256, 4096) for K in (0, 16) for depth in (0, 5) for dtype in ("float32", "float64")]:
    ok = measure(B, K, depth, dtype)
    if not ok:
        break

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
print("wrote", OUT)
sys.exit(0 if ok else 1)
