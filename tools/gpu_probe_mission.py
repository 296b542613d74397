"""Developer probe (GPU box): what flying waypoint missions costs in the closed-loop Monte-Carlo, and what the one launch gains over the chain.

The shape of bench.py's Monte-Carlo leg -- 4096 drones x 33 planning cycles x 15 steps at sim_dt 0.01, horizon-6 plans -- with W = 4 waypoints per
drone, then the same at 64 drones: the launch-bound end.  float32 and float64, HIP events, warm (60 ms of untimed load first, as bench.py's
warm_device), the forms alternating from the same fresh state, median and minimum of 10:

* ClosedLoopMonteCarlo.run_mission_fused (one se3mpc_monte_carlo_mission_* launch) against ClosedLoopMonteCarlo.run_mission (se3mpc_mission_goal_* +
  se3mpc_solve_* + se3mpc_closed_loop_* per cycle: 99 launches), without a field;
* ClosedLoopMonteCarlo.run_fused (se3mpc_monte_carlo_*, which this work does not touch) on the same drones with one fixed goal: the difference to
  run_mission_fused is the cost of the mission step itself.

Each row carries a position checksum of the two mission forms of its first pair, which must agree to the bit; a row that does not ends the probe
with status 1.

`python tools/gpu_probe_mission.py [out.json]` (default profiles/mission.json)."""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mission.json")
ops = Ops(); dev = ops.be.device
CYCLES, SUBSTEPS, SIM_DT, REPS, WARM_MS, W = 33, 15, 0.01, 10, 60.0, 4
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


def measure(S, name, dtype, g):
    p0 = torch.tensor([0.0, 0.0, 4.0], dtype=dtype, device=dev).repeat(S, 1) + 0.2 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    v0 = 0.3 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    hops = torch.tensor([0.5, 0.3, 3.4], dtype=torch.float64, device=dev) + torch.randn(S, W, 3, dtype=torch.float64, device=dev, generator=g)
    wp = (p0.double()[:, None, :] + torch.cumsum(hops, dim=1)).contiguous()            # a chain of waypoints above each drone
    labels = torch.randint(0, 4, (S, W), dtype=torch.int32, device=dev, generator=g)
    goal = wp[:, 0].to(dtype).contiguous()
    wind = torch.randn(S, 3, dtype=dtype, device=dev, generator=g).contiguous()
    fused = lambda: mc.run_mission_fused(p0, v0, wp, labels, CYCLES, SUBSTEPS, SIM_DT, wind=wind)
    chain = lambda: mc.run_mission(p0, v0, wp, labels, CYCLES, SUBSTEPS, SIM_DT, wind=wind)
    fixed = lambda: mc.run_fused(p0, v0, goal, CYCLES, SUBSTEPS, SIM_DT, wind=wind)
    warm(chain)
    fused(); fixed(); torch.cuda.synchronize()
    t_n, t_o, t_f, first = [], [], [], None
    for _ in range(REPS):
        torch.cuda.synchronize(); us, out_n = event_us(fused); t_n.append(us)
        torch.cuda.synchronize(); us, out_o = event_us(chain); t_o.append(us)
        torch.cuda.synchronize(); us, _ = event_us(fixed); t_f.append(us)
        if first is None:
            same = all(bool(torch.equal(out_n[k], out_o[k])) for k in ("pos", "vel", "time", "controller_state", "mission_state", "goal"))
            first = (float(out_n["pos"].double().sum()), float(out_o["pos"].double().sum()), same,
                     torch.bincount(out_n["phase"].long(), minlength=6).tolist(), int(out_n["waypoint_index"].max()))
    med = lambda t: float(np.median(t)) * 1e-3
    row = dict(what=f"run_mission_fused (1 launch) vs run_mission ({3 * CYCLES} launches) vs run_fused with a fixed goal (1 launch)", dtype=name, drones=S,
               waypoints=W, cycles=CYCLES, substeps=SUBSTEPS, horizon=prm.horizon, fused_ms_median=med(t_n), fused_ms_min=float(np.min(t_n)) * 1e-3,
               chain_ms_median=med(t_o), chain_ms_min=float(np.min(t_o)) * 1e-3, fixed_goal_ms_median=med(t_f), fixed_goal_ms_min=float(np.min(t_f)) * 1e-3,
               fused_over_chain=med(t_n) / med(t_o), fused_over_fixed_goal=med(t_n) / med(t_f), fused_pos_checksum=first[0], chain_pos_checksum=first[1],
               same_bits=first[2], end_phases=first[3], max_waypoint_index=first[4])
    results.append(row); print(json.dumps(row), flush=True)
    return first[2]


g = torch.Generator(device=dev); g.manual_seed(5)
ok = True
for S in (4096, 64):
    for name, dtype in (("float32", torch.float32), ("float64", torch.float64)):
        ok = ok and measure(S, name, dtype, g)
        if not ok:
            break
    if not ok:
        break

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
print("wrote", OUT)
sys.exit(0 if ok else 1)
