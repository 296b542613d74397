"""Developer probe (GPU box): what flying the TrajectorySmoother and the MotorMixer inside the one-launch Monte-Carlo gains and costs.

The shape of bench.py's Monte-Carlo leg -- 4096 drones x 33 planning cycles x 15 control + simulator steps at sim_dt 0.01, horizon-6 plans, the
leg's scene -- with both stages and one health row per drone, float32 and float64, HIP events, warm (60 ms of untimed load first, as
bench.py's warm_device), forms alternating from the same fresh state, median and minimum of 10:

* ClosedLoopMonteCarlo.run_fused_staged (one se3mpc_monte_carlo_staged_* launch) against ClosedLoopMonteCarlo.run with the same stages
  (se3mpc_solve_* + se3mpc_smoother_update_* + se3mpc_closed_loop_actuated_* per cycle: 99 launches; the kernels of that chain compute what
  the parent commit's do);
* the same against ClosedLoopMonteCarlo.run_fused (se3mpc_monte_carlo_*, no stages): the price of the two stages inside one launch.

Each row carries a position checksum of both forms (the first pair must agree to the bit; the second differs: the stages change the flight).

`python tools/gpu_probe_monte_carlo_staged.py [out.json]` (default profiles/monte_carlo_staged.json)."""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "monte_carlo_staged.json")
ops = Ops(); dev = ops.be.device
S, CYCLES, SUBSTEPS, SIM_DT, REPS, WARM_MS = 4096, 33, 15, 0.01, 10, 60.0
prm = Params.reference_defaults()
smp, mp = SmootherParams.reference_defaults(), ops.lib.mixer_default_params()
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


g = torch.Generator(device=dev); g.manual_seed(5)
for name, dtype in (("float32", torch.float32), ("float64", torch.float64)):
    p0 = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev).repeat(S, 1) + 0.2 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    v0 = 0.3 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
    goal = torch.tensor([8.0, 0.0, 5.0], dtype=dtype, device=dev).repeat(S, 1).contiguous()
    wind = torch.randn(S, 3, dtype=dtype, device=dev, generator=g).contiguous()
    health = (0.6 + 0.4 * torch.rand(S, 4, dtype=dtype, device=dev, generator=g)).contiguous()
    stages = dict(smoother=smp, mixer=mp, motor_health=health)
    staged = lambda: mc.run_fused_staged(p0, v0, goal, CYCLES, SUBSTEPS, SIM_DT, wind=wind, **stages)["pos"]
    chain = lambda: mc.run(p0, v0, goal, CYCLES, SUBSTEPS, SIM_DT, wind=wind, **stages)["pos"]
    plain = lambda: mc.run_fused(p0, v0, goal, CYCLES, SUBSTEPS, SIM_DT, wind=wind)["pos"]
    for what, old in ((f"run_fused_staged (1 launch) vs run with smoother + mixer ({3 * CYCLES} launches)", chain),
                      ("run_fused_staged (smoother + mixer) vs run_fused (no stages)", plain)):
        warm(old)
        staged(); torch.cuda.synchronize()
        t_n, t_o = [], []
        for _ in range(REPS):
            torch.cuda.synchronize(); us, pos_n = event_us(staged); t_n.append(us)
            torch.cuda.synchronize(); us, pos_o = event_us(old); t_o.append(us)
        row = dict(what=what, dtype=name, drones=S, cycles=CYCLES, substeps=SUBSTEPS, horizon=prm.horizon, new_us_median=float(np.median(t_n)),
                   new_us_min=float(np.min(t_n)), old_us_median=float(np.median(t_o)), old_us_min=float(np.min(t_o)),
                   ratio_median=float(np.median(t_n) / np.median(t_o)), new_pos_checksum=float(pos_n.double().sum()),
                   old_pos_checksum=float(pos_o.double().sum()), same_bits=bool(torch.equal(pos_n, pos_o)))
        results.append(row); print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
print("wrote", OUT)
