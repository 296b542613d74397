"""Developer probe (GPU box): what flying the TrajectorySmoother and the MotorMixer inside the one-launch closed-loop MPPI Monte-Carlo gains
and costs against the chain of launches it fuses.

Scene and shape of tools/gpu_probe_mppi_closed_loop.py: N = 30 at a plan step of 0.1 s, S = 256 samples, 8 iterations, 33
cycles x 15 simulator steps of 0.01 s, K = 16 spheres; B in {256, 4096}, float32 and float64, both stages, one health row per drone.

* ClosedLoopMonteCarlo.run_mppi_fused_staged (one se3mpc_mppi_closed_loop_staged_* launch, with the clearance) against
* ClosedLoopMonteCarlo.run_mppi(smoother=, mixer=, motor_health=): se3mpc_mppi_closed_loop_* as the planner, se3mpc_smoother_update_*,
  se3mpc_closed_loop_actuated_* per cycle, 99 launches, no clearance -- the parent commit's code, unchanged.

HIP events; every shape is run once untimed in both forms first; then the two forms alternate from the same fresh state, median of 10.  The
spread of repeating the same form is recorded per form ((max - min) / median of its 10 runs).  The position bytes of the first pair must
agree.

`python tools/gpu_probe_mppi_closed_loop_staged.py [out.json]` (default profiles/mppi_closed_loop_staged.json)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dart_planner_amd.capi import Params, SmootherParams  # noqa: E402
from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402
from tools.gpu_probe_mppi_closed_loop import CYCLES, ITERS, LAM, N, PLAN_DT, S, SIGMA, SIM_DT, SUBSTEPS, W_OBS, scene  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mppi_closed_loop_staged.json")
K, REPS = 16, 10
ops = Ops()
smp, mp = SmootherParams.reference_defaults(), ops.lib.mixer_default_params()
mc = ClosedLoopMonteCarlo(ops, Params.reference_defaults(horizon=N, dt=PLAN_DT), ops.lib.controller_default_params(), ops.lib.simulator_default_params())
results = []


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); b.synchronize()
    return a.elapsed_time(b), out


for B in (256, 4096):
    for dtype in ("float32", "float64"):
        p0, v0, goal, sph, wind = scene(torch, B, K, dtype)
        rng = np.random.default_rng(3)
        health = torch.tensor(rng.uniform(0.6, 1.0, (B, 4)), dtype=p0.dtype, device=p0.device)
        kw = dict(seed=1, spheres=sph, obstacle_weight=W_OBS, wind=wind, smoother=smp, mixer=mp, motor_health=health)
        args = (p0, v0, goal, CYCLES, SUBSTEPS, SIM_DT, S, ITERS, SIGMA, LAM)
        fused = lambda: mc.run_mppi_fused_staged(*args, **kw)
        chain = lambda: mc.run_mppi(*args, **kw)
        first_f, first_c = fused(), chain()                      # the untimed warm-up of this shape, and the pair whose bytes are compared
        torch.cuda.synchronize()
        same = bool(torch.equal(first_f["pos"].view(torch.uint8), first_c["pos"].view(torch.uint8)))
        clr = first_f["clearance"].double()
        t_f, t_c = [], []
        for _ in range(REPS):
            torch.cuda.synchronize(); ms, _o = event_ms(fused); t_f.append(ms)
            torch.cuda.synchronize(); ms, _o = event_ms(chain); t_c.append(ms)
        spread = lambda t: float((np.max(t) - np.min(t)) / np.median(t))
        row = dict(what=f"run_mppi_fused_staged (1 launch) vs run_mppi with smoother + mixer ({3 * CYCLES} launches)", dtype=dtype, drones=B, samples=S,
                   iters=ITERS, horizon=N, spheres=K, cycles=CYCLES, substeps=SUBSTEPS, reps=REPS, fused_ms_median=float(np.median(t_f)),
                   fused_ms_min=float(np.min(t_f)), fused_spread=spread(t_f), chain_ms_median=float(np.median(t_c)), chain_ms_min=float(np.min(t_c)),
                   chain_spread=spread(t_c), ratio_median=float(np.median(t_f) / np.median(t_c)), same_position_bytes=same,
                   clearance_min=float(clr.min()), clearance_median=float(clr.median()), drones_inside_a_sphere=int((clr < 0).sum()))
        results.append(row); print(json.dumps(row), flush=True)
        assert same, "the one launch and the chain disagree"

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
print("wrote", OUT)
