"""Developer probe (GPU box): what the actuator stage (MotorMixer + motor model + realised wrench) costs per drone-step.

4096 drones x 330 steps on one plan per drone (30 rows), float32 and float64, HIP events, warm (60 ms of untimed load first, as bench.py's
warm_device), alternating, median and minimum of 10:

* se3mpc_closed_loop_actuated_* without the smoother against se3mpc_closed_loop_* at the same shape;
* the same with the smoother against se3mpc_closed_loop_smoothed_*;
* the per-step chain se3mpc_control_plan_* -> se3mpc_mixer_mix_* -> se3mpc_mixer_readback_* -> se3mpc_simulator_step_* (4 x 330 launches).

closed_loop.hip and smoother.hip are the parent commit's files unchanged, so the two plain kernels of this build are the parent commit's.

`python tools/gpu_probe_mixer.py [out.json]` (default profiles/mixer_launch.json)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dart_planner_amd.capi import SmootherParams  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mixer_launch.json")
ops = Ops(); dev = ops.be.device
B, NSTEPS, N, SIM_DT, REPS, WARM_MS = 4096, 330, 30, 0.001, 10, 60.0
cp, sp, smp, mp = ops.lib.controller_default_params(), ops.lib.simulator_default_params(), SmootherParams.reference_defaults(), ops.lib.mixer_default_params()
results = []


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3


def warm(fn):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < WARM_MS:
        fn(); torch.cuda.synchronize()


for name, dtype in (("float32", torch.float32), ("float64", torch.float64)):
    g = torch.Generator(device=dev); g.manual_seed(7)
    k = torch.arange(N, dtype=torch.float64, device=dev)
    ts = 5.0 + k * 0.011
    start = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev) + 0.2 * torch.randn(B, 1, 3, dtype=dtype, device=dev, generator=g)
    V = (0.5 * torch.randn(B, 1, 3, dtype=dtype, device=dev, generator=g)).expand(B, N, 3).contiguous()
    P = (start + V * (k * 0.011).to(dtype)[None, :, None]).contiguous()
    A = torch.zeros(B, N, 3, dtype=dtype, device=dev)
    pos0, vel0 = P[:, 0].contiguous(), V[:, 0].contiguous()
    zeros = torch.zeros(B, 3, dtype=dtype, device=dev)
    plan = (ts, P, V, A)

    def fresh(smoothed):
        s = dict(st=ops.controller_state(cp, B), mx=ops.mixer_state(B), sm=None, time=torch.full((B,), 5.0, dtype=torch.float64, device=dev), pos=pos0.clone(),
                 vel=vel0.clone(), att=zeros.clone(), om=zeros.clone())
        if smoothed:
            s["sm"] = ops.smoother_state(B)
            ops.smoother_update(smp, s["sm"], s["time"], *plan)
        return s

    fl = lambda s: (s["time"], s["pos"], s["vel"], s["att"], s["om"])
    actuated = lambda s: ops.closed_loop_actuated(mp, cp, sp, s["st"], s["mx"], *fl(s), *plan, nsteps=NSTEPS, sim_dt=SIM_DT, smoother=smp if s["sm"] is not None else None,
                                                  smoother_state=s["sm"])
    plain = lambda s: ops.closed_loop(cp, sp, s["st"], *fl(s), *plan, nsteps=NSTEPS, sim_dt=SIM_DT, stop_at_plan_end=False)
    smoothed_plain = lambda s: ops.closed_loop_smoothed(smp, cp, sp, s["st"], s["sm"], *fl(s), *plan, nsteps=NSTEPS, sim_dt=SIM_DT)

    def chain(s):
        for _ in range(NSTEPS):
            cmd = ops.control_plan(cp, s["st"], s["time"], s["time"], s["pos"], s["vel"], s["att"], s["om"], *plan)
            mix = ops.mixer_mix(mp, cmd["thrust"], cmd["torque"], s["mx"])
            w = ops.mixer_readback(mp, mix["pwm"], want=("wrench",))["wrench"]
            ops.simulator_step(sp, *fl(s), w[:, 0].contiguous(), w[:, 1:4].contiguous(), SIM_DT)

    for what, with_sm, new, old in (("se3mpc_closed_loop_actuated (no smoother) vs se3mpc_closed_loop", False, actuated, plain),
                                    ("se3mpc_closed_loop_actuated (smoother) vs se3mpc_closed_loop_smoothed", True, actuated, smoothed_plain),
                                    ("per-step chain control_plan + mixer_mix + mixer_readback + simulator_step vs se3mpc_closed_loop_actuated (no smoother)", False, chain, actuated)):
        warm(lambda: old(fresh(with_sm)))
        new(fresh(with_sm)); torch.cuda.synchronize()
        t_n, t_o = [], []
        for _ in range(REPS if new is not chain else 3):
            s = fresh(with_sm); torch.cuda.synchronize(); t_n.append(event_us(lambda: new(s)))
            s = fresh(with_sm); torch.cuda.synchronize(); t_o.append(event_us(lambda: old(s)))
        row = dict(what=what, dtype=name, drones=B, steps=NSTEPS, plan_rows=N, new_us_median=float(np.median(t_n)), new_us_min=float(np.min(t_n)),
                   old_us_median=float(np.median(t_o)), old_us_min=float(np.min(t_o)), ratio_median=float(np.median(t_n) / np.median(t_o)),
                   new_ns_per_drone_step=float(np.median(t_n) * 1e3 / (B * NSTEPS)), old_ns_per_drone_step=float(np.median(t_o) * 1e3 / (B * NSTEPS)))
        results.append(row); print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
print("wrote", OUT)
