"""Developer probe (GPU box): what the reference's edge loop costs per launch, and whether loading the popped ring entry one step ahead shows.

One measurement per invocation, appended to the output file, so that a driver script can give every step a time limit of its own and stop at
the first that fails:

    for step in depth0 depth1 depth5 depth9 depth5_late depth9_late chained5; do
        timeout -k 10 120 python tools/gpu_probe_edge_loop.py $step profiles/edge_loop_launch.json || break
    done

* depthD: se3mpc_edge_loop_* at 4096 drones x 100 steps on one 30-row plan per drone with a latency buffer of D slots (0 = none), float32 and
  float64, HIP events around one launch, warm, median and minimum of 20 launches, each from the same fresh state.
* depthD_late: the same with se3mpc_set_edge_loop_variant(1): every ring entry loaded by the push that pops it.
* chainedD: the same 100 steps as 300 launches (se3mpc_latency_push_* -> se3mpc_onboard_control_* -> se3mpc_simulator_step_*), HIP events around
  the whole chain, median and minimum of 5."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402

STEP = sys.argv[1] if len(sys.argv) > 1 else "depth5"
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "edge_loop_launch.json")
m = re.fullmatch(r"(depth|chained)(\d+)(_late)?", STEP)
assert m, "step: depthD, depthD_late or chainedD"
chained, depth, late = m.group(1) == "chained", int(m.group(2)), bool(m.group(3))
ops = Ops(); dev = ops.be.device
B, NSTEPS, N, SIM_DT = 4096, 100, 30, 0.01
REPS = 5 if chained else 20
op, sp = ops.lib.onboard_default_params(), ops.lib.simulator_default_params()
rows = []


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3


for name, dtype, suf in (("float32", torch.float32, "f32"), ("float64", torch.float64, "f64")):
    g = torch.Generator(device=dev); g.manual_seed(7)
    k = torch.arange(N, dtype=torch.float64, device=dev)
    ts = 100.055 + k * 0.1
    start = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev) + 0.2 * torch.randn(B, 1, 3, dtype=dtype, device=dev, generator=g)
    V = (0.3 * torch.randn(B, 1, 3, dtype=dtype, device=dev, generator=g)).expand(B, N, 3).contiguous()
    P = (start + V * (k * 0.1).to(dtype)[None, :, None]).contiguous()
    A = torch.zeros(B, N, 3, dtype=dtype, device=dev)
    pos0 = P[:, 0].contiguous()
    zeros = torch.zeros(B, 3, dtype=dtype, device=dev)

    def fresh():
        return dict(st=ops.onboard_state(B), buf=ops.latency_buffer(B, depth, suf), fl=(torch.full((B,), 100.0, dtype=torch.float64, device=dev), pos0.clone(),
                                                                                        zeros.clone(), zeros.clone(), zeros.clone()))

    def one_launch(s):
        ops.edge_loop(op, sp, s["st"], s["buf"], *s["fl"], ts, P, V, A, nsteps=NSTEPS, sim_dt=SIM_DT)

    def chain(s):
        for _ in range(NSTEPS):
            d = ops.latency_push(s["buf"], *s["fl"])
            cmd = ops.onboard_control(op, s["st"], d["time"], d["pos"], d["att"], d["omega"], ts, P, V, A)
            ops.simulator_step(sp, *s["fl"], cmd["thrust"], cmd["torque"], SIM_DT)

    fn = chain if chained else one_launch
    ops.lib.set_edge_loop_variant(1 if late else 0)
    fn(fresh())                                                  # warm: code objects, allocator pools
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        s = fresh(); torch.cuda.synchronize(); t.append(event_us(lambda: fn(s)))
    ops.lib.set_edge_loop_variant(0)
    row = dict(what="300 chained launches" if chained else "se3mpc_edge_loop, one launch", step=STEP, depth=depth, ring_entry_loaded="by the pop" if late else "one step ahead",
               dtype=name, drones=B, steps=NSTEPS, plan_rows=N, us_median=float(np.median(t)), us_min=float(np.min(t)),
               ns_per_drone_step=float(np.median(t) * 1e3 / (B * NSTEPS)))
    rows.append(row); print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
prev = json.load(open(OUT)) if os.path.exists(OUT) else []
with open(OUT, "w") as f:
    json.dump(prev + rows, f, indent=1)
print("appended", len(rows), "rows to", OUT)
