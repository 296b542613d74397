"""Developer probe (GPU box): what the uncertainty field costs at the mission planner's default grid -- exploration_radius
50 m at 0.5 m: 200 x 200 x 40 = 1.6 M voxels.  One process, HIP events, warm (60 ms of untimed load first), median and minimum of 10:

* one stamp of radius 3 m (what the mission planner does per global replan) and 4096 stamps in one launch (a swarm on one shared scene);
* 4096 point updates; the statistics;
* the region extraction on a fresh field (one region of 1.6 M voxels), after 200 random stamps and after 4096 random stamps.

`python tools/gpu_probe_ufield.py [out.json]` (default profiles/ufield_launch.json).  With `--regions-only` it runs the three region
extractions five times each and times nothing: the run to put under `rocprofv3 --kernel-trace --stats`, whose per-kernel table gives the
labelling kernels' share of the call (tools/summarize_ufield_trace.py)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REGIONS_ONLY = "--regions-only" in sys.argv
OUT = args[0] if args else os.path.join(ROOT, "profiles", "ufield_launch.json")
ops = Ops(); dev = ops.be.device
N, RES, ORIGIN, MAX_REGIONS, REPS, WARM_MS = (200, 200, 40), 0.5, (-50.0, -50.0, 0.0), 4096, 10, 60.0
results = []


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3


def warm(fn):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < WARM_MS:
        fn(); torch.cuda.synchronize()


def timed(what, fn, reset=None, **more):
    """median / minimum of REPS; `reset` (untimed) puts the field back before every repetition"""
    warm(fn)
    t = []
    for _ in range(REPS):
        if reset is not None:
            reset()
        torch.cuda.synchronize()
        t.append(event_us(fn))
    row = dict(what=what, grid=list(N), us_median=float(np.median(t)), us_min=float(np.min(t)), **more)
    results.append(row); print(json.dumps(row), flush=True)


u = torch.empty(N, dtype=torch.float64, device=dev)
c = torch.empty(N, dtype=torch.float64, device=dev)
desc = ops.ufield_desc(u, c, ORIGIN, RES)
ws = ops.ufield_workspace(N, MAX_REGIONS)
labels = torch.empty(N, dtype=torch.int32, device=dev)
fill = lambda: ops.ufield_fill(desc)
g = torch.Generator(device=dev); g.manual_seed(11)
lo, hi = torch.tensor(ORIGIN, dtype=torch.float64, device=dev), torch.tensor([50.0, 50.0, 20.0], dtype=torch.float64, device=dev)


def stamps(S, radius, factor):
    centres = (lo + (hi - lo) * torch.rand(S, 3, dtype=torch.float64, device=dev, generator=g)).contiguous()
    r = torch.full((S,), radius, dtype=torch.float64, device=dev)
    return centres, r, torch.full((S,), int(radius / RES), dtype=torch.int32, device=dev), torch.full((S,), factor, dtype=torch.float64, device=dev)


one, swarm, two_hundred = stamps(1, 3.0, 0.2), stamps(4096, 3.0, 0.2), stamps(200, 3.0, 0.5)
swarm_half = (swarm[0], swarm[1], swarm[2], torch.full((4096,), 0.5, dtype=torch.float64, device=dev))
regions = lambda: ops.ufield_regions(desc, 0.7, 1.0, MAX_REGIONS, workspace=ws, labels=labels)
fields = (("fresh field", lambda: fill()), ("after 200 random stamps (radius 3 m, factor 0.5)", lambda: (fill(), ops.ufield_stamp(desc, *two_hundred))),
          ("after 4096 random stamps (radius 3 m, factor 0.5)", lambda: (fill(), ops.ufield_stamp(desc, *swarm_half))))

if REGIONS_ONLY:
    for what, prepare in fields:
        prepare()
        for _ in range(5):
            out = regions()
        torch.cuda.synchronize()
        print(what, out["counts"].tolist(), flush=True)
    sys.exit(0)

fill(); torch.cuda.synchronize()
timed("fill", fill)
timed("one stamp, radius 3 m", lambda: ops.ufield_stamp(desc, *one), stamps=1)
timed("4096 stamps in one launch, radius 3 m", lambda: ops.ufield_stamp(desc, *swarm), reset=fill, stamps=4096)
pts = (lo + (hi - lo) * torch.rand(4096, 3, dtype=torch.float64, device=dev, generator=g)).contiguous()
pts[:512] = pts[0] + 0.01 * torch.rand(512, 3, dtype=torch.float64, device=dev, generator=g)        # 512 points around one spot
unc = torch.rand(4096, dtype=torch.float64, device=dev, generator=g)
timed("4096 point updates (512 of them around one spot)", lambda: ops.ufield_update_points(desc, pts, unc, None, 0.1, ws), points=4096)
timed("statistics", lambda: ops.ufield_statistics(desc, 0.7, workspace=ws))
for what, prepare in fields:
    prepare()
    out = regions(); torch.cuda.synchronize()
    written, found = out["counts"].tolist()
    timed("regions, " + what, regions, regions_written=written, regions_found=found, max_regions=MAX_REGIONS,
          largest_region_voxels=int(round(float(out["regions"][:written, 10].max()) / RES ** 3)) if written else 0)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
print("wrote", OUT)
