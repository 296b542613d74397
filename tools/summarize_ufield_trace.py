"""Reduce the `rocprofv3 --kernel-trace --stats` table of `tools/gpu_probe_ufield.py --regions-only` to the share each kernel of
se3mpc_ufield_regions has in the call, and the share of the three labelling launches (tiles, faces, flatten).

`python tools/summarize_ufield_trace.py <directory with *kernel_stats.csv> [out.json]` (default profiles/ufield_regions_kernels.json)."""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ufield_regions_kernels.json")
REGION_KERNELS = ("label_tiles", "merge_faces", "flatten_facts", "region_count", "region_scan", "region_scatter", "region_sum", "region_finish")
LABELLING = REGION_KERNELS[:3]
rows = {}
for path in glob.glob(os.path.join(src, "**", "*kernel_stats.csv"), recursive=True):
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r"ufield_(\w+)_kernel", r["Name"])
            if m and m.group(1) in REGION_KERNELS:
                k = rows.setdefault(m.group(1), dict(calls=0, total_ns=0))
                k["calls"] += int(r["Calls"])
                k["total_ns"] += int(r["TotalDurationNs"])
total = sum(k["total_ns"] for k in rows.values())
for name, k in rows.items():
    k["share"] = k["total_ns"] / total
    k["average_us"] = k["total_ns"] / k["calls"] / 1e3
result = dict(kernels={n: rows[n] for n in REGION_KERNELS if n in rows}, labelling_share=sum(rows[n]["total_ns"] for n in LABELLING if n in rows) / total if total else None,
              note="three fields (fresh, 200 stamps, 4096 stamps) x 5 extractions at 200 x 200 x 40, kernel time under the tracer")
with open(out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result, indent=1))
