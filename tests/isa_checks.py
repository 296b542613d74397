"""What the ISA tests share: a source of dart_planner_amd/csrc compiled to gfx950 ISA with the Makefile's own HIPFLAGS, and the register
statistics of its kernels."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dart_planner_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def makefile_hipflags():
    """HIPFLAGS of csrc/Makefile with its make variables substituted (continuation lines joined)."""
    txt = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", txt, flags=re.M)
    assert m, "HIPFLAGS not found in csrc/Makefile"
    subst = {"ARCH": "gfx950", "ROOT": ROOT, "EXTRA_HIPFLAGS": ""}
    return re.sub(r"\$\((\w+)\)", lambda v: subst[v.group(1)], m.group(1)).split()


def compile_isa(name, tmp_path_factory):
    """The listing of csrc/<name>.hip (skips the calling test where there is no hipcc)."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    src = os.path.join(CSRC, name + ".hip")
    assert os.path.exists(src), f"dart_planner_amd/csrc/{name}.hip is missing"
    out = str(tmp_path_factory.mktemp("isa") / (name + ".s"))
    subprocess.run([HIPCC] + makefile_hipflags() + ["--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    return open(out).read()


def kernel_stats(asm, key):
    """{kernel symbol: {vgpr, agpr, scratch, occupancy, vgpr_spill}} of the kernels whose symbol contains `key`, from the per-function
    comment blocks and the metadata."""
    stats = {}
    for m in re.finditer(rf"^(_Z\w*{key}\w*):[^\n]*$(.*?)^; Occupancy: (\d+)", asm, flags=re.M | re.S):
        body = m.group(2)
        get = lambda k: int(re.findall(rf"; {k}: (\d+)", body)[-1])
        stats[m.group(1)] = dict(vgpr=get("NumVgprs"), agpr=get("NumAgprs"), scratch=get("ScratchSize"), occupancy=int(m.group(3)))
    for m in re.finditer(rf"\.name:\s+(_Z\w*{key}\w*).*?\.vgpr_spill_count:\s+(\d+)", asm, flags=re.S):
        if m.group(1) in stats:
            stats[m.group(1)]["vgpr_spill"] = int(m.group(2))
    return stats
