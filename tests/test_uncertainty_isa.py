"""CPU: every kernel of dart_planner_amd/csrc/uncertainty_field.hip, compiled device-only for gfx950 with the Makefile's flags, needs no
spilled registers and no scratch memory, and its LDS fits a CU's 160 KB.  Read from the code-object metadata of a `hipcc -S`."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_uncertainty_kernels_do_not_spill():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    src = os.path.join(ROOT, "dart_planner_amd", "csrc", "uncertainty_field.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "uncertainty_field.s")
        subprocess.run([hipcc if os.path.exists(hipcc) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "dart_planner_amd", "csrc"), "-Wall", "-Wno-unused-function", "-Wno-pass-failed", "-fno-gpu-rdc",
                        "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", src, "-o", out],
                       check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = [blk for blk in meta.split("  - .agpr_count:")[1:] if "ufield_" in blk]
    names = sorted(re.search(r"\.name:\s+(\S+)", blk).group(1) for blk in kernels)
    assert len(kernels) == 17, names
    for blk in kernels:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, (
            name, get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size"))
        assert get("group_segment_fixed_size") <= 160 * 1024, (name, get("group_segment_fixed_size"))
