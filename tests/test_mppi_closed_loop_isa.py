"""CPU: dart_planner_amd/csrc/mppi_closed_loop.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.  Both instantiations of the
closed-loop MPPI kernel keep their registers (no VGPR spills, no scratch, no AGPRs) at the occupancy their __launch_bounds__ declare, and
the file is built from the shared device headers: it defines none of their functions itself.  The counts printed here are the ones
DESIGN.md 5.8c quotes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dart_planner_amd", "csrc")
SRC = os.path.join(CSRC, "mppi_closed_loop.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def makefile_hipflags():
    """HIPFLAGS of csrc/Makefile with its make variables substituted (continuation lines joined)."""
    txt = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", txt, flags=re.M)
    assert m, "HIPFLAGS not found in csrc/Makefile"
    subst = {"ARCH": "gfx950", "ROOT": ROOT, "EXTRA_HIPFLAGS": ""}
    return re.sub(r"\$\((\w+)\)", lambda v: subst[v.group(1)], m.group(1)).split()


def declared_waves():
    """Wavefronts per SIMD the source declares per type: {'f': .., 'd': ..} from LoopWaves."""
    src = open(SRC).read()
    gen = re.search(r"struct LoopWaves \{ static constexpr int value = (\d+); \};", src)
    dbl = re.search(r"struct LoopWaves<double> \{ static constexpr int value = (\d+); \};", src)
    assert gen and dbl, "LoopWaves not found"
    assert re.search(r"__launch_bounds__\(kBlock, LoopWaves<R>::value\)\s*mppi_closed_loop_kernel", src), "the kernel's launch bounds"
    return {"f": int(gen.group(1)), "d": int(dbl.group(1))}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "mppi_closed_loop.s")
    subprocess.run([HIPCC] + makefile_hipflags() + ["--cuda-device-only", "-S", SRC, "-o", out], check=True, capture_output=True)
    return open(out).read()


def kernel_stats(asm):
    stats = {}
    for m in re.finditer(r"^(_Z\w*mppi_closed_loop_kernel\w*):[^\n]*$(.*?)^; Occupancy: (\d+)", asm, flags=re.M | re.S):
        body = m.group(2)
        get = lambda key: int(re.findall(rf"; {key}: (\d+)", body)[-1])
        stats[m.group(1)] = dict(vgpr=get("NumVgprs"), agpr=get("NumAgprs"), scratch=get("ScratchSize"), occupancy=int(m.group(3)))
    for m in re.finditer(r"\.name:\s+(_Z\w*mppi_closed_loop_kernel\w*).*?\.vgpr_spill_count:\s+(\d+)", asm, flags=re.S):
        if m.group(1) in stats:
            stats[m.group(1)]["vgpr_spill"] = int(m.group(2))
    return stats


def test_closed_loop_mppi_kernels_keep_their_registers(isa):
    st = kernel_stats(isa)
    waves = declared_waves()
    by_type = {t: [n for n in st if f"mppi_closed_loop_kernelI{t}E" in n] for t in "fd"}
    assert all(len(v) == 1 for v in by_type.values()), sorted(st)
    for t, (n,) in by_type.items():
        s = st[n]
        print(f"{n}: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}"
              f" (declared {waves[t]})")
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0 and s["agpr"] == 0, (n, s)
        assert s["occupancy"] == waves[t] and s["vgpr"] <= 512 // waves[t], (n, s, waves[t])


def test_the_file_is_built_from_the_shared_headers():
    src = re.sub(r"//[^\n]*", "", open(SRC).read())
    assert re.search(r'#include\s+"mppi_device.hpp"', src) and re.search(r'#include\s+"closed_loop_device.hpp"', src)
    assert src.index('"closed_loop_device.hpp"') < src.index('"mppi_device.hpp"'), "closed_loop_device.hpp first, under contract(off)"
    assert re.search(r"#pragma clang fp contract\(off\)\s*#include\s+\"closed_loop_device.hpp\"", src)
    for fn in ("weighted_pass", "draw", "roll_step", "sample_cost", "philox4x32_10", "control_step", "sample_plan", "simulator_step"):
        assert not re.search(rf"\b(void|double|R|int|Roll<R>)\s+{fn}\s*\(", src), f"{fn} is defined in mppi_closed_loop.hip"
        assert re.search(rf"\b{fn}\b", open(os.path.join(CSRC, "mppi_device.hpp")).read() + open(os.path.join(CSRC, "closed_loop_device.hpp")).read())
