"""CPU: dart_planner_amd/csrc/mppi_closed_loop.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.  Both instantiations of the
closed-loop MPPI kernel keep their registers (no VGPR spills, no scratch, no AGPRs) at the occupancy their __launch_bounds__ declare, and
the file is built from the shared device headers: it defines none of their functions itself.  The counts printed here are the ones
DESIGN.md 5.8c quotes."""
import os
import re

import pytest

from isa_checks import CSRC, compile_isa, kernel_stats

SRC = os.path.join(CSRC, "mppi_closed_loop.hip")


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
    return compile_isa("mppi_closed_loop", tmp_path_factory)


def test_closed_loop_mppi_kernels_keep_their_registers(isa):
    st = kernel_stats(isa, "mppi_closed_loop_kernel")
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
    for fn in ("weighted_pass", "draw", "roll_step", "sample_cost", "philox4x32_10", "control_step", "sample_plan", "simulator_step",
               "flight_step", "fly_steps", "drone_block", "drone_load", "drone_store", "lds_view", "nominal_update", "check_mppi_args", "fail"):
        assert not re.search(rf"\b(void|double|R|int|Roll<R>|DroneBlock<R>|LdsView<R>)\s+{fn}\s*\(", src), f"{fn} is defined in mppi_closed_loop.hip"
        assert re.search(rf"\b{fn}\b", open(os.path.join(CSRC, "mppi_device.hpp")).read() + open(os.path.join(CSRC, "closed_loop_device.hpp")).read())
