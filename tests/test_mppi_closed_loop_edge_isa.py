"""CPU: dart_planner_amd/csrc/mppi_closed_loop_edge.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.  Exactly the float32 and the
float64 instantiation of mppi_closed_loop_edge_kernel exist; each spills no vector register, uses no scratch memory and has the occupancy its
__launch_bounds__ declares (EdgeLoopWaves).  Resource metadata only.  The counts printed here are the ones DESIGN.md 5.8e quotes."""
import os
import re

import pytest

from isa_checks import CSRC, compile_isa, kernel_stats

SRC = os.path.join(CSRC, "mppi_closed_loop_edge.hip")


def declared_waves():
    """Wavefronts per SIMD the source declares per type: {'f': .., 'd': ..} from EdgeLoopWaves."""
    src = open(SRC).read()
    gen = re.search(r"struct EdgeLoopWaves \{ static constexpr int value = (\d+); \};", src)
    dbl = re.search(r"struct EdgeLoopWaves<double> \{ static constexpr int value = (\d+); \};", src)
    assert gen and dbl, "EdgeLoopWaves not found"
    assert re.search(r"__launch_bounds__\(kBlock, EdgeLoopWaves<R>::value\)\s*mppi_closed_loop_edge_kernel", src), "the kernel's launch bounds"
    return {"f": int(gen.group(1)), "d": int(dbl.group(1))}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa("mppi_closed_loop_edge", tmp_path_factory)


def test_both_instantiations_keep_their_registers(isa):
    st = kernel_stats(isa, "mppi_closed_loop_edge_kernel")
    waves = declared_waves()
    variants = sorted(re.search(r"mppi_closed_loop_edge_kernelI([fd])E", n).group(1) for n in st)
    assert variants == ["d", "f"], sorted(st)
    for n, s in sorted(st.items()):
        t = re.search(r"mppi_closed_loop_edge_kernelI([fd])E", n).group(1)
        print(f"mppi_closed_loop_edge_kernel<{'float' if t == 'f' else 'double'}>: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, "
              f"{s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']} (declared {waves[t]})")
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0, (n, s)
        assert s["occupancy"] == waves[t] and s["vgpr"] + s["agpr"] <= 512 // waves[t], (n, s, waves[t])


def test_the_act_phase_is_the_shared_one():
    """The kernel and monte_carlo_edge_kernel call one edge_act: neither file defines it (or the records around it) itself."""
    shared = open(os.path.join(CSRC, "edge_act_device.hpp")).read()
    for fn in ("edge_act", "edge_load", "edge_store"):
        assert re.search(rf"\bvoid\s+{fn}\s*\(", shared), f"{fn} is not defined in edge_act_device.hpp"
    for name in ("mppi_closed_loop_edge.hip", "monte_carlo_edge.hip"):
        src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
        assert re.search(r"#pragma clang fp contract\(off\)\s*#include\s+\"edge_act_device.hpp\"", src), f"{name}: edge_act_device.hpp under contract(off)"
        for fn in ("edge_act", "edge_load", "edge_store", "edge_step", "onboard_step", "hand_over_plan", "clearance_chunk", "weighted_pass"):
            assert not re.search(rf"\bvoid\s+{fn}\s*\(", src) and not re.search(rf"\bdouble\s+{fn}\s*\(", src), f"{fn} is defined in {name}"
        assert not re.search(r"struct\s+(EdgeRecords|EdgeBlock)\b", src), f"{name} defines the records itself"
