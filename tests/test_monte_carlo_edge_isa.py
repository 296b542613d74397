"""CPU: dart_planner_amd/csrc/monte_carlo_edge.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.  Every instantiation of
monte_carlo_edge_kernel -- float32 / float64 x the four solver group sizes -- spills no vector register, uses no scratch memory and has the
occupancy its __launch_bounds__ declares (SE3MPC_MC_WAVES = 1 wavefront per SIMD).  Resource metadata only.  The counts printed here are the
ones DESIGN.md 5.7g quotes."""
import re

import pytest

from isa_checks import compile_isa, kernel_stats


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa("monte_carlo_edge", tmp_path_factory)


def test_every_instantiation_keeps_its_registers(isa):
    found = kernel_stats(isa, "monte_carlo_edge_kernel")
    variants = sorted(re.search(r"kernelI([fd])Li(\d+)EE", n).groups() for n in found)
    assert variants == sorted((t, str(g)) for t in "fd" for g in (8, 16, 32, 64)), sorted(found)
    for n, s in sorted(found.items()):
        t, g = re.search(r"kernelI([fd])Li(\d+)EE", n).groups()
        print(f"monte_carlo_edge_kernel<{'float' if t == 'f' else 'double'}, {g}>: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, "
              f"{s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}")
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0, (n, s)
        assert s["occupancy"] == 1, (n, s)
