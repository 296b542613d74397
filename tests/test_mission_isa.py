"""CPU: dart_planner_amd/csrc/mission.hip and monte_carlo_mission.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.  The mission_goal
kernels use no scratch memory and spill no vector register; every instantiation of monte_carlo_mission_kernel spills no more than
monte_carlo_kernel of the same type and group size in the same build.  Resource metadata only.  The counts printed here are the ones DESIGN.md
5.10 quotes."""
import re

import pytest

from isa_checks import compile_isa, kernel_stats


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    return {name: compile_isa(name, tmp_path_factory) for name in ("mission", "monte_carlo", "monte_carlo_mission")}


def test_mission_goal_kernels_need_no_scratch(listings):
    found = kernel_stats(listings["mission"], "mission_goal_kernel")
    assert sorted(re.search(r"kernelI([fd])E", n).group(1) for n in found) == ["d", "f"], sorted(found)
    for n, s in sorted(found.items()):
        print(f"{n}: {s['vgpr']} VGPRs, scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}")
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0, (n, s)


def test_one_launch_kernel_spills_no_more_than_monte_carlo_kernel(listings):
    variant = lambda n: re.search(r"kernelI([fd])Li(\d+)E", n).groups()
    base = {variant(n): s for n, s in kernel_stats(listings["monte_carlo"], "monte_carlo_kernel").items()}
    found = {variant(n): s for n, s in kernel_stats(listings["monte_carlo_mission"], "monte_carlo_mission_kernel").items()}
    assert sorted(found) == sorted(base) == sorted((t, str(g)) for t in "fd" for g in (8, 16, 32, 64)), (sorted(found), sorted(base))
    for v in sorted(found):
        s, b = found[v], base[v]
        print(f"monte_carlo_mission_kernel<{'float' if v[0] == 'f' else 'double'}, {v[1]}>: {s['vgpr']} VGPRs, scratch {s['scratch']} B, "
              f"{s['vgpr_spill']} VGPR spills, occupancy {s['occupancy']}  (monte_carlo_kernel: {b['vgpr']} VGPRs, scratch {b['scratch']} B, "
              f"{b['vgpr_spill']} spills)")
        assert s["vgpr_spill"] <= b["vgpr_spill"] and s["scratch"] <= b["scratch"], (v, s, b)
        assert s["occupancy"] == b["occupancy"], (v, s, b)
