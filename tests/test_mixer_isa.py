"""CPU: dart_planner_amd/csrc/mixer.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.  The mix, readback and reset kernels need
neither spilled vector registers nor scratch memory.  For the four instantiations of the actuated closed loop (float32 / float64, with and
without the smoother) the counts are printed -- they are the ones DESIGN.md 5.7d quotes -- and, per precision, the form without the
smoother spills no more than the form with it.  Resource metadata only."""
import pytest

from isa_checks import compile_isa, kernel_stats


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa("mixer", tmp_path_factory)


def show(name, s):
    print(f"{name}: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}")


def test_mix_and_readback_kernels_keep_their_registers(isa):
    found = {}
    for key, count in (("mixer_reset_kernel", 1), ("mixer_mix_kernel", 2), ("mixer_readback_kernel", 2)):
        st = kernel_stats(isa, key)
        assert len(st) == count, (key, sorted(st))
        found.update(st)
    for n, s in sorted(found.items()):
        show(n, s)
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0, (n, s)


def test_actuated_loop_without_smoother_spills_no_more_than_with_it(isa):
    loops = kernel_stats(isa, "closed_loop_actuated_kernel")
    assert len(loops) == 4, sorted(loops)
    for n, s in sorted(loops.items()):
        show(n, s)
    for t in "fd":
        (wn, w), = [(n, s) for n, s in loops.items() if f"closed_loop_actuated_kernelI{t}Lb1E" in n]
        (pn, p), = [(n, s) for n, s in loops.items() if f"closed_loop_actuated_kernelI{t}Lb0E" in n]
        assert p["vgpr_spill"] <= w["vgpr_spill"], (pn, p, wn, w)
