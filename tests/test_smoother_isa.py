"""CPU: dart_planner_amd/csrc/smoother.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.  The four smoother kernels (reset, update,
desired and the smoothed closed loop, the last three in both precisions) need neither spilled vector registers nor scratch memory, and the
smoothed loop spills no more than closed_loop_kernel of closed_loop.hip in the same build.  Resource metadata only.  The counts printed
here are the ones DESIGN.md 5.7c quotes."""
import pytest

from isa_checks import compile_isa, kernel_stats


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa("smoother", tmp_path_factory)


@pytest.fixture(scope="module")
def isa_closed_loop(tmp_path_factory):
    return compile_isa("closed_loop", tmp_path_factory)


def show(name, s):
    print(f"{name}: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}")


def test_smoother_kernels_keep_their_registers(isa):
    found = {}
    for key, count in (("smoother_reset_kernel", 1), ("smoother_update_kernel", 2), ("smoother_desired_kernel", 2), ("closed_loop_smoothed_kernel", 2)):
        st = kernel_stats(isa, key)
        assert len(st) == count, (key, sorted(st))
        found.update(st)
    for n, s in sorted(found.items()):
        show(n, s)
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0, (n, s)


def test_smoothed_loop_spills_no_more_than_the_plain_loop(isa, isa_closed_loop):
    plain = {n: s for n, s in kernel_stats(isa_closed_loop, "closed_loop_kernel").items() if "mppi" not in n}
    smooth = kernel_stats(isa, "closed_loop_smoothed_kernel")
    assert len(plain) == 2 and len(smooth) == 2, (sorted(plain), sorted(smooth))
    for t in "fd":
        (pn, p), = [(n, s) for n, s in plain.items() if f"closed_loop_kernelI{t}E" in n]
        (sn, s), = [(n, s) for n, s in smooth.items() if f"closed_loop_smoothed_kernelI{t}E" in n]
        show(pn, p); show(sn, s)
        assert s["vgpr_spill"] <= p["vgpr_spill"], (sn, s, pn, p)
