"""CPU: dart_planner_amd/csrc/edge_loop.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.  The edge-loop kernels (the record reset, and
latency push, onboard control and the edge loop in both precisions) need neither spilled vector registers nor scratch memory, and the edge loop
spills no more than closed_loop_kernel of closed_loop.hip in the same build.  Resource metadata only.  The counts printed here are the ones
DESIGN.md 5.7f quotes."""
import pytest

from isa_checks import compile_isa, kernel_stats


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa("edge_loop", tmp_path_factory)


@pytest.fixture(scope="module")
def isa_closed_loop(tmp_path_factory):
    return compile_isa("closed_loop", tmp_path_factory)


def show(name, s):
    print(f"{name}: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}")


def test_edge_kernels_keep_their_registers(isa):
    found = {}
    for key, count in (("words_reset_kernel", 1), ("latency_push_kernel", 2), ("onboard_control_kernel", 2), ("edge_loop_kernel", 2)):
        st = kernel_stats(isa, key)
        assert len(st) == count, (key, sorted(st))
        found.update(st)
    for n, s in sorted(found.items()):
        show(n, s)
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0, (n, s)


def test_edge_loop_spills_no_more_than_the_plain_loop(isa, isa_closed_loop):
    plain = {n: s for n, s in kernel_stats(isa_closed_loop, "closed_loop_kernel").items() if "mppi" not in n}
    edge = kernel_stats(isa, "edge_loop_kernel")
    assert len(plain) == 2 and len(edge) == 2, (sorted(plain), sorted(edge))
    for t in "fd":
        (pn, p), = [(n, s) for n, s in plain.items() if f"closed_loop_kernelI{t}E" in n]
        (en, e), = [(n, s) for n, s in edge.items() if f"edge_loop_kernelI{t}E" in n]
        show(pn, p); show(en, e)
        assert e["vgpr_spill"] <= p["vgpr_spill"], (en, e, pn, p)
