"""CPU: dart_planner_amd/csrc/mppi.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS: every MPPI kernel instantiation keeps
its registers (no VGPR spills, no scratch, no AGPRs) within the four-wavefronts-per-SIMD budget its __launch_bounds__ asks for.
The VGPR counts printed here are the ones DESIGN.md 5.8 quotes."""
import pytest

from isa_checks import compile_isa, kernel_stats


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa("mppi", tmp_path_factory)


def test_mppi_kernels_keep_their_registers(isa):
    st = kernel_stats(isa, "mppi")
    names = sorted(st)
    assert any("mppi_kernelIf" in n for n in names) and any("mppi_kernelId" in n for n in names), names
    assert any("mppi_samples_kernelIf" in n for n in names) and any("mppi_samples_kernelId" in n for n in names), names
    for n in names:
        s = st[n]
        print(f"{n}: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}")
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0 and s["agpr"] == 0, (n, s)
        if "mppi_kernel" in n and "samples" not in n:
            assert s["vgpr"] <= 128 and s["occupancy"] >= 4, (n, s)            # __launch_bounds__(256, 4): four wavefronts per SIMD
