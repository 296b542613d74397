"""CPU: dart_planner_amd/csrc/mppi_moving.hip and mppi_closed_loop_moving.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.
Every instantiation keeps its registers (no VGPR spills, no scratch, no AGPRs): mppi_moving_kernel within the four-wavefronts-per-SIMD
budget of mppi_kernel, mppi_closed_loop_moving_kernel within the LoopWaves<R> budgets of mppi_closed_loop_kernel (float32 three wavefronts
per SIMD, float64 two).  Register metadata only.  The counts printed here are the ones DESIGN.md 5.8f quotes."""
import pytest

from isa_checks import compile_isa, kernel_stats


def _report(n, s):
    print(f"{n}: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}")
    assert s.get("vgpr_spill") == 0 and s["scratch"] == 0 and s["agpr"] == 0, (n, s)


def test_moving_planner_keeps_its_registers(tmp_path_factory):
    st = kernel_stats(compile_isa("mppi_moving", tmp_path_factory), "mppi_moving_kernel")
    assert sorted(t for t in "fd" for n in st if f"mppi_moving_kernelI{t}E" in n) == ["d", "f"] and len(st) == 2, sorted(st)
    for n, s in sorted(st.items()):
        _report(n, s)
        assert s["vgpr"] <= 128 and s["occupancy"] >= 4, (n, s)            # __launch_bounds__(256, 4): four wavefronts per SIMD


def test_moving_closed_loop_keeps_the_loop_budgets(tmp_path_factory):
    st = kernel_stats(compile_isa("mppi_closed_loop_moving", tmp_path_factory), "mppi_closed_loop_moving_kernel")
    waves = {"f": 3, "d": 2}                                                 # LoopWaves<R> of mppi_closed_loop_kernel
    for t, w in waves.items():
        names = [n for n in st if f"mppi_closed_loop_moving_kernelI{t}E" in n]
        assert len(names) == 1, sorted(st)
        s = st[names[0]]
        _report(names[0], s)
        assert s["occupancy"] >= w and s["vgpr"] <= 512 // w, (names[0], s, w)
