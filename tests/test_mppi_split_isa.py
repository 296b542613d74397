"""CPU: dart_planner_amd/csrc/mppi_split.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS: both split-sample MPPI kernels, in
both types, keep their registers (no VGPR spills, no scratch, no AGPRs), and the iteration kernel stays within the
four-wavefronts-per-SIMD budget its __launch_bounds__ asks for -- the budget mppi_kernel is held to (tests/test_mppi_isa.py).
The VGPR counts printed here are the ones DESIGN.md 5.8b quotes."""
import os
import re

import pytest

from isa_checks import CSRC, compile_isa, kernel_stats


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa("mppi_split", tmp_path_factory)


def test_split_kernels_keep_their_registers(isa):
    st = kernel_stats(isa, "mppi_split")
    names = sorted(st)
    for kernel in ("mppi_split_iter_kernelIf", "mppi_split_iter_kernelId", "mppi_split_finish_kernelIf", "mppi_split_finish_kernelId"):
        assert sum(kernel in n for n in names) == 1, (kernel, names)
    assert len(names) == 4, names
    for n in names:
        s = st[n]
        print(f"{n}: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}")
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0 and s["agpr"] == 0, (n, s)
        if "iter_kernel" in n:
            assert s["vgpr"] <= 128 and s["occupancy"] >= 4, (n, s)            # __launch_bounds__(256, 4): four wavefronts per SIMD


def test_the_device_code_is_shared_not_copied():
    """mppi.hip and mppi_split.hip take the sampler, the rollout, the weighted pass, the update, the LDS view and the argument rules from
    csrc/mppi_device.hpp; neither defines them."""
    header = open(os.path.join(CSRC, "mppi_device.hpp")).read()
    for name in ("philox4x32_10", "box_muller", "draw", "roll_step", "sample_cost", "box_clip", "orderable_bits", "lds_layout", "weighted_pass", "lds_view",
                 "nominal_update", "check_mppi_args", "fail"):
        assert re.search(rf"\b{name}\(", header), name
        for f in ("mppi.hip", "mppi_split.hip"):
            src = open(os.path.join(CSRC, f)).read()
            assert '#include "mppi_device.hpp"' in src
            assert not re.search(rf"^(__device__|__host__|inline|static)[^\n;]*\b{name}\(", src, flags=re.M), (f, name)
