"""CPU: dart_planner_amd/csrc/mppi_closed_loop_staged.hip compiled to gfx950 ISA with the Makefile's own HIPFLAGS.  Exactly the six
instantiations of mppi_closed_loop_staged_kernel exist -- float32 / float64 x (smoother, mixer, both) --, each spills no vector register, uses
no scratch memory and has the occupancy its __launch_bounds__ declares (StagedLoopWaves).  Resource metadata only.  The counts printed here
are the ones DESIGN.md 5.8d quotes."""
import os
import re

import pytest

from isa_checks import CSRC, compile_isa, kernel_stats

SRC = os.path.join(CSRC, "mppi_closed_loop_staged.hip")
VARIANT = r"kernelI([fd])Lb([01])ELb([01])E"


def declared_waves():
    """Wavefronts per SIMD the source declares: {(type, smoother, mixer): n} from StagedLoopWaves and its specialisations."""
    src = open(SRC).read()
    assert re.search(r"__launch_bounds__\(kBlock, \(StagedLoopWaves<R, SMOOTH, MIX>::value\)\)\s*mppi_closed_loop_staged_kernel", src), "the kernel's launch bounds"
    gen = re.search(r"struct StagedLoopWaves \{ static constexpr int value = (\d+); \};", src)
    dbl = re.search(r"struct StagedLoopWaves<double, SMOOTH, MIX> \{ static constexpr int value = (\d+); \};", src)
    assert gen and dbl, "StagedLoopWaves not found"
    waves = {(t, s, m): int((gen if t == "f" else dbl).group(1)) for t in "fd" for s, m in ("10", "01", "11")}
    for t, s, m, n in re.findall(r"struct StagedLoopWaves<(float|double), (true|false), (true|false)> \{ static constexpr int value = (\d+); \};", src):
        waves[(t[0], "1" if s == "true" else "0", "1" if m == "true" else "0")] = int(n)
    return waves


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa("mppi_closed_loop_staged", tmp_path_factory)


def test_every_instantiation_keeps_its_registers(isa):
    found = kernel_stats(isa, "mppi_closed_loop_staged_kernel")
    waves = declared_waves()
    variants = sorted(re.search(VARIANT, n).groups() for n in found)
    assert variants == sorted((t, s, m) for t in "fd" for s, m in ("10", "01", "11")), sorted(found)
    for n, s in sorted(found.items()):
        key = re.search(VARIANT, n).groups()
        t, sm, mx = key
        print(f"mppi_closed_loop_staged_kernel<{'float' if t == 'f' else 'double'}, smoother={sm}, mixer={mx}>: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, "
              f"scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']} (declared {waves[key]})")
        assert s.get("vgpr_spill") == 0 and s["scratch"] == 0, (n, s)
        assert s["occupancy"] == waves[key], (n, s, waves[key])
