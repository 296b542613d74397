"""CPU: the kernels of tracked spheres and shared plans (dart_planner_amd/csrc/mppi_tracks.hip, mppi_closed_loop_tracks.hip and the
shared-plans part of mppi_swarm.hip) compiled to gfx950 ISA with the Makefile's own HIPFLAGS keep their registers (no VGPR spills, no
scratch, no AGPRs) within their launch bounds, and the tracked form of the context (an empty base of Ctx, a third template switch of
mppi_device.hpp's functions) left every MPPI kernel that was there before exactly as it was: the register statistics below were read
off the commit before the tracked form existed.  Register metadata only.  The counts printed here are the ones DESIGN.md 5.8h quotes."""
import re

import pytest

from isa_checks import compile_isa, kernel_stats

# file -> kernel<template arguments> -> (VGPRs, AGPRs, scratch bytes, occupancy, VGPR spills), before mppi_device.hpp learnt of tracks
BEFORE = {
    "mppi": {
        "mppi_kernel<d>": (118, 0, 0, 4, 0),
        "mppi_kernel<f>": (83, 0, 0, 5, 0),
        "mppi_samples_kernel<d>": (110, 0, 0, 4, 0),
        "mppi_samples_kernel<f>": (58, 0, 0, 8, 0),
    },
    "mppi_closed_loop": {
        "mppi_closed_loop_kernel<d>": (234, 0, 0, 2, 0),
        "mppi_closed_loop_kernel<f>": (139, 0, 0, 3, 0),
    },
    "mppi_closed_loop_edge": {
        "mppi_closed_loop_edge_kernel<d>": (243, 0, 0, 2, 0),
        "mppi_closed_loop_edge_kernel<f>": (144, 0, 0, 3, 0),
    },
    "mppi_closed_loop_moving": {
        "mppi_closed_loop_moving_kernel<d>": (236, 0, 0, 2, 0),
        "mppi_closed_loop_moving_kernel<f>": (141, 0, 0, 3, 0),
    },
    "mppi_closed_loop_staged": {
        "mppi_closed_loop_staged_kernel<dLb0ELb1E>": (256, 5, 0, 1, 0),
        "mppi_closed_loop_staged_kernel<dLb1ELb0E>": (256, 28, 0, 1, 0),
        "mppi_closed_loop_staged_kernel<dLb1ELb1E>": (256, 52, 0, 1, 0),
        "mppi_closed_loop_staged_kernel<fLb0ELb1E>": (156, 0, 0, 3, 0),
        "mppi_closed_loop_staged_kernel<fLb1ELb0E>": (178, 0, 0, 2, 0),
        "mppi_closed_loop_staged_kernel<fLb1ELb1E>": (195, 0, 0, 2, 0),
    },
    "mppi_moving": {
        "mppi_moving_kernel<d>": (120, 0, 0, 4, 0),
        "mppi_moving_kernel<f>": (83, 0, 0, 5, 0),
    },
    "mppi_split": {
        "mppi_split_iter_kernel<d>": (122, 0, 0, 4, 0),
        "mppi_split_iter_kernel<f>": (83, 0, 0, 5, 0),
        "mppi_split_finish_kernel<d>": (106, 0, 0, 4, 0),
        "mppi_split_finish_kernel<f>": (56, 0, 0, 8, 0),
    },
    "mppi_swarm": {
        "swarm_seed_kernel<d>": (8, 0, 0, 8, 0),
        "swarm_seed_kernel<f>": (8, 0, 0, 8, 0),
        "mppi_swarm_cycle_kernel<d>": (207, 0, 0, 2, 0),
        "mppi_swarm_cycle_kernel<f>": (100, 0, 0, 4, 0),
        "swarm_separation_kernel<d>": (24, 0, 0, 8, 0),
        "swarm_separation_kernel<f>": (20, 0, 0, 8, 0),
    },
}
NEW_IN_SWARM = ("swarm_intent_kernel", "mppi_swarm_intent_cycle_kernel")


def _by_name(stats):
    """{kernel<template arguments>: (vgpr, agpr, scratch, occupancy, vgpr_spill)} of isa_checks.kernel_stats' {symbol: dict}."""
    out = {}
    for sym, s in stats.items():
        m = re.search(r"\d+([a-z_]+_kernel)I(.+?)EEv", sym)
        assert m, sym
        out[f"{m.group(1)}<{m.group(2)}>"] = (s["vgpr"], s["agpr"], s["scratch"], s["occupancy"], s.get("vgpr_spill"))
    return out


@pytest.fixture(scope="module")
def swarm_asm(tmp_path_factory):
    return compile_isa("mppi_swarm", tmp_path_factory)


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_the_kernels_that_were_there_compile_as_before(tmp_path_factory, swarm_asm, name):
    asm = swarm_asm if name == "mppi_swarm" else compile_isa(name, tmp_path_factory)
    got = {k: v for k, v in _by_name(kernel_stats(asm, "")).items() if not k.startswith(NEW_IN_SWARM)}
    for k in sorted(got):
        print(k, got[k])
    assert got == BEFORE[name]


def _report(n, s):
    print(f"{n}: {s['vgpr']} VGPRs, {s['agpr']} AGPRs, scratch {s['scratch']} B, {s.get('vgpr_spill', '?')} VGPR spills, occupancy {s['occupancy']}")
    assert s.get("vgpr_spill") == 0 and s["scratch"] == 0 and s["agpr"] == 0, (n, s)


def _both_types(st, kernel):
    names = {t: [n for n in st if f"{kernel}I{t}E" in n] for t in "fd"}
    assert all(len(v) == 1 for v in names.values()), sorted(st)
    return {t: v[0] for t, v in names.items()}


def test_tracks_planner_keeps_its_registers(tmp_path_factory):
    st = kernel_stats(compile_isa("mppi_tracks", tmp_path_factory), "mppi_tracks_kernel")
    assert len(st) == 2, sorted(st)
    for t, n in _both_types(st, "mppi_tracks_kernel").items():
        _report(n, st[n])
        assert st[n]["vgpr"] <= 128 and st[n]["occupancy"] >= 4, (n, st[n])            # __launch_bounds__(256, 4): four wavefronts per SIMD


def test_tracks_closed_loop_keeps_the_loop_budgets(tmp_path_factory):
    st = kernel_stats(compile_isa("mppi_closed_loop_tracks", tmp_path_factory), "mppi_closed_loop_tracks_kernel")
    for t, w in {"f": 3, "d": 2}.items():                                               # the wavefronts per SIMD of the moving loop
        n = _both_types(st, "mppi_closed_loop_tracks_kernel")[t]
        _report(n, st[n])
        assert st[n]["occupancy"] >= w and st[n]["vgpr"] <= 512 // w, (n, st[n], w)


def test_shared_plans_cycle_keeps_the_swarm_budgets(swarm_asm):
    st = kernel_stats(swarm_asm, "mppi_swarm_intent_cycle_kernel")
    for t, w in {"f": 3, "d": 2}.items():                                               # SwarmWaves<R>
        n = _both_types(st, "mppi_swarm_intent_cycle_kernel")[t]
        _report(n, st[n])
        assert st[n]["occupancy"] >= w and st[n]["vgpr"] <= 512 // w, (n, st[n], w)
    seed = kernel_stats(swarm_asm, "swarm_intent_kernel")
    for t, n in _both_types(seed, "swarm_intent_kernel").items():
        _report(n, seed[n])
