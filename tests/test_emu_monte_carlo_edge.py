"""CPU suite: se3mpc_monte_carlo_edge_* / ClosedLoopMonteCarlo.run_edge_fused -- the one-launch Monte-Carlo on the reference's edge loop (latency
buffer -> OnboardController -> simulator) -- on the product kernels compiled for the host (tests/emu): the checks of
tests/monte_carlo_edge_checks.py, and the host logic of run_edge_fused on recorded library calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import build_emu  # noqa: E402
from numpy_backend import TorchCpuBackend  # noqa: E402

from dart_planner_amd import capi  # noqa: E402
from dart_planner_amd.ops import Ops  # noqa: E402
import parity_checks as pc  # noqa: E402
import monte_carlo_edge_checks as ec  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), dt)


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", ec.SHAPES)
@pytest.mark.parametrize("substeps", ec.SUBSTEPS)
def test_chain_conditions_are_not_vacuous(emu_ops, dt, N, B, substeps):
    ec.check_not_vacuous(harness(emu_ops, dt), N, B, substeps)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", ec.SHAPES)
@pytest.mark.parametrize("substeps", ec.SUBSTEPS)
@pytest.mark.parametrize("depth", ec.DEPTHS)
def test_one_launch_equals_the_chain_byte_for_byte(emu_ops, dt, N, B, substeps, depth):
    ec.check_equals_chain(harness(emu_ops, dt), N, B, depth, substeps, last_plan=depth == 2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", ec.SHAPES)
@pytest.mark.parametrize("wind", [None, "shared"])
def test_one_launch_equals_the_chain_without_and_with_shared_wind(emu_ops, dt, N, B, wind):
    ec.check_equals_chain(harness(emu_ops, dt), N, B, 5, 4, wind=wind)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,B", ec.SHAPES)
@pytest.mark.parametrize("depth", [1, 5])
def test_a_second_launch_continues_the_first(emu_ops, dt, N, B, depth):
    ec.check_run_continues(harness(emu_ops, dt), N, B, depth, 4)


@pytest.mark.parametrize("dt", DTYPES)
def test_argument_rules(emu_ops, dt):
    ec.check_argument_rules(harness(emu_ops, dt))


# ---- host logic of run_edge_fused: the library calls are recorded, not made, on zero-filled buffers
def recorded(ops, monkeypatch, overflow=0):
    import torch
    calls = []
    monkeypatch.setattr(ops.lib, "call", lambda base, suf, *args, params=None: calls.append(f"{base}_{suf}"))
    monkeypatch.setattr(ops.lib, "loop_call", lambda base, suf, *args: calls.append(f"{base}_{suf}"))
    for name in ("controller_reset", "onboard_reset", "latency_reset"):
        monkeypatch.setattr(ops.lib, name, lambda *args, name=name: calls.append(name))
    monkeypatch.setattr(ops.be, "empty", lambda shape, kind: torch.full(shape, overflow if kind == "i32" else 0, dtype=ops.be._dt[kind]))
    return calls


def edge_mc(ops):
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    B = 2
    mc = ClosedLoopMonteCarlo(ops, Params.reference_defaults(horizon=6))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    return mc, (z(B, 3), z(B, 3), torch.ones(B, 3, dtype=torch.float64), 3, 2, 0.01)


@pytest.mark.parametrize("depth", [0, 1, 5])
def test_run_edge_fused_resets_its_records_and_launches_once(emu_ops, monkeypatch, depth):
    mc, args = edge_mc(emu_ops)                                           # (the default parameters: before the calls are recorded)
    onboard = emu_ops.lib.onboard_default_params()
    calls = recorded(emu_ops, monkeypatch)
    out = mc.run_edge_fused(*args, latency_depth=depth, onboard=onboard, want_last_plan=depth == 1)
    assert calls == ["onboard_reset"] + ["latency_reset"] * (depth > 0) + ["monte_carlo_edge_f64"]
    assert sorted(out) == sorted(["pos", "vel", "att", "omega", "time", "onboard_state", "latency", "zero_thrust_steps", "logs", "last_plan"])
    assert out["logs"] == [] and out["latency"]["depth"] == depth and (out["latency"]["ring"] is None) == (depth == 0)
    assert tuple(out["onboard_state"].shape) == (2, 14) and not out["zero_thrust_steps"].any()
    assert (out["last_plan"] is None) == (depth != 1)
    if depth == 1:
        assert sorted(out["last_plan"]) == ["accelerations", "info", "overflowed", "x"] and tuple(out["last_plan"]["x"].shape) == (2, 54)


def test_run_edge_fused_repeats_an_overflowed_run_with_the_chain(emu_ops, monkeypatch):
    import torch
    mc, args = edge_mc(emu_ops)
    onboard, wind = emu_ops.lib.onboard_default_params(), torch.ones(3, dtype=torch.float64)
    calls = recorded(emu_ops, monkeypatch, overflow=1)
    seen = {}
    monkeypatch.setattr(mc, "run_edge", lambda *a, **kw: seen.update(args=a, kw=kw) or "chain")
    assert mc.run_edge_fused(*args, latency_depth=3, onboard=onboard, wind=wind) == "chain"
    assert calls[-1] == "monte_carlo_edge_f64" and calls.count("monte_carlo_edge_f64") == 1
    assert all(a is b for a, b in zip(seen["args"], args)) and len(seen["args"]) == len(args)
    assert seen["kw"] == dict(latency_depth=3, onboard=onboard, wind=wind) and seen["kw"]["onboard"] is onboard and seen["kw"]["wind"] is wind


def test_monte_carlo_edge_checks_its_operands_before_any_call(emu_ops, monkeypatch):
    import torch
    mc, (p0, v0, goal, cycles, substeps, sim_dt) = edge_mc(emu_ops)
    ops = emu_ops
    op, st, buf = ops.lib.onboard_default_params(), ops.onboard_state(2), ops.latency_buffer(2, 3, "f64")
    time, z = torch.zeros(2, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    calls = recorded(ops, monkeypatch)
    good = dict(onboard_state=st, buf=buf, time=time, pos=p0, vel=v0, att=z, omega=z.clone(), goal=goal)
    bad = [dict(onboard_state=torch.zeros(2, 12, dtype=torch.float64)), dict(buf=dict(buf, ring=torch.zeros(3, 12, 3, dtype=torch.float64))),
           dict(buf=dict(buf, depth=1001)), dict(time=torch.zeros(2, dtype=torch.float32)), dict(vel=torch.zeros(3, 3, dtype=torch.float64)),
           dict(goal=torch.zeros(2, 3, dtype=torch.float32)), dict(wind=torch.zeros(2, dtype=torch.float64)),
           dict(zero_thrust_steps=torch.zeros(2, dtype=torch.int64))]
    for change in bad:
        kw = dict(good, **change)
        more = {k: kw.pop(k) for k in ("wind", "zero_thrust_steps") if k in kw}
        with pytest.raises(ValueError):
            ops.monte_carlo_edge(mc.params, op, mc.simulator, kw["onboard_state"], kw["buf"], kw["time"], kw["pos"], kw["vel"], kw["att"], kw["omega"],
                                 kw["goal"], cycles, substeps, sim_dt, **more)
    assert calls == []


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_equals_chain_with_a_different_constant_in_every_block(emu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    ec.check_equals_chain(harness(emu_ops, dt), L["N"], L["B"], 2, L["substeps"], last_plan=True, cycles=L["cycles"], blocks=ps.loop_blocks(L["N"]))
