"""CPU suite: se3mpc_mppi_closed_loop_edge_* / Ops.mppi_closed_loop_edge / ClosedLoopMonteCarlo.run_mppi_edge_fused -- the one-launch closed-loop
MPPI Monte-Carlo on the reference's edge loop (latency buffer -> OnboardController -> simulator) -- on the product kernels compiled for the host
(tests/emu): the checks of tests/mppi_closed_loop_edge_checks.py at the shapes the emulation flies in seconds (EMU_SHAPES there, and the full
block once), and the host logic of run_mppi_edge / run_mppi_edge_fused on recorded library calls.  A run takes about two seconds here, so the
depths are swept with per-drone wind and the other two winds at depth 5; the GPU suite flies the full product."""
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
import mppi_closed_loop_edge_checks as ec  # noqa: E402


@pytest.fixture(scope="module")
def emu_ops():
    return Ops(TorchCpuBackend(), capi.Library(build_emu.build()))


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone(), lambda a: a.numpy(), dt)


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.EMU_SHAPES)
@pytest.mark.parametrize("substeps", ec.SUBSTEPS)
def test_chain_conditions_are_not_vacuous(emu_ops, dt, shape, substeps):
    ec.check_not_vacuous(harness(emu_ops, dt), shape, substeps)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.EMU_SHAPES)
@pytest.mark.parametrize("substeps", ec.SUBSTEPS)
@pytest.mark.parametrize("depth", ec.DEPTHS)
def test_one_launch_equals_the_chain_byte_for_byte(emu_ops, dt, shape, substeps, depth):
    ec.check_equals_chain(harness(emu_ops, dt), shape, depth, substeps, last_plan=depth == 2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.EMU_SHAPES)
@pytest.mark.parametrize("substeps", ec.SUBSTEPS)
@pytest.mark.parametrize("wind", [None, "shared"])
def test_one_launch_equals_the_chain_without_and_with_shared_wind(emu_ops, dt, shape, substeps, wind):
    ec.check_equals_chain(harness(emu_ops, dt), shape, 5, substeps, wind=wind)


def test_a_full_block_equals_the_chain_byte_for_byte(emu_ops):
    h = harness(emu_ops, np.float32)
    ec.check_equals_chain(h, ec.SHAPES[1], 5, 4)
    ref = ec.chain(h, ec.SHAPES[1], 5, 4)                           # (the chain's own conditions at this shape, on the run just compared)
    assert all(np.isfinite(v).all() for v in ref.values()) and (ref["zero_thrust_steps"] >= 1).all()
    assert (ref["latency_state"][:, 2] == ec.CYCLES * 4).all() and (ref["latency_state"][:, 0] == 5).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.EMU_SHAPES)
@pytest.mark.parametrize("depth", [1, 5])
def test_one_call_of_four_cycles_equals_four_calls_and_one_plus_three(emu_ops, dt, shape, depth):
    ec.check_cycles_equal_calls(harness(emu_ops, dt), shape, depth, 4)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.EMU_SHAPES)
@pytest.mark.parametrize("depth", [0, 5])
def test_a_slice_of_the_drones_gives_their_rows_and_ring_columns(emu_ops, dt, shape, depth):
    ec.check_slices(harness(emu_ops, dt), shape, depth, 10)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("depth", ec.LONG_DEPTHS)
def test_an_act_phase_of_two_chunks_byte_for_byte(emu_ops, dt, depth):
    ec.check_long_act(harness(emu_ops, dt), ec.EMU_SHAPES[1], depth)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [s for s in ec.EMU_SHAPES if s[2]])
@pytest.mark.parametrize("substeps", ec.SUBSTEPS)
def test_clearance_agrees_with_the_logged_chain(emu_ops, dt, shape, substeps):
    ec.check_clearance(harness(emu_ops, dt), shape, 5, substeps)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ec.EMU_SHAPES)
def test_without_steps_it_is_the_planner_and_touches_no_record(emu_ops, dt, shape):
    ec.check_planner_inside(harness(emu_ops, dt), shape)


@pytest.mark.parametrize("dt", DTYPES)
def test_argument_rules(emu_ops, dt):
    ec.check_argument_rules(harness(emu_ops, dt))


# ---- host logic of run_mppi_edge / run_mppi_edge_fused: the library calls are recorded, not made, on zero-filled buffers
def recorded(ops, monkeypatch):
    import torch
    calls = []
    monkeypatch.setattr(ops.lib, "call", lambda base, suf, *args, params=None: calls.append(f"{base}_{suf}"))
    monkeypatch.setattr(ops.lib, "loop_call", lambda base, suf, *args: calls.append(f"{base}_{suf}"))
    for name in ("controller_reset", "onboard_reset", "latency_reset"):
        monkeypatch.setattr(ops.lib, name, lambda *args, name=name: calls.append(name))
    monkeypatch.setattr(ops.be, "empty", lambda shape, kind: torch.zeros(shape, dtype=ops.be._dt[kind]))
    return calls


def edge_mc(ops):
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    B = 2
    mc = ClosedLoopMonteCarlo(ops, Params.reference_defaults(horizon=6, dt=0.1))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    return mc, (z(B, 3), z(B, 3), torch.ones(B, 3, dtype=torch.float64), 3, 2, 0.01, 64, 2, 1.0, 50.0)


RESULT_KEYS = ["pos", "vel", "att", "omega", "time", "onboard_state", "latency", "zero_thrust_steps", "logs", "U", "cost", "trace", "clearance"]


@pytest.mark.parametrize("depth", [0, 1, 5])
def test_run_mppi_edge_fused_resets_its_records_and_launches_once(emu_ops, monkeypatch, depth):
    import torch
    mc, args = edge_mc(emu_ops)                                           # (the default parameters: before the calls are recorded)
    onboard = emu_ops.lib.onboard_default_params()
    spheres = torch.zeros(3, 4, dtype=torch.float64) if depth == 5 else None
    calls = recorded(emu_ops, monkeypatch)
    out = mc.run_mppi_edge_fused(*args, latency_depth=depth, onboard=onboard, want_last_plan=depth == 1, spheres=spheres)
    assert calls == ["onboard_reset"] + ["latency_reset"] * (depth > 0) + ["mppi_closed_loop_edge_f64"]
    assert sorted(out) == sorted(RESULT_KEYS + ["plan_last"]) and "controller_state" not in out
    assert out["logs"] == [] and out["latency"]["depth"] == depth and (out["latency"]["ring"] is None) == (depth == 0)
    assert tuple(out["onboard_state"].shape) == (2, 14) and not out["zero_thrust_steps"].any() and out["trace"].shape == (2, 3, 2)
    assert (out["plan_last"] is None) == (depth != 1) and (depth != 1 or tuple(out["plan_last"].shape) == (2, 3, 6, 3))
    assert (out["clearance"] is None) == (spheres is None) and (spheres is None or bool(torch.isinf(out["clearance"]).all()))


@pytest.mark.parametrize("depth", [0, 3])
@pytest.mark.parametrize("log", [False, True])
def test_run_mppi_edge_makes_one_planner_and_one_edge_loop_call_per_cycle(emu_ops, monkeypatch, depth, log):
    mc, args = edge_mc(emu_ops)
    onboard = emu_ops.lib.onboard_default_params()
    calls = recorded(emu_ops, monkeypatch)
    out = mc.run_mppi_edge(*args, latency_depth=depth, onboard=onboard, log=log)
    assert calls == ["controller_reset", "onboard_reset"] + ["latency_reset"] * (depth > 0) + ["mppi_closed_loop_f64", "edge_loop_f64"] * 3
    assert sorted(out) == sorted(RESULT_KEYS) and out["clearance"] is None and out["trace"].shape == (2, 3, 2)
    assert len(out["logs"]) == (3 if log else 0)
    if log:
        plan, flown = out["logs"][0]
        assert tuple(plan["plan_last"].shape) == (2, 3, 6, 3) and tuple(flown["log_state"].shape) == (2, 2, 12)


def test_mppi_closed_loop_edge_checks_its_operands_before_any_call(emu_ops, monkeypatch):
    import torch
    mc, (p0, v0, goal, cycles, substeps, sim_dt, S, iters, sigma, lam) = edge_mc(emu_ops)
    ops = emu_ops
    op, st, buf = ops.lib.onboard_default_params(), ops.onboard_state(2), ops.latency_buffer(2, 3, "f64")
    time, z = torch.zeros(2, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    U = torch.zeros(2, 6, 3, dtype=torch.float64)
    calls = recorded(ops, monkeypatch)
    good = dict(onboard_state=st, buf=buf, time=time, pos=p0, vel=v0, att=z, omega=z.clone(), goal=goal, U=U)
    bad = [dict(onboard_state=torch.zeros(2, 12, dtype=torch.float64)), dict(buf=dict(buf, ring=torch.zeros(3, 12, 3, dtype=torch.float64))),
           dict(buf=dict(buf, depth=1001)), dict(time=torch.zeros(2, dtype=torch.float32)), dict(U=torch.zeros(2, 5, 3, dtype=torch.float64)),
           dict(U=torch.zeros(2, 6, 3, dtype=torch.float32)), dict(vel=torch.zeros(3, 3, dtype=torch.float64)),
           dict(goal=torch.zeros(2, 3, dtype=torch.float32)), dict(wind=torch.zeros(2, dtype=torch.float64)),
           dict(zero_thrust_steps=torch.zeros(2, dtype=torch.int64)), dict(clearance=torch.zeros(3, dtype=torch.float64)),
           dict(spheres=torch.zeros(2, 3, dtype=torch.float64))]
    for change in bad:
        kw = dict(good, **change)
        more = {k: kw.pop(k) for k in ("wind", "zero_thrust_steps", "clearance", "spheres") if k in kw}
        with pytest.raises(ValueError):
            ops.mppi_closed_loop_edge(mc.params, op, mc.simulator, kw["onboard_state"], kw["buf"], kw["time"], kw["pos"], kw["vel"], kw["att"], kw["omega"],
                                      kw["goal"], kw["U"], cycles, substeps, sim_dt, S, iters, sigma, lam, **more)
    assert calls == []
    ops.mppi_closed_loop_edge(mc.params, op, mc.simulator, st, buf, time, p0, v0, z, z.clone(), goal, U, cycles, substeps, sim_dt, S, iters, sigma, lam)
    assert calls == ["mppi_closed_loop_edge_f64"]


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_equals_chain_with_a_different_constant_in_every_block(emu_ops, dt):
    """Every parameter block its own mass, gravity and max_thrust (tests/param_sets.LOOP_BLOCKS): at the defaults planner and simulator
    agree (1.5 kg, 9.81 m/s^2), and a fused kernel that read one block's constant from another would still equal its chain."""
    import param_sets as ps
    L = ps.LOOP_SHAPE
    ec.check_equals_chain(harness(emu_ops, dt), (L["N"], L["B"], L["K"], 64), 2, L["substeps"], last_plan=True, cycles=L["cycles"],
                          blocks=ps.loop_blocks(L["N"], dt=ec.PLAN_DT))
