"""The checks of the mission layer's goal source (dart_planner_amd/csrc/mission.hip, monte_carlo_mission.hip), shared by the CPU
suite (tests/test_emu_mission.py: the kernels compiled for the host) and the GPU suite (tests/test_gpu_mission.py).  `h` is a
parity_checks.Harness (ops, to_dev, to_host, dt = the IO type).

Discrete outputs -- phase, waypoint index, plan count, stamp flags, radius_voxels -- are compared exactly everywhere.  Against the golden file
(the reference's own class) float64 goals and last_global_plan_time to REL = 1e-12: the only inexact steps are np.linalg.norm and one division.
Against tests/mission_oracle.py on the same inputs: float64 goals to REL, float32 goals equal to the oracle's float64 goal rounded to float32,
because every decision and all arithmetic are made in double.  Chains against chains and the one launch against the chain: bit for bit."""
import json
import os

import numpy as np

from dart_planner_amd import capi
from dart_planner_amd.capi import MissionParams, Params
from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo

import mission_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-12
_cache = {}


def golden():
    if "golden" not in _cache:
        with open(os.path.join(GOLDEN, "mission_cases.json")) as f:
            meta = json.load(f)
        _cache["golden"] = (meta, dict(np.load(os.path.join(GOLDEN, "mission_cases.npz"))))
    return _cache["golden"]


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    err = np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1.0), initial=0.0)
    assert err <= REL, (what, err)
    return err


def suffix(h):
    return "f64" if h.dt == np.float64 else "f32"


def mission_params(m):
    return MissionParams.reference_defaults(safety_margin=m["safety_margin"], use_neural_scene=m["use_neural_scene"])


def device_field(h, meta):
    """a fresh 20 x 20 x 20 field of the golden file's neural missions -> (u, c, descriptor)"""
    n = tuple(int(round((hi - lo) / meta["field_resolution"])) for lo, hi in zip(*meta["field_bounds"]))
    u, c = h.to_dev(np.zeros(n)), h.to_dev(np.zeros(n))
    desc = h.ops.ufield_desc(u, c, meta["field_bounds"][0], meta["field_resolution"])
    h.ops.ufield_fill(desc)
    return u, c, desc


# ------------------------------------------------------------------------------------------------ golden sequences
def fly_mission(h, m, g, pos, field=None):
    """the recorded call sequence of mission m through the C ABI, B = 1 -> per call goal, record, stamp row (host arrays)"""
    ops, key = h.ops, m["key"]
    st = ops.mission_state(1)
    if m["preset"] is not None:
        st[0, 0] = float(mo.PHASES.index(m["preset"]))
    wp, lab = h.to_dev(g[key + "wp"]), h.to_dev(g[key + "labels"])
    mp = mission_params(m)
    goals, recs, rvs, radii = [], [], [], []
    for t in range(m["calls"]):
        out = ops.mission_goal(mp, st, h.to_dev(g[key + "now"][t:t + 1]), h.to_dev(np.ascontiguousarray(pos[t:t + 1])), wp, lab, resolution=1.0)
        if field is not None:
            s = out["stamps"]
            ops.ufield_stamp(field, s["centres"], s["radius"], s["radius_voxels"], s["factor"])
        goals.append(out["goal"])
        recs.append(st.clone())
        rvs.append(out["stamps"]["radius_voxels"])
        radii.append(out["stamps"]["radius"])
    host = lambda xs: np.concatenate([np.array(h.to_host(x)) for x in xs])
    return host(goals), host(recs), host(rvs), host(radii)


def check_golden_sequences(h):
    """float64: the reference's own sequences.  float32: the same call sequences on float32-rounded positions, against the oracle."""
    meta, g = golden()
    worst = 0.0
    for m in meta["missions"]:
        key = m["key"]
        pos = g[key + "pos"].astype(h.dt)
        goal, rec, rv, radius = fly_mission(h, m, g, pos)
        if h.dt == np.float64:
            want = dict(goal=g[key + "goal"], phase=g[key + "phase"], index=g[key + "index"], last=g[key + "last"], plans=g[key + "plans"], stamp=g[key + "stamp"])
        else:
            prm = mo.params(safety_margin=m["safety_margin"], use_neural_scene=int(m["use_neural_scene"]))
            r = mo.fresh()
            if m["preset"] is not None:
                r[0] = float(mo.PHASES.index(m["preset"]))
            want = dict(goal=[], phase=[], index=[], last=[], plans=[], stamp=[])
            for t in range(m["calls"]):
                go, stamped = mo.step(prm, r, g[key + "now"][t], pos[t].astype(np.float64), g[key + "wp"], g[key + "labels"])
                for k, v in zip(("goal", "phase", "index", "last", "plans", "stamp"), (go, r[0], r[1], r[2], r[3], stamped)):
                    want[k].append(v)
            want = {k: np.array(v) for k, v in want.items()}
        assert np.array_equal(rec[:, 0], want["phase"]) and np.array_equal(rec[:, 1], want["index"]) and np.array_equal(rec[:, 3], want["plans"]), m["tag"]
        stamped = np.asarray(want["stamp"]).astype(bool)
        assert np.array_equal(rv, np.where(stamped, 3, -1)) and np.array_equal(radius, np.where(stamped, 3.0, -1.0)), m["tag"]
        worst = max(worst, close(rec[:, 2], want["last"], m["tag"] + " last_global_plan_time"))
        if h.dt == np.float64:
            worst = max(worst, close(goal, want["goal"], m["tag"] + " goal"))
        else:
            same_bits(goal, want["goal"].astype(np.float32), m["tag"] + " goal")
    print(f"{len(meta['missions'])} missions, {np.dtype(h.dt).name}: worst relative error {worst:.3g}")


def check_mirror_class(h):
    """the golden sequences through dart_planner_amd.planning.global_mission_planner, the neural missions with the mirror's own field"""
    from dart_planner_amd.common.types import DroneState
    from dart_planner_amd.neural_scene import UncertaintyField
    from dart_planner_amd.planning.global_mission_planner import GlobalMissionConfig, GlobalMissionPlanner, MissionPhase, SemanticWaypoint
    meta, g = golden()
    for m in meta["missions"][::3] + [m for m in meta["missions"] if m["use_neural_scene"]]:
        key, clock = m["key"], [0.0]
        field = UncertaintyField(np.array(meta["field_bounds"]), meta["field_resolution"], ops=h.ops) if m["use_neural_scene"] else None
        planner = GlobalMissionPlanner(GlobalMissionConfig(safety_margin=m["safety_margin"], use_neural_scene=m["use_neural_scene"]), ops=h.ops,
                                       clock=lambda: clock[0], uncertainty_field=field)
        assert planner.current_phase is MissionPhase.TAKEOFF and planner.current_waypoint_index == 0 and planner.last_global_plan_time == 0.0
        planner.set_mission_waypoints([SemanticWaypoint(position=g[key + "wp"][w], semantic_label=m["labels"][w], uncertainty=0.1, priority=1)
                                       for w in range(m["W"])])
        if m["preset"] is not None:
            planner.current_phase = MissionPhase(m["preset"])
        for t in range(m["calls"]):
            clock[0] = float(g[key + "now"][t])
            goal = planner.get_current_goal(DroneState(timestamp=clock[0], position=g[key + "pos"][t]))
            close(goal, g[key + "goal"][t], f"{m['tag']} call {t}")
            assert planner.current_phase.value == mo.PHASES[g[key + "phase"][t]] and planner.current_waypoint_index == g[key + "index"][t], (m["tag"], t)
            close(planner.last_global_plan_time, g[key + "last"][t], m["tag"])
        status = planner.get_mission_status()
        assert status["current_phase"] == m["end_phase"] and status["waypoint_progress"] == f"{m['end_index']}/{m['W']}", (m["tag"], status)
        assert status["planning_history_length"] == g[key + "plans"][-1] and status["neural_scene_updates"] == m["stamps"], (m["tag"], status)
        if field is not None:
            same_bits(field.uncertainty_grid, g[key + "u"], m["tag"] + " uncertainty")
            same_bits(field.observation_count, g[key + "c"], m["tag"] + " observation_count")


def check_stamp_table(h):
    """float64: the stamp rows of the neural missions through se3mpc_ufield_stamp give the golden grids bit for bit; -1 rows change nothing"""
    meta, g = golden()
    for m in meta["missions"]:
        if not m["use_neural_scene"]:
            continue
        u, c, desc = device_field(h, meta)
        _, rec, rv, _ = fly_mission(h, m, g, g[m["key"] + "pos"], field=desc)
        assert int((rv >= 0).sum()) == m["stamps"] >= 3
        same_bits(np.array(h.to_host(u)), g[m["key"] + "u"], m["tag"] + " uncertainty")
        same_bits(np.array(h.to_host(c)), g[m["key"] + "c"], m["tag"] + " observation_count")
        before = np.array(h.to_host(u)).copy(), np.array(h.to_host(c)).copy()
        off = m["key"]
        st = h.ops.mission_state(4)
        out = h.ops.mission_goal(MissionParams.reference_defaults(use_neural_scene=False), st, h.to_dev(np.full(4, 1000.0)), h.to_dev(g[off + "pos"][:4].copy()),
                                 h.to_dev(g[off + "wp"]), h.to_dev(g[off + "labels"]), resolution=1.0)
        s = out["stamps"]
        assert np.all(np.array(h.to_host(s["radius_voxels"])) == -1) and np.all(np.array(h.to_host(s["radius"])) == -1.0)
        assert np.all(np.array(h.to_host(st))[:, 3] == 1.0)                                          # every drone made its global plan
        h.ops.ufield_stamp(desc, s["centres"], s["radius"], s["radius_voxels"], s["factor"])
        same_bits(np.array(h.to_host(u)), before[0], "a table of -1 rows: uncertainty")
        same_bits(np.array(h.to_host(c)), before[1], "a table of -1 rows: observation_count")


# ------------------------------------------------------------------------------------------------ random batches against the oracle
def random_batch(B, W, per_drone, seed):
    rng = np.random.default_rng(seed)
    wp = rng.uniform(-8, 8, (B, W, 3) if per_drone else (W, 3)) + [0, 0, 9]
    labels = rng.integers(0, 5, (B, W) if per_drone else (W,)).astype(np.int32)        # 4: a code the header does not name = any other label
    pos = rng.uniform(-8, 8, (B, 3)) + [0, 0, 7]
    pos[rng.random(B) < 0.2, 2] = rng.uniform(0.0, 0.45)                               # below the emergency altitude
    rec = np.zeros((B, 4))
    rec[:, 0] = rng.integers(0, 6, B)                                                  # the drones of one wavefront in different phases
    rec[:, 1] = rng.integers(0, W + 1, B)
    rec[:, 2] = rng.choice((0.0, 999.5, 999.95), B)
    rec[:, 3] = rng.integers(0, 9, B)
    if W:                                                                              # some drones within reach of their current waypoint
        near = np.flatnonzero((rng.random(B) < 0.4) & (rec[:, 1] < W))
        for b in near:
            w = (wp[b] if per_drone else wp)[int(rec[b, 1])]
            pos[b] = w + rng.uniform(-1, 1, 3)
        on = near[:1]                                                                  # ... and one exactly on an obstacle waypoint: norm 0
        for b in on:
            pos[b] = (wp[b] if per_drone else wp)[int(rec[b, 1])]
    if B > 2:
        pos[1] = np.nan                                                                # a NaN drone
        rec[2, 1] = W + 7                                                              # a preset index past the table
    if B > 5:
        rec[4, 1] = -3.0
        rec[5, 0] = 9.0                                                                # a phase word outside the enum
    now = np.full(B, 1000.0) + rng.uniform(0, 0.8, B)
    return wp, labels, pos, rec, now


def check_random_batch(h, B, W, per_drone):
    for neural in (1, 0):
        wp, labels, pos, rec, now = random_batch(B, W, per_drone, 1000 * B + 10 * W + per_drone)
        pos = pos.astype(h.dt)
        prm = mo.params(safety_margin=1.5, use_neural_scene=neural, exploration_radius=7.0)
        mp = MissionParams.reference_defaults(safety_margin=1.5, use_neural_scene=neural, exploration_radius=7.0)
        want_rec = rec.copy()
        want = mo.batch(prm, want_rec, now, pos.astype(np.float64), wp, labels, resolution=0.7)
        st = h.to_dev(rec.copy())
        dirty = lambda shape, dt: h.to_dev(np.frombuffer(b"\x7b" * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy())
        stamps = dict(centres=dirty((B, 3), np.float64), radius=dirty((B,), np.float64), radius_voxels=dirty((B,), np.int32), factor=dirty((B,), np.float64))
        out = h.ops.mission_goal(mp, st, h.to_dev(now), h.to_dev(pos), h.to_dev(wp), h.to_dev(labels), resolution=0.7, goal=dirty((B, 3), h.dt), stamps=stamps)
        got_rec = np.array(h.to_host(st))
        what = f"B={B} W={W} per_drone={per_drone} neural={neural}"
        same_bits(got_rec, want_rec, what + " records")
        goal = np.array(h.to_host(out["goal"]))
        if h.dt == np.float64:
            close(goal, want["goal"], what + " goal")
        else:
            same_bits(goal, want["goal"].astype(np.float32), what + " goal")
        s = {k: np.array(h.to_host(v)) for k, v in out["stamps"].items()}
        same_bits(s["centres"], want["centres"], what + " centres")
        for k in ("radius", "radius_voxels", "factor"):
            same_bits(s[k], want[k], f"{what} {k}")
        assert neural == 0 or (0 < int((s["radius_voxels"] == 4).sum()) < B or B == 1), what      # int(3.0 / 0.7) = 4; some replanned, some did not
        assert len(set(got_rec[:, 0])) >= min(B, 4) or B == 1, what


# ------------------------------------------------------------------------------------------------ missions in the closed loop
CYCLES, SUBSTEPS, SIM_DT = 6, 5, 0.0025
# a replan period of two cycles (the reference's 1 s would let only the first call plan): stamps in cycles 0, 2 and 4
LOOP_MISSION = dict(global_replan_period=0.02)


def scene(B, W=3, seed=5):
    """drones around 4 m up (most below, some above the takeoff altitude; a few below the emergency altitude) and, per drone, waypoint 0 1.2 to
    2.6 m away (inside and outside the reach distance), the others further out"""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(-3, 3, (B, 3)) + [0, 0, 4.3]
    p0[rng.random(B) < 0.15, 2] = rng.uniform(0.1, 0.4)
    v0 = rng.normal(0, 0.2, (B, 3))
    wp = np.zeros((B, W, 3))
    d = rng.normal(0, 1, (B, 3))
    wp[:, 0] = p0 + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.2, 2.6, (B, 1))
    for w in range(1, W):
        wp[:, w] = wp[:, w - 1] + rng.uniform(-3, 3, (B, 3))
    labels = rng.integers(0, 4, (B, W)).astype(np.int32)
    wind = rng.normal(0, 1, (B, 3))
    return p0, v0, wp, labels, wind


RESULT_KEYS = ("pos", "vel", "att", "omega", "time", "controller_state", "mission_state", "goal", "phase", "waypoint_index")


def _host(h, out):
    return {k: np.array(h.to_host(out[k])) for k in RESULT_KEYS}


def _mc(h, N):
    return ClosedLoopMonteCarlo(h.ops, Params.reference_defaults(horizon=N))


_chain = {}


def chain(h, N, B, cycles=CYCLES):
    """ClosedLoopMonteCarlo.run_mission on a fresh field, as host arrays (computed once, never written)"""
    key = (id(h.ops), np.dtype(h.dt).name, N, B, cycles)
    if key not in _chain:
        meta, _ = golden()
        p0, v0, wp, labels, wind = scene(B)
        u, c, desc = device_field(h, meta)
        out = _mc(h, N).run_mission(h.prob(p0), h.prob(v0), h.to_dev(wp), h.to_dev(labels), cycles, SUBSTEPS, SIM_DT, mission=MissionParams.reference_defaults(**LOOP_MISSION),
                                    field=desc, wind=h.prob(wind), log=True)
        res = _host(h, out)
        res.update(u=np.array(h.to_host(u)), c=np.array(h.to_host(c)), goals=np.array(h.to_host(out["goals"])), phases=np.array(h.to_host(out["phases"])))
        for v in res.values():
            v.setflags(write=False)
        _chain[key] = res
    return _chain[key]


def check_run_mission_equals_hand_chain(h, N=6, B=65):
    """run_mission == mission_goal + ufield_stamp + solve + closed_loop calls made here, bit for bit; and the run is not vacuous"""
    import torch
    ops = h.ops
    ref = chain(h, N, B)
    meta, _ = golden()
    p0, v0, wp, labels, wind = scene(B)
    mc, mp = _mc(h, N), MissionParams.reference_defaults(**LOOP_MISSION)
    u, c, desc = device_field(h, meta)
    pos, vel, wpd, lab, wnd = h.prob(p0), h.prob(v0), h.to_dev(wp), h.to_dev(labels), h.prob(wind)
    att, om, time = torch.zeros_like(pos), torch.zeros_like(pos), h.to_dev(np.zeros(B))
    st, ms = ops.controller_state(mc.controller, B), ops.mission_state(B)
    k = h.to_dev(np.arange(N, dtype=np.float64))
    goals, phases = [], []
    for cyc in range(CYCLES):
        mg = ops.mission_goal(mp, ms, time + 1000.0, pos, wpd, lab, resolution=meta["field_resolution"])
        s = mg["stamps"]
        ops.ufield_stamp(desc, s["centres"], s["radius"], s["radius_voxels"], s["factor"])
        goals.append(np.array(h.to_host(mg["goal"])).copy())
        phases.append(np.array(h.to_host(ms))[:, 0].astype(np.int32))
        sol = ops.solve(mc.params, pos, vel, mg["goal"], want_trajectory="accelerations")
        X = sol["x"]
        ops.closed_loop(mc.controller, mc.simulator, st, time, pos, vel, att, om, (cyc * SUBSTEPS * SIM_DT) + k * mc.params.dt, X, X[:, 3 * N:], sol["accelerations"],
                        nsteps=SUBSTEPS, sim_dt=SIM_DT, strides=(9 * N, 9 * N, 3 * N), wind=wnd, stop_at_plan_end=False)
    rec = np.array(h.to_host(ms))
    got = dict(pos=pos, vel=vel, att=att, omega=om, time=time, controller_state=st, mission_state=ms, goal=mg["goal"])
    for key, v in got.items():
        same_bits(np.array(h.to_host(v)), ref[key], key)
    same_bits(rec[:, 0].astype(np.int32), ref["phase"], "phase")
    same_bits(rec[:, 1].astype(np.int32), ref["waypoint_index"], "waypoint_index")
    same_bits(np.array(goals), ref["goals"], "logged goals")
    same_bits(np.array(phases), ref["phases"], "logged phases")
    same_bits(np.array(h.to_host(u)), ref["u"], "uncertainty")
    same_bits(np.array(h.to_host(c)), ref["c"], "observation_count")
    # conditions on the chain under which the byte comparisons say something
    assert all(np.isfinite(ref[key]).all() for key in ref)
    assert (rec[:, 3] == 3.0).all() and (ref["c"] > 0).any() and (ref["u"] < 1.0).any(), "three global plans per drone, stamps on the field"
    assert {mo.TAKEOFF, mo.NAVIGATION, mo.EMERGENCY} <= set(ref["phase"].tolist()) and {0, 1} <= set(ref["waypoint_index"].tolist()), (
        sorted(set(ref["phase"].tolist())), sorted(set(ref["waypoint_index"].tolist())))
    assert (ref["goals"][0] != ref["goals"][-1]).any(axis=1).sum() >= B // 4, "the goal moves during the run"


def check_fused_equals_chain(h, N, B):
    """run_mission_fused == run_mission on every returned tensor and on the field's two grids, bit for bit"""
    ref = chain(h, N, B)
    meta, _ = golden()
    p0, v0, wp, labels, wind = scene(B)
    u, c, desc = device_field(h, meta)
    out = _mc(h, N).run_mission_fused(h.prob(p0), h.prob(v0), h.to_dev(wp), h.to_dev(labels), CYCLES, SUBSTEPS, SIM_DT,
                                      mission=MissionParams.reference_defaults(**LOOP_MISSION), field=desc, wind=h.prob(wind))
    assert out["logs"] == [] and out["last_plan"] is None
    got = _host(h, out)
    for key in RESULT_KEYS:
        same_bits(got[key], ref[key], f"N={N} B={B}: {key}")
    same_bits(np.array(h.to_host(u)), ref["u"], "uncertainty")
    same_bits(np.array(h.to_host(c)), ref["c"], "observation_count")
    assert np.isfinite(ref["pos"]).all() and (ref["c"] > 0).any()


def check_fused_continues(h, N=6, B=65):
    """two launches of CYCLES / 2 cycles (the second with first_cycle = CYCLES / 2 on the first's operands) == one of CYCLES == the chain; the
    stamp logs of the two launches, applied one after the other, give the chain's grids"""
    ref = chain(h, N, B)
    meta, _ = golden()
    p0, v0, wp, labels, wind = scene(B)
    u, c, desc = device_field(h, meta)
    mc, mp = _mc(h, N), MissionParams.reference_defaults(**LOOP_MISSION)
    args = (h.to_dev(wp), h.to_dev(labels), CYCLES // 2, SUBSTEPS, SIM_DT)
    first = mc.run_mission_fused(h.prob(p0), h.prob(v0), *args, mission=mp, field=desc, wind=h.prob(wind))
    half = chain(h, N, B, CYCLES // 2)
    for key in RESULT_KEYS:
        same_bits(np.array(h.to_host(first[key])), half[key], f"after {CYCLES // 2} cycles: {key}")
    out = mc.run_mission_fused(None, None, *args, mission=mp, field=desc, wind=h.prob(wind), first_cycle=CYCLES // 2, resume=first)
    got = _host(h, out)
    for key in RESULT_KEYS:
        same_bits(got[key], ref[key], f"{CYCLES // 2} + {CYCLES // 2} cycles: {key}")
    same_bits(np.array(h.to_host(u)), ref["u"], "uncertainty")
    same_bits(np.array(h.to_host(c)), ref["c"], "observation_count")


# Chosen by running this check under emulation (float64 and float32 alike): with sim_dt 0.01 and 5 steps per cycle every drone of this loop
# climbs under saturated thrust (3.52 m/s^2), whatever its goal.  Observed, counting cycles from 0: the drones started at z = 4.0 leave TAKEOFF in
# cycle 11 (z = 4.53), their goal is waypoint 1 from cycle 19 (z = 5.61 against the 5.49 at which waypoint 0 is within reach; 5.44 the cycle
# before); the drone started at z = 0.2 is in EMERGENCY from its first call and its goal max(0, z - 2) leaves 0 in cycle 22 (z = 1.82 in cycle 20,
# 1.99 in cycle 21).  21 cycles (0 .. 20) show all three with those margins.
BEHAVIOUR_CYCLES = 21


def check_behaviour(h, cycles=BEHAVIOUR_CYCLES, report=False):
    """on the chain form: drones started at z = 4 with waypoint 0 ahead leave TAKEOFF, advance the index and end on another goal than the first;
    a drone started at z = 0.2 ends in EMERGENCY with goal z = 0"""
    B = 3
    p0 = np.array([[0.0, 0.0, 4.0], [1.0, -2.0, 4.0], [0.5, 0.5, 0.2]])
    # The reference's DroneSimulator applies the thrust along z whatever the attitude (simulator.py:59), so without wind a drone only climbs
    # or falls: "ahead" is up.  Waypoint 0 lies 3.45 m from the start and still 2.96 m from the takeoff altitude, inside the reach distance from z = 5.49.
    wp = np.array([[0.5, 0.3, 7.4], [9.0, 4.0, 9.0], [12.0, -3.0, 5.0]])
    wp = np.stack([wp, wp + [1.0, -2.0, 0.0], wp])
    labels = np.array([0, 3, 2], np.int32)
    out = _mc(h, 6).run_mission(h.prob(p0), h.prob(np.zeros((B, 3))), h.to_dev(wp), h.to_dev(labels), cycles, 5, 0.01, log=True)
    phases, goals, idx = np.array(h.to_host(out["phases"])), np.array(h.to_host(out["goals"])), np.array(h.to_host(out["waypoint_index"]))
    if report:
        for b in range(2):
            left = int(np.argmax(phases[:, b] != mo.TAKEOFF)) if (phases[:, b] != mo.TAKEOFF).any() else -1
            on1 = (goals[:, b] == wp[b, 1].astype(h.dt)).all(axis=1)
            print(f"{np.dtype(h.dt).name} drone {b}: leaves TAKEOFF in cycle {left}, goal = waypoint 1 from cycle {int(np.argmax(on1)) if on1.any() else -1}")
    assert np.isfinite(np.array(h.to_host(out["pos"]))).all()
    for b in range(2):
        assert phases[0, b] == mo.TAKEOFF and phases[-1, b] == mo.NAVIGATION, (b, phases[:, b])
        assert idx[b] >= 1 and (goals[-1, b] != goals[0, b]).any(), (b, idx[b], goals[0, b], goals[-1, b])
        assert goals[0, b, 2] == 5.0 and (goals[0, b, :2] == p0[b, :2].astype(h.dt)).all()
    assert (phases[:, 2] == mo.EMERGENCY).all() and int(np.array(h.to_host(out["phase"]))[2]) == mo.EMERGENCY and (goals[:, 2, 2] == 0.0).all()


def check_unbuilt_forms(h):
    import pytest
    mc = _mc(h, 6)
    z = h.prob(np.zeros((2, 3)))
    wp, lab = h.to_dev(np.zeros((1, 3))), h.to_dev(np.zeros(1, np.int32))
    for kw in (dict(smoother=capi.SmootherParams.reference_defaults()), dict(mixer=capi.MixerParams.reference_defaults()), dict(latency_depth=5),
               dict(swarm_size=2), dict(sphere_velocities=z)):
        with pytest.raises(ValueError, match="DESIGN.md 5.10"):
            mc.run_mission(z, z, wp, lab, 1, 1, 0.01, **kw)
        with pytest.raises(ValueError, match="DESIGN.md 5.10"):
            mc.run_mission_fused(z, z, wp, lab, 1, 1, 0.01, **kw)
    with pytest.raises(ValueError, match="planner"):
        mc.run_mission(z, z, wp, lab, 1, 1, 0.01, planner="shooting")
    with pytest.raises(TypeError):
        mc.run_mission(z, z, wp, lab, 1, 1, 0.01, gaol=z)


def check_mppi_missions(h, B=5):
    """planner="mppi": the chain of mission_goal + one-cycle se3mpc_mppi_closed_loop_* calls made here, bit for bit"""
    import torch
    ops = h.ops
    N = 6
    p0, v0, wp, labels, wind = scene(B)
    mc, mp = _mc(h, N), MissionParams.reference_defaults(**LOOP_MISSION)
    spheres = h.prob(np.array([[1.0, 0.5, 4.5, 0.4], [-2.0, 1.0, 4.0, 0.6]]))
    kw = dict(n_samples=64, iters=2, sigma=0.8, temperature=1.0, seed=3, spheres=spheres, obstacle_weight=50.0)
    out = mc.run_mission(h.prob(p0), h.prob(v0), h.to_dev(wp), h.to_dev(labels), 3, SUBSTEPS, SIM_DT, mission=mp, planner="mppi", wind=h.prob(wind), **kw)
    pos, vel, wnd = h.prob(p0), h.prob(v0), h.prob(wind)
    att, om, time = torch.zeros_like(pos), torch.zeros_like(pos), h.to_dev(np.zeros(B))
    st, ms = ops.controller_state(mc.controller, B), ops.mission_state(B)
    U, clr = mc._mppi_start(pos, None), None
    for cyc in range(3):
        mg = ops.mission_goal(mp, ms, time + 1000.0, pos, h.to_dev(wp), h.to_dev(labels))
        step = ops.mppi_closed_loop(mc.params, mc.controller, mc.simulator, st, time, pos, vel, att, om, mg["goal"], U, 1, SUBSTEPS, SIM_DT, kw["n_samples"],
                                    kw["iters"], kw["sigma"], kw["temperature"], seed=3, cycle_base=cyc, shift=mc.resolve_shift(SUBSTEPS, SIM_DT), spheres=spheres,
                                    obstacle_weight=50.0, wind=wnd, clearance=clr)
        clr = step["clearance"]
    for key, v in dict(pos=pos, vel=vel, time=time, controller_state=st, mission_state=ms, goal=mg["goal"], U=U, clearance=clr, cost=step["cost"]).items():
        same_bits(np.array(h.to_host(out[key])), np.array(h.to_host(v)), "mppi mission: " + key)
    assert tuple(out["trace"].shape) == (B, 3, 2) and np.isfinite(np.array(h.to_host(out["clearance"]))).all()


# ------------------------------------------------------------------------------------------------ argument rules
def check_invalid_arguments(h):
    """every rule of include/se3mpc.h returns its code and writes nothing"""
    import torch
    ops, lib, suf = h.ops, h.ops.lib, suffix(h)
    ptr, stream = ops.be.ptr, ops.be.stream()
    NULL, SHAPE, PARAM = -1, -3, -4
    B, W = 3, 2
    good = MissionParams.reference_defaults()
    assert bytes(lib.mission_default_params()) == bytes(good) and lib.check_mission_params(good) == 0 and lib.check_mission_params(None) == NULL
    bad_params = [good.copy(safety_margin=float("nan")), good.copy(stamp_factor=float("inf")), good.copy(global_replan_period=0.0),
                  good.copy(global_replan_period=-1.0)]
    assert all(lib.check_mission_params(p) == PARAM for p in bad_params)
    d = lambda *s: h.to_dev(np.full(s, 7.0))
    z = lambda *s: h.prob(np.full(s, 7.0))
    now, st, wp, cen, rad, fac = d(B), d(B, 4), d(B, W, 3), d(B, 3), d(B), d(B)          # the tables: room for per-drone strides
    lab, rv = h.to_dev(np.full(B * W, 7, np.int32)), h.to_dev(np.full(B, 7, np.int32))
    pos, goal = z(B, 3), z(B, 3)
    default = dict(mp=good, B=B, now=ptr(now), pos=ptr(pos), st=ptr(st), wp=ptr(wp), ws=0, lab=ptr(lab), ls=0, W=W, res=1.0, goal=ptr(goal), cen=ptr(cen),
                   rad=ptr(rad), rv=ptr(rv), fac=ptr(fac))

    def status(**kw):
        a = dict(default, **kw)
        assert not set(kw) - set(default)
        return lib.loop_status("mission_goal", suf, a["mp"], a["B"], a["now"], a["pos"], a["st"], a["wp"], a["ws"], a["lab"], a["ls"], a["W"], a["res"], a["goal"],
                               a["cen"], a["rad"], a["rv"], a["fac"], stream)
    rejected = [(NULL, dict(mp=None))] + [(PARAM, dict(mp=p)) for p in bad_params] + [
        (NULL, dict(now=0)), (NULL, dict(pos=0)), (NULL, dict(st=0)), (NULL, dict(goal=0)), (NULL, dict(cen=0)), (NULL, dict(rad=0)), (NULL, dict(rv=0)),
        (NULL, dict(fac=0)), (NULL, dict(wp=0)), (NULL, dict(lab=0)),
        (SHAPE, dict(B=-1)), (SHAPE, dict(W=-1)), (SHAPE, dict(ws=3 * W - 1)), (SHAPE, dict(ws=-6)), (SHAPE, dict(ls=W - 1)), (SHAPE, dict(ls=-2)),
        (PARAM, dict(res=0.0)), (PARAM, dict(res=float("nan"))), (PARAM, dict(res=float("inf")))]
    for code, kw in rejected:
        assert status(**kw) == code, (code, kw, status(**kw))
    # the one-launch entry point: the same rules, and parameters without a goal
    prm, cp, sp = Params.reference_defaults(), lib.controller_default_params(), lib.simulator_default_params()
    time, cst, over = d(B), d(B, 12), h.to_dev(np.full(1, 7, np.int32))
    vel, att, om = z(B, 3), z(B, 3), z(B, 3)
    fdefault = dict(default, prm=prm, cp=cp, sp=sp, cycles=1, substeps=2, sim_dt=0.01, first=0, epoch=1000.0, wind=0, wstride=0, time=ptr(time), vel=ptr(vel),
                    att=ptr(att), om=ptr(om), cst=ptr(cst), over=ptr(over))

    def fused(**kw):
        a = dict(fdefault, **kw)
        assert not set(kw) - set(fdefault)
        return lib.loop_status("monte_carlo_mission", suf, a["prm"], a["cp"], a["sp"], a["mp"], a["B"], a["cycles"], a["substeps"], a["sim_dt"], a["first"], a["epoch"],
                               a["wp"], a["ws"], a["lab"], a["ls"], a["W"], a["res"], a["wind"], a["wstride"], a["time"], a["pos"], a["vel"], a["att"], a["om"],
                               a["cst"], a["st"], a["goal"], a["cen"], a["rad"], a["rv"], a["fac"], 0, 0, 0, a["over"], stream)
    rejected = [(PARAM, dict(prm=Params.reference_defaults(has_goal=0))), (NULL, dict(prm=None)), (NULL, dict(cp=None)), (NULL, dict(sp=None)), (NULL, dict(mp=None))] + [
        (PARAM, dict(mp=p)) for p in bad_params] + [
        (NULL, dict(time=0)), (NULL, dict(pos=0)), (NULL, dict(vel=0)), (NULL, dict(att=0)), (NULL, dict(om=0)), (NULL, dict(cst=0)), (NULL, dict(st=0)),
        (NULL, dict(goal=0)), (NULL, dict(over=0)), (NULL, dict(wp=0)), (NULL, dict(lab=0)), (NULL, dict(cen=0)), (NULL, dict(rv=0, fac=0)),
        (SHAPE, dict(B=-1)), (SHAPE, dict(W=-1)), (SHAPE, dict(ws=3 * W - 1)), (SHAPE, dict(ls=W - 1)), (SHAPE, dict(cycles=-1)), (SHAPE, dict(substeps=-1)),
        (SHAPE, dict(first=-1)), (SHAPE, dict(first=2 ** 30, cycles=2 ** 30 - 1, substeps=2)), (SHAPE, dict(wind=ptr(vel), wstride=2)),
        (PARAM, dict(res=0.0)), (PARAM, dict(sim_dt=float("nan"))), (PARAM, dict(epoch=float("inf")))]
    for code, kw in rejected:
        assert fused(**kw) == code, (code, kw, fused(**kw))
    if hasattr(torch, "cuda") and torch.cuda.is_available():
        torch.cuda.synchronize()
    assert int(h.to_host(over)[0]) == 7 and all((np.asarray(h.to_host(a)) == 7).all() for a in (now, st, wp, cen, rad, fac, lab, rv, pos, goal, time, cst, vel, att, om)), \
        "a rejected call wrote an operand"
    # accepted: B = 0 with nothing there; W = 0 without tables; per-drone strides; no stamp log
    assert status(B=0, now=0, pos=0, st=0, goal=0, cen=0, rad=0, rv=0, fac=0, wp=0, lab=0) == 0 and fused(B=0, time=0, pos=0, over=0, st=0, goal=0) == 0
    assert int(h.to_host(over)[0]) == 7
    st2, cst2, time2 = ops.mission_state(B), ops.controller_state(cp, B), h.to_dev(np.zeros(B))
    assert status(st=ptr(st2), W=0, wp=0, lab=0) == 0 and status(st=ptr(st2), W=1, ws=3, ls=1) == 0
    assert status(st=ptr(st2), mp=good.copy(use_neural_scene=False), res=0.0) == 0
    assert fused(st=ptr(st2), cst=ptr(cst2), time=ptr(time2), cen=0, rad=0, rv=0, fac=0, cycles=0) == 0
    if hasattr(torch, "cuda") and torch.cuda.is_available():
        torch.cuda.synchronize()
    assert int(h.to_host(over)[0]) == 0
