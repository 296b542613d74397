#!/usr/bin/env python3
"""Golden vectors for the mission layer's goal source, produced by RUNNING THE REFERENCE'S OWN CLASS in the build container:
GlobalMissionPlanner (/root/reference/src/dart_planner/planning/global_mission_planner.py), imported unchanged.  Only inputs and what the class
returned go into the files.

Stand-ins, written to a temp directory and deleted: ``pint`` -- units tagging only; the class reads ``.magnitude`` of its quantities, so
``Q_(x, unit)`` returns an ndarray subclass that has one (the identity stand-in of make_golden.py has none).  ``time.time`` of the module is a
scripted clock (the value the mission's call sequence sets), ``np.random.random`` is pinned to 1.0 while the class runs so that no simulated
high-uncertainty region ever appears (mission.py:434): the np.random parts are not part of the product.

Every mission is a sequence of ``get_current_goal`` calls on a kinematic follower that never lands exactly on its goal:
``pos += min(gain, step / |d|) * d`` with d = goal - pos.  No solver runs here.  Missions: W = 0 .. 4 waypoints of every label; safety_margin
1.5, 2.5 and 2.0 (the 2.0 missions are cut at 28 calls, before the follower converges onto the reach threshold); start altitudes 0 .. 6 m (below
0.5 m the first call declares an emergency); records preset to EXPLORATION and MAPPING; clock steps 0.11 .. 0.45 s from 1000 s.  Four missions run
with use_neural_scene on a 20 x 20 x 20 field at 1 m, whose two grids are recorded at the end.

The generator runs tests/mission_oracle.py beside the class, asserts that the two agree (discrete outputs exactly, goals to 1e-12) and that every
decision that can change the outcome -- the takeoff altitude, the reach distance, the emergency altitude of a global plan outside LANDING and
EMERGENCY, the replan gate -- stays MARGIN = 1e-6 from its threshold, and that every stamp keeps every voxel-centre distance 1e-9 from its radius.
It discards nothing.  Writes mission_cases.npz / .json."""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.environ.get("SE3MPC_GOLDEN_OUT", HERE)
REF_SRC = "/root/reference/src"
sys.path.insert(0, os.path.dirname(HERE))
import mission_oracle as mo  # noqa: E402
import uncertainty_oracle as uo  # noqa: E402

MARGIN, STAMP_MARGIN = 1e-6, 1e-9
FIELD_BOUNDS, FIELD_RES = [[-10.0, -10.0, 0.0], [10.0, 10.0, 20.0]], 1.0

PINT_INIT = '''
import numpy as np
class Quantity(np.ndarray):
    def __new__(cls, value, unit=None): return np.asarray(value, dtype=float).view(cls)
    @property
    def magnitude(self): return np.asarray(self)
    def to(self, unit): return self
class UnitRegistry:
    def __init__(self, *a, **k): pass
    def setup_matplotlib(self, *a, **k): pass
    def __contains__(self, item): return True
    def define(self, s): pass
    def Quantity(self, value, unit=None): return Quantity(value)
'''
PINT_ERRORS = "class DimensionalityError(Exception): pass\n"


def _install_standins():
    d = tempfile.mkdtemp(prefix="se3mpc_golden_")
    os.makedirs(os.path.join(d, "pint"))
    with open(os.path.join(d, "pint", "__init__.py"), "w") as f:
        f.write(PINT_INIT)
    with open(os.path.join(d, "pint", "errors.py"), "w") as f:
        f.write(PINT_ERRORS)
    sys.path.insert(0, d)
    sys.path.insert(1, REF_SRC)
    sys.dont_write_bytecode = True
    os.environ.setdefault("DART_ENV", "test")
    os.environ.setdefault("DART_SECRET_KEY", "golden")
    os.environ.setdefault("DART_ZMQ_SECRET", "golden")
    return d


def main():
    tmp = _install_standins()
    try:
        import logging
        logging.disable(logging.CRITICAL)
        import dart_planner.planning.global_mission_planner as ref
        from dart_planner.common.types import DroneState
        from dart_planner.common.units import Q_
        from dart_planner.neural_scene.uncertainty_field import UncertaintyField

        class Clock:
            now = 0.0

            @classmethod
            def time(cls):
                return cls.now
        ref.time = Clock
        real_random = np.random.random
        np.random.random = lambda size=None: 1.0 if size is None else np.ones(size)

        rng = np.random.default_rng(20261020)
        out, meta = {}, {"margin": MARGIN, "stamp_margin": STAMP_MARGIN, "field_bounds": FIELD_BOUNDS, "field_resolution": FIELD_RES, "missions": []}
        worst = {"decision": np.inf, "stamp": np.inf}
        LABEL_NAMES = ["safe_zone", "obstacle", "landing_pad", "doorway"]

        def run(tag, W, label_names, safety_margin, z0, calls, preset=None, neural=False, spread=8.0, step=1.2):
            key = f"m{len(meta['missions']):02d}_"
            wp = np.zeros((W, 3))
            at = np.array([rng.uniform(-4, 4), rng.uniform(-4, 4), 5.0])
            for w in range(W):                                                     # a chain of waypoints, each at least 3 m from the one before
                hop = rng.uniform(-1, 1, 3) * [spread, spread, 1.5]
                hop[:2] *= max(1.0, 3.0 / np.linalg.norm(hop[:2]))
                at = np.clip(at + hop, [-8.5, -8.5, 2.5], [8.5, 8.5, 9.0]) if neural else at + hop
                at[2] = max(at[2], 2.5)
                wp[w] = at
            cfg = ref.GlobalMissionConfig(safety_margin=Q_(safety_margin, "m"), use_neural_scene=bool(neural))
            planner = ref.GlobalMissionPlanner(cfg)
            if neural:
                planner.uncertainty_field = UncertaintyField(np.array(FIELD_BOUNDS), FIELD_RES)
                orc_field = uo.Field(FIELD_BOUNDS, FIELD_RES)
            planner.set_mission_waypoints([ref.SemanticWaypoint(position=Q_(wp[w].copy(), "m"), semantic_label=label_names[w], uncertainty=0.1, priority=1)
                                           for w in range(W)])
            prm = mo.params(safety_margin=safety_margin, use_neural_scene=int(neural))
            rec = mo.fresh()
            if preset is not None:
                planner.current_phase = ref.MissionPhase(preset)
                rec[0] = float(mo.PHASES.index(preset))
            labels = np.array([mo.label_code(n) for n in label_names], np.int32).reshape(W)
            pos = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), z0]) if neural else np.array([rng.uniform(-6, 6), rng.uniform(-6, 6), z0])
            gain, dt = float(rng.uniform(0.35, 0.6)), float(rng.uniform(0.11, 0.45))
            now = 1000.0
            T = calls
            log = dict(now=np.zeros(T), pos=np.zeros((T, 3)), goal=np.zeros((T, 3)), phase=np.zeros(T, np.int32), index=np.zeros(T, np.int32),
                       last=np.zeros(T), stamp=np.zeros(T, np.int32), plans=np.zeros(T, np.int32))
            phases_seen = set()
            for t in range(T):
                Clock.now = now
                state = DroneState(timestamp=now, position=Q_(pos.copy(), "m"))
                updates_before = planner.neural_scene_model.total_updates if neural else 0
                g = np.asarray(planner.get_current_goal(state), float).copy()
                stamped = neural and planner.neural_scene_model.total_updates == updates_before + 1
                margins = []
                g_orc, s_orc = mo.step(prm, rec, now, pos, wp, labels, margins)
                assert s_orc == stamped, (tag, t)
                assert mo.PHASES[int(rec[0])] == planner.current_phase.value and int(rec[1]) == planner.current_waypoint_index, (tag, t, rec)
                assert rec[2] == planner.last_global_plan_time and int(rec[3]) == len(planner.planning_history), (tag, t, rec)
                assert np.max(np.abs(g_orc - g)) <= 1e-12 * max(1.0, np.max(np.abs(g))), (tag, t, g_orc, g)
                assert min(margins) >= MARGIN, (tag, t, margins)
                worst["decision"] = min(worst["decision"], min(margins))
                if stamped:
                    _, d = uo.stamp_distances(orc_field, pos, prm["stamp_radius"])
                    gap = float(np.min(np.abs(d - prm["stamp_radius"]))) if d.size else np.inf
                    assert gap >= STAMP_MARGIN, (tag, t, gap)
                    worst["stamp"] = min(worst["stamp"], gap)
                    uo.stamp(orc_field, pos, prm["stamp_radius"], prm["stamp_factor"])
                log["now"][t], log["pos"][t], log["goal"][t] = now, pos, g
                log["phase"][t], log["index"][t], log["last"][t] = int(rec[0]), int(rec[1]), rec[2]
                log["stamp"][t], log["plans"][t] = int(stamped), int(rec[3])
                phases_seen.add(int(rec[0]))
                d = g - pos
                n = float(np.linalg.norm(d))
                pos = pos + min(gain, step / n) * d if n > 0 else pos
                now = now + dt
            for k, v in log.items():
                out[key + k] = v
            out[key + "wp"], out[key + "labels"] = wp, labels
            if neural:
                assert np.array_equal(orc_field.u, planner.uncertainty_field.uncertainty_grid) and np.array_equal(orc_field.c, planner.uncertainty_field.observation_count), tag
                out[key + "u"], out[key + "c"] = planner.uncertainty_field.uncertainty_grid, planner.uncertainty_field.observation_count
            meta["missions"].append(dict(key=key, tag=tag, W=W, labels=list(label_names), safety_margin=safety_margin, z0=z0, calls=T, preset=preset,
                                         use_neural_scene=bool(neural), gain=gain, clock_step=dt, end_phase=mo.PHASES[int(rec[0])], end_index=int(rec[1]),
                                         phases=sorted(phases_seen), stamps=int(log["stamp"].sum())))

        z_grid = [0.0, 0.2, 0.45, 0.8, 1.5, 2.5, 3.5, 4.2, 4.8, 5.5, 6.0]
        n = 0
        for W in range(5):
            for margin in (1.5, 2.5, 2.0):
                names = [LABEL_NAMES[(n + w) % 4] for w in range(W)]
                calls = 28 if margin == 2.0 else int(rng.integers(40, 61))
                run(f"W{W}_margin{margin}", W, names, margin, z_grid[(3 + 2 * n) % len(z_grid)], calls, step=0.5 if margin == 2.0 else 1.2)
                n += 1
        for W, names in ((1, ["obstacle"]), (2, ["obstacle", "safe_zone"]), (3, ["doorway", "obstacle", "landing_pad"]), (1, ["landing_pad"]),
                         (2, ["safe_zone", "doorway"]), (4, ["safe_zone", "doorway", "safe_zone", "doorway"])):
            run("labels_" + "_".join(names), W, names, 1.5, 4.8, int(rng.integers(40, 61)), spread=5.0)
        run("obstacles_only", 4, ["obstacle"] * 4, 1.5, 3.5, 60, spread=4.0)
        for z0 in (0.0, 0.2, 0.3, 0.45):
            run(f"starts_low_{z0}", 2, ["safe_zone", "obstacle"], 1.5, z0, 30)
        for preset, W, names in (("exploration", 0, []), ("exploration", 2, ["safe_zone", "obstacle"]), ("mapping", 2, ["safe_zone", "doorway"]),
                                 ("mapping", 0, []), ("mapping", 3, ["obstacle", "landing_pad", "safe_zone"])):
            run(f"preset_{preset}_W{W}", W, names, 2.5, 5.5, int(rng.integers(32, 50)), preset=preset, spread=5.0)
        run("short_hops_to_landing", 3, ["safe_zone", "doorway", "safe_zone"], 1.5, 4.8, 60, spread=3.0)
        run("landing_from_mapping", 1, ["doorway"], 1.5, 6.0, 50, preset="mapping", spread=3.0)
        for tag, W, names, z0 in (("neural_takeoff", 3, ["safe_zone", "obstacle", "doorway"], 1.5), ("neural_low", 1, ["safe_zone"], 0.2),
                                  ("neural_pad", 2, ["doorway", "landing_pad"], 4.8), ("neural_hover", 0, [], 3.5)):
            run(tag, W, names, 1.5, z0, 40, neural=True, spread=4.0)

        np.random.random = real_random
        missions = meta["missions"]
        meta["worst"] = {k: (v if np.isfinite(v) else None) for k, v in worst.items()}
        assert len(missions) >= 36 and all(28 <= m["calls"] <= 60 for m in missions), len(missions)
        assert worst["decision"] >= MARGIN and worst["stamp"] >= STAMP_MARGIN, worst
        assert {p for m in missions for p in m["phases"]} == set(range(6)), "not every phase occurred"
        assert {m["end_phase"] for m in missions} >= {"navigation", "mapping", "exploration", "landing", "emergency"}, {m["end_phase"] for m in missions}
        assert {(m["W"], m["end_index"]) for m in missions} >= {(W, i) for W in range(5) for i in range(W + 1) if W in (0, 1, 2, 3)}, sorted(
            {(m["W"], m["end_index"]) for m in missions})
        assert {i for m in missions if m["W"] == 4 for i in [m["end_index"]]} and {n for m in missions for n in m["labels"]} == set(LABEL_NAMES)
        assert sum(m["use_neural_scene"] for m in missions) == 4 and all(m["stamps"] >= 3 for m in missions if m["use_neural_scene"])
        np.savez_compressed(os.path.join(OUT_DIR, "mission_cases.npz"), **out)
        with open(os.path.join(OUT_DIR, "mission_cases.json"), "w") as f:
            json.dump(meta, f, indent=1)
        print("wrote mission_cases.npz / .json:", len(missions), "missions,", sum(m["calls"] for m in missions), "calls; ends",
              sorted({(m["end_phase"], m["W"], m["end_index"]) for m in missions}), "worst", worst)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
