"""CPU: tests/mission_oracle.py against the sequences the reference's own GlobalMissionPlanner produced (tests/golden/mission_cases.*): discrete
outputs exactly, goals and last_global_plan_time to 1e-12, and the stamps it makes give the recorded grids bit for bit."""
import numpy as np

import mission_checks as mc
import mission_oracle as mo
import uncertainty_oracle as uo


def test_oracle_reproduces_the_reference_sequences():
    meta, g = mc.golden()
    assert len(meta["missions"]) >= 36 and meta["worst"]["decision"] >= meta["margin"] == 1e-6
    for m in meta["missions"]:
        key = m["key"]
        prm = mo.params(safety_margin=m["safety_margin"], use_neural_scene=int(m["use_neural_scene"]))
        rec = mo.fresh()
        if m["preset"] is not None:
            rec[0] = float(mo.PHASES.index(m["preset"]))
        field = uo.Field(meta["field_bounds"], meta["field_resolution"]) if m["use_neural_scene"] else None
        for t in range(m["calls"]):
            goal, stamped = mo.step(prm, rec, g[key + "now"][t], g[key + "pos"][t], g[key + "wp"], g[key + "labels"])
            assert (int(rec[0]), int(rec[1]), int(rec[3]), int(stamped)) == (g[key + "phase"][t], g[key + "index"][t], g[key + "plans"][t], g[key + "stamp"][t]), (m["tag"], t)
            mc.close(goal, g[key + "goal"][t], f"{m['tag']} call {t}")
            mc.close(rec[2], g[key + "last"][t], m["tag"])
            if stamped:
                uo.stamp(field, g[key + "pos"][t], prm["stamp_radius"], prm["stamp_factor"])
        assert mo.PHASES[int(rec[0])] == m["end_phase"] and int(rec[1]) == m["end_index"]
        if field is not None:
            assert np.array_equal(field.u, g[key + "u"]) and np.array_equal(field.c, g[key + "c"]), m["tag"]


def test_golden_file_covers_what_the_checks_rely_on():
    meta, g = mc.golden()
    ms = meta["missions"]
    assert {p for m in ms for p in m["phases"]} == set(range(6))
    assert {m["end_phase"] for m in ms} >= {"navigation", "mapping", "exploration", "landing", "emergency"}
    assert {m["W"] for m in ms} == set(range(5)) and {m["safety_margin"] for m in ms} == {1.5, 2.0, 2.5}
    assert {n for m in ms for n in m["labels"]} == {"safe_zone", "obstacle", "landing_pad", "doorway"}
    assert all(m["calls"] == 28 for m in ms if m["safety_margin"] == 2.0) and all(28 <= m["calls"] <= 60 for m in ms)
    assert sum(m["use_neural_scene"] for m in ms) == 4 and {m["preset"] for m in ms} == {None, "exploration", "mapping"}
    assert any(m["z0"] < 0.5 and g[m["key"] + "phase"][0] == mo.EMERGENCY for m in ms)
