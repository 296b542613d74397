"""CPU: tests/smoother_oracle.py (the float64 NumPy restatement of the reference's TrajectorySmoother) against tests/golden/smoother_cases.npz, the
vectors of the reference's own class: every recorded call to 1e-10 (the reference's t**3 goes through pow, so this is not bit-exact), branch
codes, clocks and flag bits exact."""
import numpy as np
import pytest

import smoother_checks as sc
import smoother_oracle as so

DATA, META = sc.golden()


def oracle_params(seq):
    return so.params(transition_time=seq["transition_time"], **seq["members"])


@pytest.mark.parametrize("seq", META["sequences"], ids=lambda s: s["tag"])
def test_sequence(seq):
    key, prm = seq["key"], oracle_params(seq)
    state, cur = so.reset(1), None
    for e in range(seq["events"]):
        t = np.array([DATA[key + "t"][e]])
        if DATA[key + "kind"][e] == 1:
            new = sc.golden_plan(DATA, key, int(DATA[key + "plan"][e]))
            so.update(prm, state, t, cur, new)
            cur = new
        else:
            x, br = so.desired(prm, state, t, DATA[key + "pos"][e][None], DATA[key + "vel"][e][None], cur)
            assert br[0] == DATA[key + "branch"][e], e
            assert np.max(np.abs(x[0] - DATA[key + "out"][e])) <= 1e-10, e
        ref = DATA[key + "state"][e]
        assert np.array_equal(state[0, 21:25], ref[21:25]) and np.max(np.abs(state[0, :21] - ref[:21])) <= 1e-10, e


def test_fixtures_cover_what_the_issue_lists():
    assert len(META["sequences"]) >= 12 and len(META["loops"]) == 4
    assert min(META["hits"]["branch"]) >= 5 and min(META["hits"]["clamps"].values()) >= 5
    rows = {DATA[f"{s['key']}pl{pi}_ts"].shape[0] for s in META["sequences"] for pi in range(s["plans"])}
    assert {1, 2, 6, 30} <= rows
    for s in META["sequences"]:
        assert 60 <= s["calls"] <= 300 and s["events"] - s["calls"] <= 5
    sw = [l for l in META["loops"] if l["tag"] == "switch"][0]
    assert sw["smoothed_jump"] < 0.25 * sw["raw_jump"]


def test_float32_evaluation_of_the_oracle_stays_inside_the_float32_bound():
    """The yardstick of the float32 kernels: the oracle evaluated in NumPy float32 against itself in float64 on every golden sequence."""
    worst = {}
    for seq in META["sequences"]:
        key, prm = seq["key"], oracle_params(seq)
        s64, s32, cur, err = so.reset(1), so.reset(1), None, 0.0
        for e in range(seq["events"]):
            t = np.array([DATA[key + "t"][e]])
            if DATA[key + "kind"][e] == 1:
                new = sc.golden_plan(DATA, key, int(DATA[key + "plan"][e]))
                so.update(prm, s64, t, cur, new)
                so.update(prm, s32, t, sc.rounded(cur, np.float32), sc.rounded(new, np.float32), dtype=np.float32)
                cur = new
            else:
                p, v = DATA[key + "pos"][e][None], DATA[key + "vel"][e][None]
                a, ba = so.desired(prm, s64, t, p, v, cur)
                b, bb = so.desired(prm, s32, t, p, v, sc.rounded(cur, np.float32), dtype=np.float32)
                assert ba[0] == bb[0]
                err = max(err, float(np.max(np.abs(a - b.astype(float)))))
        worst[seq["tag"]] = err
    print({k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst.values()) <= 1e-4
