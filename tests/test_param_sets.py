"""tests/param_sets.py can tell the fields of se3mpc_params apart: on the oracle alone (no device), with the inputs the device checks use,
every swap of two fields inside set A or B, and every single field set to 1.0 or to its reference default, moves at least one output that the
device checks compare by more than 100 x that output's float32 tolerance.  A kernel that reads the wrong constant therefore fails the
checks of tests/test_emu_params.py / tests/test_gpu_params.py with a margin of two decimal orders.  CPU only."""
import dataclasses
import itertools

import numpy as np
import pytest

import mppi_checks as mc
import mppi_oracle as mo
import param_sets as ps
import parity_checks as pc
from oracle import se3mpc_oracle as orc

MARGIN = 100.0
N, B = 6, 70                       # the smallest shape of the device checks


def test_sets_are_what_they_claim():
    for name in ("A", "B"):
        vals = list(ps.SETS[name].values())
        assert len(set(vals)) == len(vals), "no two fields equal"
        assert not set(vals) & {0.0, 1.0, 2.0}
        assert all(ps.SETS[name][f] != ps.DEFAULTS[f] for f in ps.FIELDS)
    assert set(ps.SETS["C"]) == set(ps.FIELDS)
    for name in ps.SETS:
        assert set(ps.SETS[name]) == set(ps.FIELDS) and ps.oracle_config(name, 6).hover_thrust == ps.SETS[name]["mass"] * ps.SETS[name]["gravity"]


def inputs(name):
    """What check_lane_kernels (seed = N), check_rollout_iterate_obstacles' scene and mppi_checks.problem build at this set."""
    cfg = ps.oracle_config(name, N)
    rng = np.random.default_rng(N)
    p0, v0, goal, T = pc.random_batch(rng, B, N, cfg=cfg)
    X = pc.lane_decision_vectors(rng, B, N, T, cfg)
    sph = pc.lane_spheres(rng)
    Xn = pc.near_sphere_vectors(X, N, N)
    _, mcfg, mp0, mv0, mgoal, U, msph = mc.problem(N, 3, 5, K=3, params=ps.overrides(name))
    Ts = np.stack([mo.samples(U[p], p, 2, 64, 1.0, 5, mcfg)[0] for p in range(3)])
    assert mcfg == cfg                                                    # (the set's own dt overrides mppi_checks.problem's 0.1 s)
    return dict(p0=p0, v0=v0, goal=goal, T=T, X=X, sph=sph, Xn=Xn, mp0=mp0, mv0=mv0, mgoal=mgoal, Ts=Ts, msph=msph)


def outputs(cfg, i):
    """name -> (array, kind, float32 tolerance): 'rel' = elementwise relative, 'vec' = of the array's largest magnitude (parity_checks.vec_close),
    'abs' = absolute.  The tolerances are parity_checks.F32's and mppi_checks.F32_COST_REL, with the factors the checks apply."""
    t = pc.F32
    o = {}
    o["objective"] = (orc.objective(i["X"], i["goal"], cfg), "rel", t["cost_rel"])
    o["gradient"] = (orc.gradient(i["X"], i["goal"], cfg), "vec", t["vec_rel"])
    c, g = orc.rollout_cost_grad(i["p0"], i["v0"], i["goal"], i["T"], cfg)
    o["rollout cost"] = (c, "rel", t["cost_rel"])
    o["rollout gradient"] = (g, "vec", t["vec_rel"])
    b = orc.bounds(cfg)
    for nm, blk in (("position", b[:3 * N]), ("velocity", b[3 * N:6 * N]), ("thrust", b[6 * N:])):       # each block is met by its own variables
        o["bounds " + nm] = (blk, "vec", t["vec_rel"] * 10)
    o["straight_line_init"] = (orc.straight_line_init(i["p0"], i["v0"], i["goal"], cfg), "vec", t["vec_rel"] * 10)
    o["dynamics_residual"] = (orc.dynamics_residual(i["X"], i["p0"], i["v0"], cfg), "vec", t["vec_rel"])
    o["physical_constraints"] = (orc.physical_constraints(i["X"], cfg), "vec", t["vec_rel"])
    o["obstacle_residual"] = (orc.obstacle_residual(i["Xn"], i["sph"][:, :3], i["sph"][:, 3], cfg), "vec", t["vec_rel"])
    ex = orc.extract_solution_batch(i["X"][:8], cfg)
    o["extract accelerations"] = (ex["accelerations"], "vec", t["vec_rel"])
    o["extract body_rates"] = (ex["body_rates"], "abs", t["rates"])
    o["mppi cost"] = (np.stack([mo.cost(i["mp0"][p], i["mv0"][p], i["mgoal"][p], i["Ts"][p], cfg, i["msph"], 40.0) for p in range(3)]), "rel",
                      mc.F32_COST_REL)
    return o


def moved(ref, new):
    """The outputs that moved by more than MARGIN x their float32 tolerance."""
    names = []
    for k, (a, kind, tol) in ref.items():
        b = new[k][0]
        d = np.abs(b - a)
        if kind == "rel":
            far = np.max(d / np.abs(a)) > MARGIN * tol
        elif kind == "vec":
            far = np.max(d) > MARGIN * tol * max(1.0, float(np.max(np.abs(a))))
        else:
            far = np.max(d) > MARGIN * tol
        if far:
            names.append(k)
    return names


@pytest.mark.parametrize("name", ["A", "B"])
def test_param_sets_discriminate(name):
    base = ps.SETS[name]
    i = inputs(name)
    cfg0 = ps.oracle_config(name, N)
    ref = outputs(cfg0, i)
    changes = [(x, y, base[y]) for x, y in itertools.permutations(ps.FIELDS, 2)]
    changes += [(x, "1.0", 1.0) for x in ps.FIELDS] + [(x, "default", ps.DEFAULTS[x]) for x in ps.FIELDS]
    blind, fewest = [], (99, None, None)
    for x, y, val in changes:
        seen = moved(ref, outputs(dataclasses.replace(cfg0, **{x: val}), i))
        if not seen:
            blind.append((x, y, val))
        fewest = min(fewest, (len(seen), x, y))
    print(f"set {name}: {len(changes)} changes, the least visible one ({fewest[1]} <- {fewest[2]}) moves {fewest[0]} outputs")
    assert not blind, f"set {name}: these changes move no compared output by {MARGIN:g} x its float32 tolerance: {blind}"
