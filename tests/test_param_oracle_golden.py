"""The oracle OFF THE REFERENCE'S DEFAULT PARAMETERS against vectors produced by the reference itself (tests/golden/make_golden_params.py:
sets A and B of tests/param_sets.py; terminal factor and position box at their defaults, which the reference hard-codes), to the tolerances
tests/test_oracle_golden.py uses for the same quantities; and the oracle's terminal_factor, which no reference vector can pin, through the
directional-derivative identity of the rollout cost.  CPU only."""
import json
import os

import numpy as np
import pytest

import param_sets as ps
from oracle import se3mpc_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = dict(rtol=1e-12, atol=1e-10)


@pytest.fixture(scope="module")
def golden_params():
    return np.load(os.path.join(GOLDEN, "param_cases.npz")), json.load(open(os.path.join(GOLDEN, "param_cases.json")))


def cfg_for(c, **kw):
    return orc.OracleConfig(prediction_horizon=c["N"], **{**c["params"], **kw})


def test_generator_restates_the_sets(golden_params):
    _, meta = golden_params
    for c in meta["cases"]:
        assert c["params"] == ps.overrides(c["set"], reference_expressible=True) and c["dt"] == ps.SETS[c["set"]]["dt"]


def test_path_functions_at_the_sets(golden_params):
    data, meta = golden_params
    cases = [c for c in meta["cases"] if c["kind"] == "path"]
    assert sorted((c["set"], c["N"]) for c in cases) == [(s, N) for s in "AB" for N in (1, 6, 30)]
    for c in cases:
        k, cfg = c["key"], cfg_for(c)
        goal, p0, v0, X = data[k + "goal"], data[k + "p0"], data[k + "v0"], data[k + "X"]
        assert np.allclose(orc.objective(X, goal, cfg), data[k + "f"], rtol=1e-13, atol=1e-9), k
        assert np.allclose(orc.gradient(X, goal, cfg), data[k + "g"], **TOL), k
        assert np.allclose(orc.dynamics_residual(X, p0, v0, cfg), data[k + "dyn"], **TOL), k
        assert np.allclose(orc.physical_constraints(X, cfg), data[k + "phys"], **TOL), k
        assert np.allclose(orc.obstacle_residual(data[k + "Xo"], data[k + "obs_c"], data[k + "obs_r"], cfg), data[k + "obs"], **TOL), k
        assert c["N"] == 1 or np.any(data[k + "obs"] < 0), k                   # (some positions are inside a margin)
        assert np.allclose(orc.straight_line_init(p0, v0, goal, cfg), data[k + "x0_init"], **TOL), k
        assert np.allclose(orc.bounds(cfg), data[k + "bounds"], **TOL), k
        ex = orc.extract_solution_batch(data[k + "Xe"], cfg)
        for name in ("accelerations", "attitudes", "body_rates", "thrusts"):
            assert np.allclose(ex[name], data[k + "ex_" + name], rtol=1e-11, atol=1e-9), (k, name)
        for x, f, g in zip(X[:2], data[k + "f"], data[k + "g"]):
            assert np.isclose(orc.objective_loops(x, goal, cfg), f, rtol=1e-14, atol=0), k
            assert np.isclose(orc.objective_ordered(x, goal, cfg), f, rtol=1e-14, atol=0), k
            assert np.allclose(orc.gradient_loops(x, goal, cfg), g, rtol=1e-15, atol=0), k


def test_solves_at_the_sets(golden_params):
    data, meta = golden_params
    cases = [c for c in meta["cases"] if c["kind"] == "solve"]
    assert sorted((c["set"], c["N"]) for c in cases) == [(s, N) for s in "AB" for N in (6, 6, 6, 20, 20, 20)]
    for c in cases:
        k = c["key"]
        cfg = cfg_for(c, max_iterations=c["maxiter"], convergence_tolerance=c["tol"])
        p0, v0, goal = data[k + "p0"], data[k + "v0"], data[k + "goal"]
        assert np.allclose(orc.straight_line_init(p0, v0, goal, cfg), data[k + "x0"], **TOL), k
        assert np.allclose(orc.bounds(cfg), data[k + "bounds"], **TOL), k
        tr, info = orc.plan(p0, v0, goal, cfg)
        assert (info["nit"], info["nfev"], info["status"]) == (c["nit"], c["nfev"], c["status"]), (k, info)
        assert np.allclose(tr["x"], data[k + "x"], **TOL), k
        for name in ("positions", "velocities", "accelerations", "attitudes", "body_rates", "thrusts"):
            assert np.allclose(tr[name], data[k + name], rtol=1e-11, atol=1e-9), (k, name)


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("term", [0.0, 4.0, 27.0, 10.0])
def test_terminal_factor_of_the_rollout_gradient(name, term):
    """The reference hard-codes the terminal factor, so no vector of its making pins the oracle's `terminal_factor`.  The rollout cost is
    quadratic in T: its central difference along any direction is exact up to rounding and must equal g . d with the adjoint gradient --
    which carries the factor as (1 + terminal_factor) on the last step's position error, while the cost carries it in the objective.
    Tolerance: identity (3) of tests/test_gpu_parity.py::test_full_size_rollout_properties, |g.d - fd| <= 2e-5 sum |g d|."""
    rng = np.random.default_rng(17)
    for N in (1, 6, 30):
        cfg = ps.oracle_config(name, N, terminal_factor=term)
        B = 5
        p0, v0, goal = rng.uniform(-20, 20, (B, 3)), rng.uniform(-5, 5, (B, 3)), rng.uniform(-20, 20, (B, 3))
        T = rng.normal(0, 2, (B, N, 3)) + [0, 0, cfg.hover_thrust]
        d = rng.normal(0, 1, (B, N, 3))
        c, g = orc.rollout_cost_grad(p0, v0, goal, T, cfg)
        P, V = orc.rollout(p0, v0, T, cfg)
        X = orc.pack(P, V, T)
        assert np.allclose(c, orc.objective(X, goal, cfg), rtol=1e-14)
        assert np.allclose(c, [orc.objective_loops(X[b], goal[b], cfg) for b in range(B)], rtol=1e-13)
        assert np.allclose(c, [orc.objective_ordered(X[b], goal[b], cfg) for b in range(B)], rtol=1e-13)
        # the terminal term itself: cost(term) - cost(0) = term * wp * |P_last - goal|^2
        c0 = orc.rollout_cost(p0, v0, goal, T, ps.oracle_config(name, N, terminal_factor=0.0))
        assert np.allclose(c - c0, term * cfg.position_weight * np.sum((P[:, -1] - goal) ** 2, axis=-1), rtol=1e-10, atol=1e-9 * np.max(c))
        fd = (orc.rollout_cost(p0, v0, goal, T + d, cfg) - orc.rollout_cost(p0, v0, goal, T - d, cfg)) / 2
        gd = np.sum(g * d, axis=(-1, -2))
        assert np.all(np.abs(gd - fd) <= 2e-5 * np.sum(np.abs(g * d), axis=(-1, -2))), (N, gd, fd)
