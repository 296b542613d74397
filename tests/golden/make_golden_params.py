#!/usr/bin/env python3
"""Golden vectors OFF THE REFERENCE'S DEFAULT PARAMETERS, made by running the reference itself (build container only, as make_golden.py:
the same identity-units stand-ins, the reference imported from where it lies, SE3MPC_GOLDEN_OUT for the reproducibility test).

Every fixture made by make_golden.py sits at the defaults of SE3MPCConfig, where several fields have the same value (velocity weight =
max velocity = 10, mass = safety margin = 1.5, acceleration weight = 1) and a restatement that reads one for the other cannot be told from
a right one.  Here each case builds the reference's own SE3MPCPlanner with a SE3MPCConfig that carries the fields of parameter set A or B
of tests/param_sets.py (the values are restated below: this script must run without the test tree on sys.path), dt injected the way
make_golden.py's make_planner does it, and mass / gravity / hover_thrust assigned after construction (planner.py:149-151 sets them in the
constructor).  The reference hard-codes the terminal factor 10 and the +-100 m position box, so those two stay at their defaults.

Recorded: what the d??_ cases of path_functions record (objective, gradient, dynamics / physical / obstacle constraints, cold start, box,
extraction) for N in {1, 6, 30} and 4 decision vectors each, and three plan_trajectory solves per set at N = 6 and N = 20.

Usage:  python tests/golden/make_golden_params.py      (rewrites tests/golden/param_cases.npz, param_cases.json)
"""
import dataclasses
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_standins  # noqa: E402

OUT_DIR = os.environ.get("SE3MPC_GOLDEN_OUT", HERE)

# tests/param_sets.py, sets A and B, without terminal_factor and position_bound (literals in the reference)
SETS = {
    "A": dict(dt=0.05, mass=0.9, gravity=3.72, position_weight=37.0, velocity_weight=6.5, acceleration_weight=0.35, thrust_weight=0.8,
              max_velocity=7.0, max_acceleration=11.0, max_thrust=17.0, min_thrust=1.25, max_tilt_angle=0.6, safety_margin=0.7),
    "B": dict(dt=0.02, mass=2.3, gravity=11.5, position_weight=8.0, velocity_weight=21.0, acceleration_weight=3.0, thrust_weight=0.045,
              max_velocity=13.0, max_acceleration=19.0, max_thrust=48.0, min_thrust=3.5, max_tilt_angle=0.35, safety_margin=2.2),
}
CONFIG_FIELDS = ("position_weight", "velocity_weight", "acceleration_weight", "thrust_weight", "max_velocity", "max_acceleration",
                 "max_thrust", "min_thrust", "max_tilt_angle", "safety_margin")


def main():
    tmp = _install_standins()
    try:
        import logging
        logging.disable(logging.CRITICAL)
        import scipy
        import dart_planner.planning.se3_mpc_planner as ref_mod
        from dart_planner.planning.se3_mpc_planner import SE3MPCPlanner, SE3MPCConfig
        from dart_planner.common.types import DroneState

        real_minimize = ref_mod.minimize
        captured = {}

        def spy_minimize(*a, **k):
            res = real_minimize(*a, **k)
            captured["res"] = res
            captured["x0"] = np.array(k.get("x0", a[1] if len(a) > 1 else None), dtype=float)
            captured["bounds"] = np.array([[float(lo), float(hi)] for lo, hi in k["bounds"]])
            return res

        ref_mod.minimize = spy_minimize

        def make_planner(s, N, tol=None, maxiter=None):
            kw = dict(prediction_horizon=N, **{f: s[f] for f in CONFIG_FIELDS})
            if tol is not None:
                kw["convergence_tolerance"] = tol
            if maxiter is not None:
                kw["max_iterations"] = maxiter
            p = SE3MPCPlanner(SE3MPCConfig(**kw))
            p.se3_config = dataclasses.replace(p.se3_config, dt=s["dt"])      # the ctor forces dt = 1/400 (planner.py:99-105)
            p.mass = np.asarray(s["mass"], float)
            p.gravity = np.asarray(s["gravity"], float)
            p.hover_thrust = p.mass * p.gravity
            return p

        def state(p0, v0):
            return DroneState(timestamp=123.0, position=np.array(p0, float), velocity=np.array(v0, float), attitude=np.zeros(3),
                              angular_velocity=np.zeros(3))

        out, meta = {}, []
        rng = np.random.default_rng(20261020)
        idx = 0
        for name, s in SETS.items():
            hover = s["mass"] * s["gravity"]
            # ------------------------------------------------- direct calls of path functions
            for N in (1, 6, 30):
                pl = make_planner(s, N)
                goal = rng.uniform(-20, 20, 3)
                pl.set_goal(goal)
                p0, v0 = rng.uniform(-20, 20, 3), rng.uniform(-5, 5, 3)
                st = state(p0, v0)
                # inside and outside the box: +-1.2 x the 100 m position box, +-1.5 x this set's velocity box, thrusts about ITS hover thrust
                X = np.concatenate([rng.uniform(-120, 120, (4, 3 * N)), rng.uniform(-1.5, 1.5, (4, 3 * N)) * s["max_velocity"],
                                    rng.normal(0, 6, (4, 3 * N)) + np.tile([0, 0, hover], N)], axis=1)
                k = f"d{idx:02d}_"; idx += 1
                out[k + "p0"], out[k + "v0"], out[k + "goal"] = p0, v0, goal
                out[k + "X"] = X
                out[k + "f"] = np.array([pl._objective_function(x) for x in X])
                out[k + "g"] = np.array([pl._objective_gradient(x) for x in X])
                out[k + "dyn"] = np.array([pl._dynamics_constraints(x, st, N) for x in X])
                out[k + "phys"] = np.array([pl._physical_constraints(x, N) for x in X])
                out[k + "x0_init"] = pl._create_straight_line_initialization(st, N)
                out[k + "bounds"] = np.array([[float(a), float(b)] for a, b in pl._setup_optimization_bounds(N)])
                K = 5
                centres = np.round(rng.uniform(0, 15, (K, 3)) * 2) / 2
                radii = np.where(np.arange(K) % 3 == 0, 1.0, rng.uniform(0.3, 2.5, K))
                for cc, rr in zip(centres, radii):
                    pl.add_obstacle(cc, np.float64(rr))
                # two of the four vectors about a metre from sphere centres: residuals of the size of (r + margin)^2 itself, some negative
                Xo = X.copy()
                Xo[:2, :3 * N] = (centres[rng.integers(K, size=(2, N))] + rng.normal(0, 1.0, (2, N, 3))).reshape(2, -1)
                out[k + "obs_c"], out[k + "obs_r"], out[k + "Xo"] = centres, radii, Xo
                out[k + "obs"] = np.array([pl._obstacle_constraints(x, N) for x in Xo])
                Xe = X.copy()
                T = Xe[:, 6 * N:].reshape(4, N, 3)
                if N >= 6:
                    T[0, 1] = 0.0; T[0, 3] = [7.0, 0.0, 0.0]; T[1, 0] = 0.0; T[1, 2] = [-3.0, 0.0, 0.0]; T[2, 4] = [0.0, 5.0, 0.0]
                    T[3, 2] = [1e-7, 0.0, 0.0]
                sols = [pl._extract_solution_from_result(x, N) for x in Xe]
                out[k + "Xe"] = Xe
                for nm in ("accelerations", "attitudes", "body_rates", "thrusts"):
                    out[k + "ex_" + nm] = np.array([sol[nm] for sol in sols])
                meta.append(dict(key=k, kind="path", set=name, N=N, dt=float(pl.se3_config.dt), K=K, params=s))
            # ------------------------------------------------- solves
            for N, tol, maxiter in ((6, None, None), (6, None, None), (6, 1e-9, 40), (20, None, None), (20, None, None), (20, 1e-9, 40)):
                pl = make_planner(s, N, tol=tol, maxiter=maxiter)
                p0, v0, goal = rng.uniform(-20, 20, 3), rng.uniform(-5, 5, 3), rng.uniform(-20, 20, 3)
                tr = pl.plan_trajectory(state(p0, v0), goal)
                res = captured["res"]
                k = f"s{idx:02d}_"; idx += 1
                out[k + "p0"], out[k + "v0"], out[k + "goal"] = p0, v0, goal
                out[k + "x0"], out[k + "bounds"] = captured["x0"], captured["bounds"]
                out[k + "x"] = np.array(res.x, float)
                out[k + "fun"] = np.array(float(res.fun))
                for nm in ("positions", "velocities", "accelerations", "attitudes", "body_rates", "thrusts"):
                    out[k + nm] = np.array(getattr(tr, nm), float)
                meta.append(dict(key=k, kind="solve", set=name, N=N, dt=float(pl.se3_config.dt), tag="params_" + name,
                                 tol=float(pl.se3_config.convergence_tolerance), maxiter=int(pl.se3_config.max_iterations),
                                 nit=int(res.nit), nfev=int(res.nfev), status=int(res.status), success=bool(res.success),
                                 message=str(res.message), params=s))
        np.savez_compressed(os.path.join(OUT_DIR, "param_cases.npz"), **out)
        with open(os.path.join(OUT_DIR, "param_cases.json"), "w") as f:
            json.dump(dict(scipy=scipy.__version__, numpy=np.__version__, cases=meta), f, indent=1)
        print("wrote param_cases.npz / param_cases.json:", len(meta), "cases")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
