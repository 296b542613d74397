"""Parameter sets off the reference's defaults, for the plan path's device checks (tests/test_emu_params.py, tests/test_gpu_params.py).

At `Params.reference_defaults()` several fields of se3mpc_params hide each other (velocity_weight == terminal_factor == max_velocity == 10,
position_weight == position_bound == 100, mass == safety_margin == 1.5, acceleration_weight == 1), so a kernel that reads one where another
belongs passes every check made there.  Within A and within B no two fields are equal, none is 0, 1 or 2 and none equals its default; C holds
the edges (zero weights, zero margin, zero minimum thrust).  tests/test_param_sets.py proves on the oracle alone that swapping any two fields of A
or of B, or putting 1.0 or the default into one, moves an output the device checks compare by more than 100 x its float32 tolerance.
"""
import numpy as np

from oracle import se3mpc_oracle as orc

FIELDS = ("dt", "mass", "gravity", "position_weight", "velocity_weight", "acceleration_weight", "thrust_weight", "terminal_factor",
          "position_bound", "max_velocity", "max_acceleration", "max_thrust", "min_thrust", "max_tilt_angle", "safety_margin")

_ROWS = {
    "A": (0.05, 0.9, 3.72, 37.0, 6.5, 0.35, 0.8, 4.0, 55.0, 7.0, 11.0, 17.0, 1.25, 0.6, 0.7),
    "B": (0.02, 2.3, 11.5, 8.0, 21.0, 3.0, 0.045, 27.0, 140.0, 13.0, 19.0, 48.0, 3.5, 0.35, 2.2),
    "C": (0.1, 1.7, 9.6, 60.0, 4.0, 0.0, 0.3, 0.0, 30.0, 6.0, 9.0, 22.0, 0.0, 1.2, 0.0),
}
SETS = {name: dict(zip(FIELDS, row)) for name, row in _ROWS.items()}

# The reference hard-codes the terminal factor 10 and the +-100 m box (planner.py:548, :383-384): vectors made by the reference itself
# (tests/golden/make_golden_params.py) use A and B with these two left at their defaults.
REFERENCE_FIXED = ("terminal_factor", "position_bound")

DEFAULTS = {f: getattr(orc.OracleConfig(), f) for f in FIELDS}

# Projected-gradient steps of check_rollout_iterate / check_rollout_iterate_obstacles (and the obstacle loop's weight) at which the FLOAT64
# ORACLE chain itself descends for every trajectory of the batch; the checks assert that on the oracle's own c_first / c_final before the
# device is called.  The plain loop's objective is quadratic in T, and a projected step of at most 1 / L descends on a box, L = the largest
# eigenvalue of its Hessian.  L was measured on the oracle's gradient (orc.rollout_cost_grad is linear in T: one column per unit thrust):
#       N =    6        7        30       33
#   A        3.09     3.39     69.3     94.9        (dt = 0.05: the rollout terms, which carry dt^2 / m per step, dominate at N = 30)
#   B        1.26     1.28     2.48     2.77
#   C        1.23     1.64     263.8    386.0
# (The default check's 0.9 is such a step at the defaults only: there 2 (wa / m^2 + wT) = 1.09 and dt = 1/400 s leaves nothing else.)
# `step` below is ~0.9 / L of the bucket's largest horizon.
# The obstacle loop (dt = the set's own, weight 40 as the default check) starts from thrusts drawn 3 N about hover, many of them outside the
# small boxes of A and C: the first projection alone can RAISE the cost, and the default check's step 2e-3 does not win that back in three
# iterations (oracle, float64, N = 6, B = 70: 4 of 70 trajectories of A end above their start, by up to 0.7 %; 2 of C's).  Measured on the
# oracle chain, trajectories that end above their start / largest relative change of the cost, 3 iterations, float64 and float32-rounded
# inputs alike:          step = 0.005      0.01           0.02           0.05
#   A (6, 70)            1 / +0.2 %     0 / -0.39 %    0 / -0.63 %    0 / -1.3 %
#   A (30, 66)           0              0 / -22 %      0 / -24 %      44 of 66 rise (past 1 / L of the horizon-30 rollout terms)
#   B (6, 70), (30, 66)  0              0              0 / -0.9 %     0
#   C (6, 70)            0              0 / -0.27 %    0 / -0.52 %    0 / -1.2 %
ITERATE = {
    "A": dict(step={7: 0.29, 33: 0.0095}, obstacle_step=0.01, obstacle_weight=40.0),
    "B": dict(step={7: 0.7, 33: 0.32}, obstacle_step=0.02, obstacle_weight=40.0),
    "C": dict(step={7: 0.55, 33: 0.0023}, obstacle_step=0.02, obstacle_weight=40.0),
}

# Seed of mppi_checks.problem for the MPPI checks at the sets: with the small safety margins of A (0.7 m against the default 1.5 m) the
# check's own precondition -- a nominal inside a sphere's margin -- needs a scene that has one; at seed 9 every nominal of every shape the
# parameter tests run is inside a margin, for A and for B (found on the oracle's penalty alone).
MPPI_SEED = 9


def iterate_step(name, N):
    """The plain loop's step for horizon N (the smallest bucket that holds it)."""
    return next(v for n, v in sorted(ITERATE[name]["step"].items()) if N <= n)


def overrides(name, reference_expressible=False):
    """The set as keyword overrides of Params.reference_defaults / check functions' `params`."""
    d = dict(SETS[name])
    if reference_expressible:
        for f in REFERENCE_FIXED:
            d.pop(f)
    return d


def oracle_config(name, N, **extra):
    return orc.OracleConfig(prediction_horizon=N, **{**SETS[name], **extra})


# ------------------------------------------------------------------ the one-launch closed loops: a different constant in every block
# The closed-loop kernels take up to four blocks that each carry a mass, a gravity and a max_thrust (planner, controller, simulator,
# OnboardController) and the mixer's max_thrust.  Where two blocks agree -- planner and simulator both have mass 1.5 and g 9.81 at the
# reference defaults -- a fused kernel that reads the wrong block's constant still equals its chain.  Here no two agree.
LOOP_BLOCKS = dict(planner=dict(mass=1.3, gravity=9.7, max_thrust=23.0), controller=dict(mass=1.1, gravity=9.9, max_thrust=21.0),
                   simulator=dict(mass=1.6, gravity=9.6, max_thrust=19.0), onboard=dict(mass=1.2, g=9.75), mixer=dict(max_thrust=9.0))
LOOP_SHAPE = dict(N=6, B=3, cycles=2, substeps=3, K=2)


def loop_blocks(N, **planner_own):
    """-> dict(prm, cp, sp, op, mixer, ccfg, sim): the C-ABI parameter structs at LOOP_BLOCKS and the oracle's configurations that state
    the same controller and simulator."""
    from dart_planner_amd.capi import ControllerParams, MixerParams, OnboardParams, Params, SimulatorParams
    from oracle import controller_oracle as co
    ccfg = co.ControllerConfig(**LOOP_BLOCKS["controller"])
    sim = co.SimulatorConfig(**LOOP_BLOCKS["simulator"])
    return dict(prm=Params.reference_defaults(**{**dict(horizon=N), **planner_own, **LOOP_BLOCKS["planner"]}),
                cp=ControllerParams.from_config(ccfg), sp=SimulatorParams.reference_defaults(**LOOP_BLOCKS["simulator"]),
                op=OnboardParams.reference_defaults(**LOOP_BLOCKS["onboard"]), mixer=MixerParams.reference_defaults(**LOOP_BLOCKS["mixer"]),
                ccfg=ccfg, sim=sim)
