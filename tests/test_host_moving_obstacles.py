"""CPU, no library: the host side of SE3MPCPlanner's moving obstacles -- the (K, 7) table, its float64 rebase to the state's timestamp,
and obstacle_clearance at each row's timestamp against a hand-computed case."""
import numpy as np
import pytest

from dart_planner_amd.common.types import Trajectory
from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner


def planner():
    return SE3MPCPlanner(SE3MPCConfig(prediction_horizon=4))


def test_table_rows_and_rebase():
    pl = planner()
    assert pl._moving_obstacle_table(None, 5.0) is None
    pl.add_obstacle(np.array([1.0, 2.0, 3.0]), 0.5)
    pl.add_moving_obstacle(np.array([0.0, -1.0, 2.0]), 0.25, np.array([2.0, 0.0, -1.0]), 4.0)
    tab = pl._moving_obstacle_table(None, 5.5)
    assert tab.shape == (2, 7) and tab.dtype == np.float64
    assert tab[0].tolist() == [1.0, 2.0, 3.0, 0.5, 0.0, 0.0, 0.0], "static obstacles come first, with zero velocity"
    assert tab[1].tolist() == [3.0, -1.0, 0.5, 0.25, 2.0, 0.0, -1.0], "centre + velocity * (now - timestamp)"
    assert np.array_equal(pl._obstacle_table(None), [[1.0, 2.0, 3.0, 0.5]]), "_obstacle_table is the static list, as before"
    assert pl._moving_obstacle_table(False, 5.5) is None
    sph, moving = pl._mppi_tables(None, 5.5)
    assert np.array_equal(sph, tab[:, :4]) and np.array_equal(moving, tab)
    pl.clear_obstacles()
    assert pl.obstacles == [] and pl.moving_obstacles == [] and pl._moving_obstacle_table(None, 5.5) is None


def test_rebase_is_float64_at_epoch_timestamps():
    """At t = 1.7e9 s a float32 clock has an ulp of 128 s; the rebase subtracts in float64 first, so the kernel only sees seconds."""
    pl, ref = planner(), planner()
    pl.add_moving_obstacle(np.array([0.0, 0.0, 2.0]), 0.3, np.array([1.5, -2.0, 0.25]), 1.7e9 - 0.75)
    ref.add_moving_obstacle(np.array([0.0, 0.0, 2.0]), 0.3, np.array([1.5, -2.0, 0.25]), -0.75)
    a, b = pl._moving_obstacle_table(None, 1.7e9), ref._moving_obstacle_table(None, 0.0)
    assert np.array_equal(a, b) and a[0, :3].tolist() == [1.125, -1.5, 2.1875]


def test_explicit_tables():
    pl = planner()
    pl.add_moving_obstacle(np.zeros(3), 1.0, np.ones(3), 0.0)
    four = np.array([[1.0, 2.0, 3.0, 0.5], [4.0, 5.0, 6.0, 0.25]])
    tab = pl._moving_obstacle_table(four, 9.0)
    assert np.array_equal(tab[:, :4], four) and np.all(tab[:, 4:] == 0), "(K, 4): static"
    assert pl._mppi_tables(four, 9.0)[1] is None, "no velocity: the static entry serves"
    seven = np.array([[1.0, 2.0, 3.0, 0.5, 0.0, 1.0, 0.0]])
    assert np.array_equal(pl._moving_obstacle_table(seven, 9.0), seven), "(K, 7): taken to hold at the state's timestamp"
    assert pl._mppi_tables(seven, 9.0)[1] is not None
    assert pl._moving_obstacle_table(np.zeros((0, 4)), 0.0) is None and pl._moving_obstacle_table(np.zeros((0, 7)), 0.0) is None


def test_obstacle_clearance_follows_the_obstacle():
    """A trajectory standing still at the origin's height while a sphere of radius 0.5 m passes: residual |p - c(t)|^2 - (r + margin)^2 at
    each row's own timestamp, by hand."""
    pl = planner()
    margin = pl.se3_config.safety_margin
    pl.add_moving_obstacle(np.array([-4.0, 0.0, 1.0]), 0.5, np.array([2.0, 0.0, 0.0]), 100.0)
    ts = 100.0 + np.array([0.0, 1.0, 2.0, 3.0])
    P = np.tile([0.0, 0.0, 1.0], (4, 1))
    z = np.zeros((4, 3))
    tr = Trajectory(timestamps=ts, positions=P, velocities=z, accelerations=z)
    d2 = np.array([16.0, 4.0, 0.0, 4.0])                              # the centre is at x = -4, -2, 0, 2
    res = d2 - (0.5 + margin) ** 2
    out = pl.obstacle_clearance(tr)
    assert out["min_residual"] == pytest.approx(res.min(), abs=1e-12) and out["min_residual"] == pytest.approx(-(0.5 + margin) ** 2, abs=1e-12)
    assert out["violation"] == pytest.approx(np.sum(np.maximum(0.0, -res)), abs=1e-12)
    # a snapshot at the table's time would have seen 16 m^2 at every row
    assert out["min_residual"] < 16.0 - (0.5 + margin) ** 2


def test_static_entries_get_the_snapshot():
    """What plan_shooting hands the static kernels: the (K, 4) part of the rebased table."""
    pl = planner()
    pl.add_obstacle(np.array([1.0, 2.0, 3.0]), 0.5)
    pl.add_moving_obstacle(np.array([0.0, -1.0, 2.0]), 0.25, np.array([2.0, 0.0, -1.0]), 4.0)
    sph, moving = pl._mppi_tables(None, 5.5)
    assert sph.flags["C_CONTIGUOUS"] and sph.tolist() == [[1.0, 2.0, 3.0, 0.5], [3.0, -1.0, 0.5, 0.25]] and moving.shape == (2, 7)
