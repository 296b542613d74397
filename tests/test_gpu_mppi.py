"""GPU suite (`-m gpu`): the MPPI planner of dart_planner_amd/csrc/mppi.hip on a real MI355X through the C ABI and Ops -- the checks of
the host-emulation suite at device sizes, the composed iteration, run-to-run identity, BASELINE config 5's shape (4096 problems x 256
samples) and the planner's obstacle scene, graph replay and warm start."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mppi_checks as mc  # noqa: E402
import mppi_oracle as mo  # noqa: E402
import parity_checks as pc  # noqa: E402


@pytest.fixture(scope="module")
def gpu_ops():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend("cuda:0"))
    assert ops.lib.device_count() >= 1, "no gfx950 device visible to libse3mpc"
    assert os.path.basename(ops.lib.path) == "libse3mpc.so"
    return ops


def harness(ops, dt):
    import torch
    return pc.Harness(ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"), lambda a: a.detach().cpu().numpy(), dt)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N,S,nprob", [(6, 64, 3), (30, 256, 4), (64, 128, 2)])
def test_noise_and_samples(gpu_ops, dt, N, S, nprob):
    mc.check_noise(harness(gpu_ops, dt), N, S, nprob)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N,S,nprob,iters,K", [(6, 64, 3, 3, 0), (6, 128, 2, 2, 3), (30, 256, 3, 3, 0), (30, 256, 2, 2, 16), (6, 640, 2, 2, 0),
                                               (50, 192, 2, 2, 5)])
def test_against_oracle(gpu_ops, dt, N, S, nprob, iters, K):
    mc.check_against_oracle(harness(gpu_ops, dt), N, S, nprob, iters, K=K)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N,S,K", [(6, 64, 0), (30, 256, 0), (30, 256, 4), (6, 1024, 0)])
def test_temperature_limits(gpu_ops, dt, N, S, K):
    mc.check_limits(harness(gpu_ops, dt), N, S, 3, iters=4, K=K)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N,S", [(6, 128), (30, 256), (30, 1024)])
def test_composed_iteration(gpu_ops, dt, N, S):
    mc.check_composition(harness(gpu_ops, dt), N, S)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("K", [0, 3])
def test_iteration_chunks_problem_slices_and_run_to_run(gpu_ops, dt, K):
    mc.check_chunking_and_slices(harness(gpu_ops, dt), 30, 320, 6, iters=3, K=K)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_invalid_arguments(gpu_ops, dt):
    mc.check_invalid_arguments(harness(gpu_ops, dt))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_full_size(gpu_ops, dt):
    """4096 problems x 256 samples x N = 30 x 8 iterations: finite, in the thrust box, identical on a second launch; lambda -> 0 keeps
    every problem's trace non-increasing."""
    import torch
    h = harness(gpu_ops, dt)
    prm, cfg, p0, v0, goal, U, sph = mc.problem(30, 4096, 21, K=16)
    run = mc.Run(h, prm, p0, v0, goal, U, sph, 1000.0)
    a = run(256, 8, 2.0, 100.0, seed=3)
    b = run(256, 8, 2.0, 100.0, seed=3)
    torch.cuda.synchronize()
    Ua, ca, ta, ka = run.host(a)
    Ub, cb, tb, kb = run.host(b)
    assert np.array_equal(Ua, Ub) and np.array_equal(ca, cb) and np.array_equal(ta, tb) and np.array_equal(ka, kb)
    lo, hi = mo.thrust_box(cfg)
    assert np.all(np.isfinite(Ua)) and np.all(np.isfinite(ca)) and np.all(np.isfinite(ta))
    assert np.all(Ua >= lo.astype(dt).astype(float)) and np.all(Ua <= hi.astype(dt).astype(float))
    assert np.all(ta[-1] <= ta[0]), "the best sample cost improves over 8 iterations"
    _, c0, t0, _ = run.host(run(256, 8, 2.0, 1e-300, seed=3))
    assert np.all(np.diff(t0, axis=0) <= 0), "lambda -> 0: non-increasing traces"


def _scene(gpu_ops):
    from dart_planner_amd.common.timing_alignment import TimingConfig, get_timing_manager, reset_timing_manager
    from dart_planner_amd.common.types import DroneState
    from dart_planner_amd.perception.explicit_geometric_mapper import ExplicitGeometricMapper
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    reset_timing_manager()
    get_timing_manager(TimingConfig(control_frequency=10.0))
    pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=30), device="cuda:0")
    assert abs(pl.se3_config.dt - 0.1) < 1e-12
    mapper = ExplicitGeometricMapper(resolution=0.5, max_range=20.0, ops=gpu_ops)
    mapper.add_obstacle(np.array([3.0, 0.0, 2.0]), 1.0)
    st = DroneState(timestamp=0.0, position=np.array([0.0, 0.0, 2.0]), velocity=np.zeros(3))
    spheres = mapper.local_obstacle_spheres(st.position, 20.0, 0.6, 20, 1.0)
    assert len(spheres) >= 1
    for c in spheres:
        pl.add_obstacle(c[:3], float(c[3]))
    return pl, mapper, st, np.array([8.0, 0.5, 2.0])


def test_mppi_plan_avoids_the_mappers_obstacle(gpu_ops):
    """The scene of test_shooting_plan_avoids_the_mappers_obstacle (10 Hz timing, N = 30, spheres from the device voxel map): the
    obstacle-blind MPPI plan is rejected by the mapper's is_trajectory_safe, the obstacle-aware one is accepted and ends within 2 m of
    the goal."""
    from dart_planner_amd.common.timing_alignment import reset_timing_manager
    try:
        pl, mapper, st, goal = _scene(gpu_ops)
        blind = pl.plan_mppi(st, goal, obstacles=False, warm_start=False)
        aware = pl.plan_mppi(st, goal, warm_start=False)
        res = dict(pl.last_result)
        safe_blind, _ = mapper.is_trajectory_safe(blind.positions, safety_margin=1.0)
        safe_aware, _ = mapper.is_trajectory_safe(aware.positions, safety_margin=1.0)
        end = np.linalg.norm(np.asarray(aware.positions)[-1] - goal)
        print(f"blind safe={safe_blind}, aware safe={safe_aware}, aware end {end:.2f} m from the goal, penalty {res['penalty']:.3g}, trace {res['trace']}")
        assert not safe_blind and safe_aware
        assert end < 2.0
    finally:
        reset_timing_manager()


def test_mppi_plan_graph_equals_eager_and_warm_starts(gpu_ops):
    """The captured plan (one hipGraph replay) equals the eager launches bit for bit, and a second warm-started call starts from exactly
    the shifted nominal."""
    from dart_planner_amd.common.timing_alignment import reset_timing_manager
    try:
        pl, mapper, st, goal = _scene(gpu_ops)
        for precision in ("f32", "f64"):
            pl._mppi_state = None
            pl.plan_mppi(st, goal, n_samples=512, iters=4, precision=precision, seed=2)
            r1 = dict(pl.last_result)
            U0, shift = pl._mppi_nominal(30, True)
            assert shift == 1 and np.array_equal(U0[:-1], r1["U"][1:]) and U0[-1].tolist() == [0.0, 0.0, pl.hover_thrust]
            ops, prm = pl._get_ops(), pl._params()
            args = (ops, prm, st.position.astype(float), st.velocity.astype(float), U0, 512, 4, pl.MPPI_SIGMA, pl.MPPI_TEMPERATURE, 2, precision,
                    pl._obstacle_table(None), pl.se3_config.obstacle_weight, pl._mppi_iter_base)
            eager, tr_e = pl._plan_mppi_eager(*args)
            pl.plan_mppi(st, goal, n_samples=512, iters=4, precision=precision, seed=2)
            r2 = dict(pl.last_result)
            assert r2["shift"] == 1 and r2["iter_base"] == r1["iter_base"] + 4
            N = 30
            assert np.array_equal(eager[6 * N:9 * N].reshape(N, 3), r2["U"]), "captured == eager (the nominal)"
            assert np.array_equal(eager[19 * N:], [r2["cost"], r2["penalty"], r2["cost_with_penalty"]]) and np.array_equal(tr_e, r2["trace"])
            captured, tr_c = pl._plan_mppi_captured(*args)
            assert np.array_equal(captured, eager) and np.array_equal(tr_c, tr_e), "graph replay == eager, bit for bit"
    finally:
        reset_timing_manager()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_plan_batch_mppi_rows(gpu_ops, precision):
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    import torch
    pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=20), device="cuda:0")
    rng = np.random.default_rng(3)
    B = 64
    pos, vel, goals = rng.uniform(-1, 1, (B, 3)) + [0, 0, 2], rng.uniform(-1, 1, (B, 3)), rng.uniform(-3, 3, (B, 3)) + [0, 0, 2]
    res = pl.plan_batch_mppi(pos, vel, goals, n_samples=256, iters=3, seed=5, precision=precision)
    ops, prm = pl._get_ops(), pl._params(has_goal=1)
    dt = torch.float32 if precision == "f32" else torch.float64
    col = lambda a: torch.tensor(np.asarray(a, float).reshape(-1, 1), dtype=dt, device="cuda:0")
    for b in (0, 17, 63):
        o = ops.mppi(prm, col(pos[b]), col(vel[b]), col(goals[b]), col(np.tile([0.0, 0.0, pl.hover_thrust], (20, 1))), 256, 3, pl.MPPI_SIGMA,
                     pl.MPPI_TEMPERATURE, seed=5, index_base=b)
        assert np.array_equal(o["U"].cpu().numpy()[:, 0].astype(float).reshape(20, 3), res["thrust_vectors"][b])
        assert float(o["cost"].cpu()[0]) == res["cost"][b]
    assert np.allclose(res["positions"][:, 0], pos, atol=1e-6)
