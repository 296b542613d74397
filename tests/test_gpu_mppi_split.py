"""GPU suite (`-m gpu`): the split-sample MPPI of dart_planner_amd/csrc/mppi_split.hip (one problem's samples over several workgroups, one
launch per iteration) on a real MI355X through the C ABI, Ops and the planner: the oracle, the unsplit kernel, run-to-run
identity at device size, the temperature limits, the argument rules, and the planner's graph replay, warm start, obstacle scene and batch."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mppi_checks as mc  # noqa: E402
import mppi_split_checks as sc  # noqa: E402
import parity_checks as pc  # noqa: E402

DTYPES = [np.float64, np.float32]
SHAPES = [(64, 1), (256, 4), (320, 5), (1024, 4), (1024, 16), (2048, 2)]          # (S, splits); the last has several chunks per split


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


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("N", [6, 30])
@pytest.mark.parametrize("S,splits", SHAPES)
def test_against_oracle(gpu_ops, dt, K, N, S, splits):
    sc.check_against_oracle(harness(gpu_ops, dt), N, S, splits, 3, (0, 1, 3), K=K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,S,K", [(6, 64, 0), (30, 256, 3), (30, 320, 0), (30, 1024, 16), (64, 2048, 0)])
def test_one_split_is_the_unsplit_kernel(gpu_ops, dt, N, S, K):
    sc.check_one_split_is_the_unsplit_kernel(harness(gpu_ops, dt), N, S, 3, iters=3, K=K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("S,splits", SHAPES[1:] + [(4096, 64)])
def test_one_iteration_any_split_against_the_unsplit_kernel(gpu_ops, dt, K, S, splits):
    sc.check_one_iteration_any_split(harness(gpu_ops, dt), 30, S, splits, 3, K=K)


@pytest.mark.parametrize("dt", DTYPES)
def test_run_to_run_identity_at_device_size(gpu_ops, dt):
    """S = 4096 x 16 splits x 8 iterations x 64 problems with 16 spheres (1024 workgroups per launch, every CU busy), launched three times:
    identical bytes, whatever order the workgroups ran in."""
    import torch
    h = harness(gpu_ops, dt)
    prm, cfg, p0, v0, goal, U, sph = mc.problem(30, 64, 21, K=16)
    run = sc.Run(h, prm, p0, v0, goal, U, sph, 1000.0)
    outs = []
    for _ in range(3):
        o = run(4096, 8, 2.0, 100.0, 16, seed=3)
        torch.cuda.synchronize()
        outs.append(run.host(o))
    for other in outs[1:]:
        for a, b, name in zip(outs[0], other, ("U", "cost", "trace", "keys")):
            assert a.tobytes() == b.tobytes(), f"{name} differs between launches"
    assert np.all(np.isfinite(outs[0][0])) and np.all(np.isfinite(outs[0][1])) and np.all(outs[0][2][-1] <= outs[0][2][0])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("S,splits,K", [(1280, 5, 0), (1024, 16, 3)])
def test_iteration_chunks_problem_slices_and_run_to_run(gpu_ops, dt, S, splits, K):
    sc.check_chunking_and_slices(harness(gpu_ops, dt), 30, S, splits, 6, iters=3, K=K)


@pytest.mark.parametrize("dt", DTYPES)
def test_temperature_limits(gpu_ops, dt):
    winners = []
    for N, S, splits in [(6, 256, 4), (30, 1024, 16), (30, 2048, 2), (6, 1024, 4)]:
        winners += sc.check_limits(harness(gpu_ops, dt), N, S, splits, 3, iters=4)
    sc.assert_winners_spread(winners)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("S,splits", [(1024, 4), (640, 2)])
def test_nan_costs_weigh_nothing(gpu_ops, dt, S, splits):
    sc.check_nan_costs_weigh_nothing(harness(gpu_ops, dt), 30, S, splits, iters=3)


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_arguments(gpu_ops, dt):
    sc.check_invalid_arguments(harness(gpu_ops, dt))


def _scene(gpu_ops):
    """The scene of tests/test_gpu_mppi.py: 10 Hz timing, N = 30, spheres from the device voxel map around one obstacle on the way."""
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


def test_split_plan_avoids_the_mappers_obstacle(gpu_ops):
    """The scene and the bounds of test_mppi_plan_avoids_the_mappers_obstacle: the split plan (the defaults, splits = 4 and "auto") is
    accepted by the mapper's is_trajectory_safe and ends within 2 m of the goal."""
    from dart_planner_amd.common.timing_alignment import reset_timing_manager
    try:
        pl, mapper, st, goal = _scene(gpu_ops)
        for splits in (4, "auto"):
            plan = pl.plan_mppi(st, goal, warm_start=False, splits=splits)
            res = dict(pl.last_result)
            safe, _ = mapper.is_trajectory_safe(plan.positions, safety_margin=1.0)
            end = np.linalg.norm(np.asarray(plan.positions)[-1] - goal)
            print(f"splits={splits} -> {res['splits']}: safe={safe}, end {end:.2f} m from the goal, penalty {res['penalty']:.3g}, trace {res['trace']}")
            assert res["splits"] == 4 and safe
            assert end < 2.0
    finally:
        reset_timing_manager()


def test_split_plan_graph_equals_eager_and_warm_starts(gpu_ops):
    """plan_mppi(splits=4): the captured plan (one hipGraph replay of the iters + 1 launches) equals the eager launches bit for bit, a
    second warm-started call starts from exactly the shifted nominal, and the iteration counter advances as on the unsplit path."""
    from dart_planner_amd.common.timing_alignment import reset_timing_manager
    try:
        pl, mapper, st, goal = _scene(gpu_ops)
        for precision in ("f32", "f64"):
            pl._mppi_state = None
            pl.plan_mppi(st, goal, n_samples=512, iters=4, precision=precision, seed=2, splits=4)
            r1 = dict(pl.last_result)
            U0, shift = pl._mppi_nominal(30, True)
            assert shift == 1 and np.array_equal(U0[:-1], r1["U"][1:]) and U0[-1].tolist() == [0.0, 0.0, pl.hover_thrust]
            ops, prm = pl._get_ops(), pl._params()
            args = (ops, prm, st.position.astype(float), st.velocity.astype(float), U0, 512, 4, pl.MPPI_SIGMA, pl.MPPI_TEMPERATURE, 2, precision,
                    pl._obstacle_table(None), pl.se3_config.obstacle_weight, pl._mppi_iter_base, 4)
            eager, tr_e = pl._plan_mppi_eager(*args)
            pl.plan_mppi(st, goal, n_samples=512, iters=4, precision=precision, seed=2, splits=4)
            r2 = dict(pl.last_result)
            assert r2["shift"] == 1 and r2["iter_base"] == r1["iter_base"] + 4 and r2["splits"] == 4
            N = 30
            assert np.array_equal(eager[6 * N:9 * N].reshape(N, 3), r2["U"]), "captured == eager (the nominal)"
            assert np.array_equal(eager[19 * N:], [r2["cost"], r2["penalty"], r2["cost_with_penalty"]]) and np.array_equal(tr_e, r2["trace"])
            captured, tr_c = pl._plan_mppi_captured(*args)
            assert np.array_equal(captured, eager) and np.array_equal(tr_c, tr_e), "graph replay == eager, bit for bit"
            assert sum(1 for k in pl._mppi_graphs if k[-1] == 4 and k[6] == precision) == 1, "one capture serves every cycle"
    finally:
        reset_timing_manager()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_split_plan_is_the_unsplit_plan(gpu_ops, precision):
    """plan_mppi(splits=1) == plan_mppi() bit for bit over a cold and two warm-started cycles (both through their captured graphs)."""
    from dart_planner_amd.common.timing_alignment import reset_timing_manager
    try:
        a, _, st, goal = _scene(gpu_ops)
        b, _, _, _ = _scene(gpu_ops)
        for cycle in range(3):
            ta = a.plan_mppi(st, goal, n_samples=1024, iters=4, precision=precision, seed=7)
            tb = b.plan_mppi(st, goal, n_samples=1024, iters=4, precision=precision, seed=7, splits=1)
            ra, rb = a.last_result, b.last_result
            assert np.array_equal(ra["U"], rb["U"]) and np.array_equal(ra["trace"], rb["trace"]), f"cycle {cycle}"
            assert (ra["cost"], ra["penalty"], ra["iter_base"], ra["shift"]) == (rb["cost"], rb["penalty"], rb["iter_base"], rb["shift"])
            assert np.array_equal(np.asarray(ta.positions), np.asarray(tb.positions))
    finally:
        reset_timing_manager()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_plan_batch_mppi_split_rows(gpu_ops, precision):
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    import torch
    pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=20), device="cuda:0")
    rng = np.random.default_rng(3)
    B = 64
    pos, vel, goals = rng.uniform(-1, 1, (B, 3)) + [0, 0, 2], rng.uniform(-1, 1, (B, 3)), rng.uniform(-3, 3, (B, 3)) + [0, 0, 2]
    res = pl.plan_batch_mppi(pos, vel, goals, n_samples=1024, iters=3, seed=5, precision=precision, splits="auto")
    ops, prm = pl._get_ops(), pl._params(has_goal=1)
    dt = torch.float32 if precision == "f32" else torch.float64
    col = lambda a: torch.tensor(np.asarray(a, float).reshape(-1, 1), dtype=dt, device="cuda:0")
    assert pl._mppi_splits("auto", 1024, B) == 4
    for b in (0, 17, 63):
        o = ops.mppi_split(prm, col(pos[b]), col(vel[b]), col(goals[b]), col(np.tile([0.0, 0.0, pl.hover_thrust], (20, 1))), 1024, 3, pl.MPPI_SIGMA,
                           pl.MPPI_TEMPERATURE, 4, seed=5, index_base=b)
        assert np.array_equal(o["U"].cpu().numpy()[:, 0].astype(float).reshape(20, 3), res["thrust_vectors"][b])
        assert float(o["cost"].cpu()[0]) == res["cost"][b]
        assert np.array_equal(o["trace"].cpu().numpy()[:, 0].astype(float), res["trace"][b])
    assert np.allclose(res["positions"][:, 0], pos, atol=1e-6)
