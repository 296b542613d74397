"""GPU: `bench.py --dump-outputs DIR` writes what the timed path computed in its last step.  A plain run with a step count that ends
in a partial launch (K mod 64 != 0) dumps cost, thrust gradient and fused argmin; the test regenerates that step's seeded inputs
(bench.make_ring, same seed, same ring) and checks the dump against the oracle's float64 rollout + cost + adjoint gradient."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    import torch
    from oracle import se3mpc_oracle as orc
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    K, out = 130, str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "3", "--dump-outputs", out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps_timed"] == K and res["ms_per_step"] > 0 and res["keys_valid"] and "cpu_baseline" not in res and "solve" not in res
    B, N, ring = res["config"]["batch_per_gpu"], res["config"]["horizon"], res["config"]["ring"]
    got = {n: np.load(os.path.join(out, n + ".npy")) for n in ("cost", "grad", "argmin_index", "argmin_cost")}
    assert sorted(res["dump_outputs"]) == sorted(got)
    assert got["cost"].dtype == np.float32 and got["cost"].shape == (B,) and got["grad"].shape == (3 * N, B)

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    p0, v0, goal, T, _, _ = bench.make_ring(torch, torch.device("cuda:0"), B, N, ring, seed=3)
    s = (K - 1) % ring
    lanes = lambda a: a[s].cpu().numpy().astype(np.float64).T          # (rows, B) -> (B, rows)
    cfg = orc.OracleConfig(prediction_horizon=N)
    c_ref, g_ref = orc.rollout_cost_grad(lanes(p0), lanes(v0), lanes(goal), lanes(T).reshape(B, N, 3), cfg)
    assert np.max(np.abs(got["cost"] - c_ref) / c_ref) <= 5e-6
    assert np.max(np.abs(got["grad"].T.reshape(B, N, 3) - g_ref)) <= 5e-6 * np.max(np.abs(g_ref))
    i = int(got["argmin_index"][0])
    assert i == int(np.argmin(got["cost"])) and got["argmin_cost"][0] == got["cost"][i]
