#!/usr/bin/env python3
"""bench.py -- SE(3) rollouts/s (horizon 30, batch 8192 per GPU) on N MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]``; for N > 1 it is
launched by ``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`` (one rank per GPU,
RCCL).  Rank 0 prints ONE JSON line.

A *step* is one pass of the hot path over one batch: the shooting-form rollout + running/terminal
cost + exact thrust gradient (SURVEY.md section 8d "canonical rollout", 4*(6N+10) B per rollout) of
``batch`` = 8192 synthetic trajectories resident in HBM, with the batch argmin folded into the same
kernel.  The batch is fixed per GPU (weak scaling); the only cross-GPU exchange is ONE bucketed
RCCL all-reduce(MIN) of the K packed (cost, index) keys at the end of the timed region
(SURVEY.md section 8e).  Steps cycle through a ring of distinct input/output batches larger than the
256 MiB Infinity Cache, so every step streams its operands from HBM.  The inputs come from a seeded
generator: the same arguments give the same inputs on every run.

A plain run is the headline alone: set-up, W warm-up steps, exactly K timed steps, the result line
(`value` = rollouts/s, `ms_per_step` = milliseconds per timed step).  The steps are independent batches
(a Monte-Carlo sweep, many planners), so `--steps-per-launch` S = 64 of them go into ONE multi-batch
kernel launch (grid.y); the K steps are floor(K / S) full launches plus one launch of the K mod S left
over, captured into hipGraphs and replayed inside the timed region.  Before the timed region the device
gets ~60 ms of untimed load of its own (`warm_device`): after the idle gap of a graph capture the card
needs 20-40 ms before a kernel's duration settles.  `--dump-outputs DIR` then writes what the last
timed step computed (cost, thrust gradient, fused argmin) as DIR/<name>.npy.

`--full` adds every other leg (SURVEY.md section 7 "report both"): the CPU baseline, the same K steps
as one launch per step (`single_launch`: sequentially dependent sampling iterations of one planner,
6 MB per launch = 1 us of HBM time, i.e. latency-bound), the p95 solve latency, the voxel map, the
BASELINE config-2 / config-3 legs, the on-device iteration loop and the closed-loop Monte-Carlo; each
`--no-<leg>` option drops one of them, `--sweep` adds saturating batch sizes.

`--gpus N` with N > 1 and no torchrun environment: bench.py starts
`python -m torch.distributed.run --nproc-per-node N bench.py ...` itself, as a child process and BEFORE
any HIP call, relays rank 0's JSON line and exits non-zero unless N ranks joined.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E peak 8.0 TB/s (6.29 TB/s measured copy)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20480, help="timed steps (exactly this many)")
    ap.add_argument("--warmup", type=int, default=200, help="untimed warm-up steps before them (rounded up to whole launches)")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beyond the headline (CPU baseline, single_launch, solve, voxel map, configs, iteration loop, closed loop)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32 / float64, <= 64 MiB)")
    ap.add_argument("--batch", type=int, default=8192, help="rollouts per GPU per step (BASELINE.json metric: 8192)")
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--ring", type=int, default=0, help="distinct batches cycled through (0 = enough to exceed 512 MiB)")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-solve", action="store_true", help="skip the p95 solve-latency leg")
    ap.add_argument("--no-obstacle-source", action="store_true", help="skip the voxel-map leg (mapper -> planner obstacles)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--steps-per-launch", type=int, default=64,
                    help="independent 8192-rollout steps issued as ONE multi-batch kernel launch (1 = one launch per step)")
    ap.add_argument("--no-single", action="store_true", help="skip the one-launch-per-step leg")
    ap.add_argument("--variant", type=int, default=0, help="se3mpc_set_rollout_variant (0 = auto)")
    ap.add_argument("--sweep", action="store_true", help="with --full: also time saturating batch sizes (extra keys)")
    ap.add_argument("--min-ms", type=float, default=20.0, help="--full legs: each timed pass is repeated until it lasts this long")
    ap.add_argument("--dry-run", action="store_true",
                    help="rank plumbing only, no HIP: spawn / rendezvous (gloo) / key all-reduce / JSON line with value null "
                         "(what the CPU test-suite runs to check that --gpus N really starts N ranks)")
    ap.add_argument("--no-configs", action="store_true", help="skip the BASELINE config-2 / config-3 legs")
    ap.add_argument("--no-iterated", action="store_true", help="skip the on-device K-iteration leg")
    ap.add_argument("--no-closed-loop", action="store_true", help="skip the closed-loop Monte-Carlo leg")
    ap.add_argument("--iterated-ks", default="0,1,4,16,64", help="iteration counts of the on-device iteration leg (profiling: one value)")
    ap.add_argument("--no-primary", action="store_true", help="profiling only, with --full: skip the rollout legs (no JSON line is printed)")
    a = ap.parse_args()
    if (a.no_primary or a.sweep) and not a.full:
        ap.error("--no-primary and --sweep select --full legs: add --full")
    if a.no_primary and a.dump_outputs:
        ap.error("--dump-outputs writes the timed rollout steps' outputs: it cannot go with --no-primary")
    if a.steps < 1:
        ap.error("--steps must be >= 1")
    return a


def make_ring(torch, dev, B, N, ring, seed):
    """cfg-2 distribution of SURVEY.md section 8d: p0 ~ U(-20,20)^3, v0 ~ U(-5,5)^3, goal ~ U(-20,20)^3,
    T = (0,0,14.715) + N(0, 2^2) clipped to the thrust box (planner.py:390-400)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    p0 = torch.rand(ring, 3, B, device=dev, generator=g) * 40 - 20
    v0 = torch.rand(ring, 3, B, device=dev, generator=g) * 10 - 5
    goal = torch.rand(ring, 3, B, device=dev, generator=g) * 40 - 20
    T = torch.randn(ring, 3 * N, B, device=dev, generator=g) * 2
    T[:, 2::3] += 14.715
    txy = 25.0 * math.sin(math.pi / 4)
    T[:, 0::3].clamp_(-txy, txy); T[:, 1::3].clamp_(-txy, txy); T[:, 2::3].clamp_(2.0, 25.0)
    cost = torch.empty(ring, B, device=dev)
    grad = torch.empty(ring, 3 * N, B, device=dev)
    return p0, v0, goal, T, cost, grad


def _cpu_worker(args):
    """One host core: the oracle's batched NumPy rollout+cost+grad in a loop for `seconds`."""
    B, N, seconds, seed = args
    import time as _t
    import numpy as _np
    from oracle import se3mpc_oracle as orc
    cfg = orc.OracleConfig(prediction_horizon=N)
    rng = _np.random.default_rng(seed)
    p0, v0, goal = rng.uniform(-20, 20, (B, 3)), rng.uniform(-5, 5, (B, 3)), rng.uniform(-20, 20, (B, 3))
    T = rng.normal(0, 2, (B, N, 3)) + [0, 0, cfg.hover_thrust]
    orc.rollout_cost_grad(p0, v0, goal, T, cfg)
    n, t0 = 0, _t.perf_counter()
    while _t.perf_counter() - t0 < seconds:
        orc.rollout_cost_grad(p0, v0, goal, T, cfg)
        n += 1
    return n, _t.perf_counter() - t0


def cpu_baseline(B, N, seconds):
    """The oracle's batched NumPy restatement of the same rollout+cost+gradient (float64) on the host cores of
    this box: one worker process per core of the box's CPU share (16 for a one-GPU box), each looping over its
    own 8192-trajectory batch; plus the reference-shaped leg (one problem per call, Python loops as in
    planner.py:516-580) on one core.  MUST run before this process touches the GPU: the workers are spawned."""
    import concurrent.futures as cf
    import multiprocessing as mp
    from oracle import se3mpc_oracle as orc
    Bs = min(B, 8192)
    cores = max(1, min(16, os.cpu_count() or 1))
    single = _cpu_worker((Bs, N, min(3.0, seconds / 4), 1))
    try:
        with cf.ProcessPoolExecutor(max_workers=cores, mp_context=mp.get_context("spawn")) as ex:
            res = list(ex.map(_cpu_worker, [(Bs, N, seconds, 10 + i) for i in range(cores)]))
    except Exception as e:                       # a box that forbids worker processes: report the single-core figure
        res, cores = [single], 1
        print(f"[bench] cpu_baseline: worker pool unavailable ({e!r}); single core only", file=sys.stderr)
    total = sum(n * Bs / el for n, el in res)
    cfg = orc.OracleConfig(prediction_horizon=N)
    rng = np.random.default_rng(1)
    p0, v0, goal = rng.uniform(-20, 20, 3), rng.uniform(-5, 5, 3), rng.uniform(-20, 20, 3)
    x = orc.straight_line_init(p0, v0, goal, cfg)
    m, t1 = 0, time.perf_counter()
    while time.perf_counter() - t1 < min(3.0, seconds / 3):
        orc.objective_loops(x, goal, cfg); orc.gradient_loops(x, goal, cfg)
        m += 1
    el1 = time.perf_counter() - t1
    # the reference-shaped SOLVE (plan_trajectory's arithmetic: per-step Python loops in f and g, SciPy L-BFGS-B), one
    # problem per call, one core: what the p95 solve latency of the `solve` leg stands beside (~5 ms at N=30)
    ts = []
    for i in range(40):
        gi = rng.uniform(-5, 5, 3); gi[2] = abs(gi[2]) + 0.5
        t2 = time.perf_counter()
        orc.plan_reference_shaped(np.array([0.0, 0.0, 1.0]), np.zeros(3), gi, cfg)
        ts.append((time.perf_counter() - t2) * 1e3)
    # the closed-loop Monte-Carlo of the `closed_loop` leg, reference-shaped on one core: per run and planning cycle one SciPy solve and 15
    # NumPy controller + simulator steps (oracle/controller_oracle.py), a bounded sample of 8 runs x 33 cycles
    from oracle import controller_oracle as co
    ccfg, csim, pcfg = co.ControllerConfig(), co.SimulatorConfig(), orc.OracleConfig()
    t3 = time.perf_counter()
    runs = 8
    for r_ in range(runs):
        pos, vel = np.array([[0.0, 0.0, 2.0]]) + 0.2 * rng.normal(size=(1, 3)), 0.3 * rng.normal(size=(1, 3))
        att, om, tt = np.zeros((1, 3)), np.zeros((1, 3)), np.zeros(1)
        cst = co.ControllerState(1, ccfg)
        for c_ in range(33):
            x, _ = orc.solve(pos[0], vel[0], np.array([8.0, 0.0, 5.0]), pcfg)
            ex = orc.extract_solution(x, pcfg)
            fin, _ = co.closed_loop(ccfg, csim, cst, pos, vel, att, om, tt, c_ * 0.15 + np.arange(6) / 400.0, x[:18].reshape(6, 3), x[18:36].reshape(6, 3),
                                    ex["accelerations"], 15, 0.01, wind=[0.5, 0.0, 0.0], stop_at_plan_end=False, log=False)
            pos, vel, att, om, tt = fin["pos"], fin["vel"], fin["att"], fin["omega"], fin["t"]
    loop_s = (time.perf_counter() - t3) / runs
    return dict(value=total, unit="rollouts/s", cores=cores, kind="port",
                closed_loop_reference_shaped=dict(what="one closed-loop run = 33 x (SciPy solve + 15 NumPy controller + simulator steps), one core",
                                                  runs=runs, seconds_per_run=loop_s, runs_per_s=1.0 / loop_s),
                sample=f"{cores} worker processes x {seconds:.0f} s of the oracle's batched NumPy rollout+cost+grad (float64), "
                       f"{Bs} trajectories per pass, horizon {N} ({sum(n for n, _ in res)} passes in all)",
                single_core_value=single[0] * Bs / single[1], reference_shaped_evals_per_s=m / el1,
                reference_shaped_solve_ms=dict(horizon=N, calls=len(ts), p50=float(np.percentile(ts, 50)), p95=float(np.percentile(ts, 95))),
                host_cpus=os.cpu_count())


def timed_region(torch, dist, world, dev, runs, keys, allreduce_min_keys):
    """The contract's timed region: barrier + synchronize, the K steps (`runs`: (graph replay or eager launches,
    count) pairs), [one bucketed all-reduce(MIN) of the step keys], synchronize + barrier; MAX over ranks.  Returns
    (elapsed_s, device_ms between the HIP events that bracket the launches on the launch stream)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for fn, count in runs:
        for _ in range(count):
            fn()
    e1.record()
    if world > 1:
        allreduce_min_keys(keys)     # the single exchange: ONE bucketed all-reduce(MIN) of the packed step keys
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    el = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    return float(el.item()), e0.elapsed_time(e1)


def capture(torch, dev, fn):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        # thread_local: with N > 1 ranks RCCL's watchdog thread issues event queries of its own; under the default (global)
        # capture mode any such call from another thread would invalidate the capture
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph.replay()                                              # one untimed replay (uploads the graph)
    torch.cuda.synchronize()
    return graph


def device_ms(torch, fn, reps):
    """Mean device time of fn() over `reps` back-to-back calls (HIP events on the launch stream)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


WARM_MS = 60.0


def warm_device(torch, fn, ms=WARM_MS, chunk=4):
    """Untimed: fn() back to back until ~`ms` of wall time has passed.  After an idle gap (graph capture, buffer set-up between two legs)
    the card needs 20-40 ms of load before a kernel's duration settles (profiles/r03f_warmup_series.txt: the 64-batch config-3 launch
    193 -> 160 us, the 64-batch rollout 65.8 -> 62.7 us, the 8192-problem solve 87.5 -> 82.8 us over the first 40 ms); every device-time
    leg is preceded by this so that it reports the steady state, not the ramp."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(chunk):
            fn()
        torch.cuda.synchronize()


MAX_GRAPH_NODES = 2048


def timed_plan(K, per_launch, ring):
    """How the K timed steps are laid out.  Step i runs on ring slot i mod `ring` (a multiple of per_launch), in
    launches of per_launch consecutive steps.  When K reaches `chunk_steps` (whole ring cycles, at most
    MAX_GRAPH_NODES full launches), one chunk is captured into a hipGraph and replayed `chunk_replays` times; the
    `tail_steps` left over (fewer than a chunk) are one more graph of full launches plus, if K mod per_launch != 0,
    one launch of that remainder.  chunk_replays x chunk_steps + tail_steps == K, always."""
    cap = max(ring, MAX_GRAPH_NODES * per_launch // ring * ring)
    chunk = cap if K >= cap else 0
    replays = K // chunk if chunk else 0
    tail = K - replays * chunk
    return dict(chunk_steps=chunk, chunk_replays=replays, tail_steps=tail,
                launches=replays * (chunk // per_launch) + math.ceil(tail / per_launch))


DUMP_LIMIT = 64 * 2 ** 20


def dump_outputs(ops, out_dir, cost, grad, key):
    """What the last timed step computed, as a caller of the rollout path receives it: `cost` float32 (B,),
    `grad` float32 (3N, B) (the thrust gradient in the kernel's lane layout), the fused batch argmin as
    `argmin_index` / `argmin_cost` float64 (1,).  Above DUMP_LIMIT bytes a fixed, seeded sample of the B
    rollouts is written instead, with its indices (`sample_index`).  -> {name: shape}"""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    idx, kc = ops.decode_key(key)
    out = {}
    B = cost.shape[0]
    if 4 * B * (1 + grad.shape[0]) > DUMP_LIMIT - 4096:
        m = (DUMP_LIMIT - 4096) // (4 * (1 + grad.shape[0]) + 8)
        pick = np.sort(np.random.default_rng(0).choice(B, m, replace=False))
        sel = torch.from_numpy(pick).to(cost.device)
        cost, grad = cost[sel], grad[:, sel]
        out["sample_index"] = pick.astype(np.float64)
    out.update(cost=cost.float().cpu().numpy(), grad=grad.float().cpu().numpy(),
               argmin_index=np.array([idx], np.float64), argmin_cost=np.array([kc], np.float64))
    for name, v in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), v)
    return {name: list(v.shape) for name, v in out.items()}


def spawn_ranks(a):
    """`--gpus N` without a torchrun environment: start N ranks as a CHILD process (never exec: this process may
    not touch the GPU before, and does not), relay the JSON line, fail loudly when fewer than N ranks joined."""
    import socket
    import subprocess
    import torch
    backend = "gloo" if a.dry_run else os.environ.get("SE3MPC_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()                  # counting devices does not initialise HIP
    if backend == "nccl" and ndev < a.gpus:
        print(f"[bench] --gpus {a.gpus} but only {ndev} GPU(s) are visible: refusing to report a {a.gpus}-GPU line",
              file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # the host driver only supports dmabuf IPC (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if proc.returncode != 0 or line is None:
        print(f"[bench] the {a.gpus}-rank child failed (rc={proc.returncode})", file=sys.stderr)
        return proc.returncode or 1
    got = json.loads(line)
    if got.get("n_gpus") != a.gpus or got.get("ranks_joined") != a.gpus:
        print(f"[bench] asked for {a.gpus} ranks, the line reports n_gpus={got.get('n_gpus')} ranks_joined={got.get('ranks_joined')}",
              file=sys.stderr)
        return 3
    print(line, flush=True)
    return 0


def dry_run(a, rank, world):
    """Everything around the kernels, without HIP: the ranks rendezvous over gloo, count themselves, all-reduce(MIN) one
    synthetic packed key per step exactly as the timed region does, and rank 0 prints a line with value = null."""
    import torch
    import torch.distributed as dist
    from dart_planner_amd.distributed import allreduce_min_keys, init_distributed
    init_distributed("gloo")
    joined = 1
    if world > 1:
        one = torch.ones(1, dtype=torch.int64)
        dist.all_reduce(one)
        joined = int(one.item())
    B, K = a.batch, max(1, a.steps)
    # rank r "finds" cost r + 1 at its first trajectory: the all-reduced key must name rank 0's trajectory 0
    keys = torch.full((K,), ((rank + 1) << 32) | (rank * B), dtype=torch.int64)
    allreduce_min_keys(keys)
    ok = bool((keys == ((1 << 32) | 0)).all())
    if rank == 0:
        print(json.dumps({"metric": "SE(3) rollouts/sec (N=30, batch=8192) + p95 solve ms, at 1/2/4/8 MI355X", "value": None,
                          "unit": "rollouts/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "dry_run": True,
                          "ranks_joined": joined, "dist_backend": "gloo" if world > 1 else None, "keys_valid": ok}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(a))
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"[bench] --gpus {a.gpus} but WORLD_SIZE={world}: the two must agree")
    if a.dry_run:
        return dry_run(a, rank, world)
    cpu_stats = None
    if rank == 0 and a.full and not a.no_cpu_baseline:
        # rank 0 only, also when several ranks run (the other ranks wait for it at the rendezvous, outside every timed region);
        # before any HIP call: it spawns worker processes
        cpu_stats = cpu_baseline(a.batch, a.horizon, a.cpu_seconds)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
    ndev = torch.cuda.device_count()
    local = local % max(ndev, 1)          # rehearsal of N ranks on a 1-GPU box (SE3MPC_DIST_BACKEND=gloo) shares the card
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    from dart_planner_amd.distributed import allreduce_min_keys, init_distributed
    backend = os.environ.get("SE3MPC_DIST_BACKEND", "nccl")
    init_distributed(backend, device=dev)
    joined = 1
    if world > 1:
        one = torch.ones(1, dtype=torch.int64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(one)
        joined = int(one.item())

    from dart_planner_amd.capi import Params
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend(dev))
    ops.lib.set_rollout_variant(a.variant)
    B, N, K, W, S = a.batch, a.horizon, a.steps, a.warmup, max(1, a.steps_per_launch)
    prm = Params.reference_defaults(horizon=N)
    bytes_per_rollout = 4 * (6 * N + 10)
    slot_bytes = 4 * B * ((9 + 3 * N) + (1 + 3 * N))
    ring = a.ring if a.ring > 0 else max(2, math.ceil(512 * 2 ** 20 / slot_bytes))
    ring = S * max(2, math.ceil(ring / S))                     # whole launches, consecutive launches on disjoint slots
    p0, v0, goal, T, cost, grad = make_ring(torch, dev, B, N, ring, seed=3 + rank)
    per = (B + 63) // 64                                        # wave-key slots per batch
    base = rank * B
    state = {}

    def launch(i0, n):
        """steps i0 .. i0+n-1 (n <= S consecutive ring slots) as ONE launch; step i's wavefronts write
        their partial argmin keys to wave_keys[i]"""
        s0 = i0 % ring
        wk = state["wave_keys"]
        if n == 1:
            ops.rollout_cost_grad(prm, p0[s0], v0[s0], goal[s0], T[s0], out=(cost[s0], grad[s0]), wave_keys=wk[i0], index_base=base)
        else:
            ops.rollout_cost_grad_batched(prm, p0[s0:s0 + n], v0[s0:s0 + n], goal[s0:s0 + n], T[s0:s0 + n], cost[s0:s0 + n],
                                          grad[s0:s0 + n], wave_keys=wk[i0:i0 + n], index_base=base)

    def run_steps(nsteps, per_launch, fold=True):
        """steps 0 .. nsteps-1 (step i on ring slot i mod ring, wave keys in row i) as launches of per_launch
        consecutive steps, the last one carrying the nsteps mod per_launch left over"""
        assert ring % per_launch == 0 and nsteps <= state["wave_keys"].shape[0]
        for i in range(0, nsteps, per_launch):
            launch(i, min(per_launch, nsteps - i))
        if fold:                                                # one bucketed fold of all steps' wave keys -> keys[step]
            ops.reduce_keys(state["wave_keys"][:nsteps], state["keys"][:nsteps])

    results, dumped = {}, None
    for mode, per_l in (("primary", S), ("single_launch", 1)):
        if a.no_primary or (mode == "single_launch" and (not a.full or S == 1 or a.no_single)):
            continue
        plan = timed_plan(K, per_l, ring)
        rows = plan["chunk_steps"] or plan["tail_steps"]         # steps of the longest graph = wave-key rows
        state["wave_keys"] = torch.zeros(rows, per, dtype=torch.int64, device=dev)
        state["keys"] = keys = torch.full((rows,), -1, dtype=torch.int64, device=dev)
        for _ in range(math.ceil(max(W, 1) / rows)):            # untimed warm-up: at least W steps, `rows` at a time
            run_steps(rows, per_l, fold=False)
        torch.cuda.synchronize()
        runs = []
        if plan["chunk_replays"]:
            runs.append((lambda: run_steps(plan["chunk_steps"], per_l), plan["chunk_replays"]))
        if plan["tail_steps"]:
            runs.append((lambda: run_steps(plan["tail_steps"], per_l), 1))
        if not a.no_graph:
            runs = [(capture(torch, dev, fn).replay, n) for fn, n in runs]
        if world > 1:
            # untimed: the first collective of a given shape pays communicator / kernel set-up (ms); the timed
            # region must only see the steady-state exchange
            allreduce_min_keys(keys.clone())
            dist.all_reduce(torch.zeros(1, dtype=torch.float64, device=dev), op=dist.ReduceOp.MAX)
        warm_device(torch, runs[0][0], chunk=1)                 # untimed, beyond the W warm-up steps: steady-state clocks
        keys.fill_(-1)
        torch.cuda.synchronize()
        elapsed, dev_ms = timed_region(torch, dist, world, dev, runs, keys, allreduce_min_keys)
        kh = keys.cpu().numpy().view(np.uint64)
        results[mode] = dict(elapsed=elapsed, launch_ms=dev_ms / plan["launches"], nlaunch=plan["launches"], per=per_l, graph=not a.no_graph,
                             plan=plan, device_ms=dev_ms, keys_valid=bool(np.all((kh & np.uint64(0xFFFFFFFF)) < np.uint64(world * B))))
        if mode == "primary" and a.dump_outputs and rank == 0:  # before any other leg reuses the ring
            dumped = dump_outputs(ops, a.dump_outputs, cost[(K - 1) % ring], grad[(K - 1) % ring], keys[(K - 1) % rows:(K - 1) % rows + 1])
        del runs
    state.pop("wave_keys", None); state.pop("keys", None)

    solve_stats = None if (not a.full or a.no_solve) else solve_leg(torch, ops, dev, B, N, rank, world)
    voxel_stats = None if (not a.full or a.no_obstacle_source or rank != 0) else obstacle_source_leg(torch, ops, dev)
    del p0, v0, goal, T, cost, grad
    torch.cuda.empty_cache()
    config_stats = None if (not a.full or a.no_configs or rank != 0) else config_legs(torch, ops, dev, a.min_ms)
    iter_stats = None if (not a.full or a.no_iterated or rank != 0) else iterated_leg(torch, ops, dev, B, N, a.min_ms, tuple(int(k) for k in a.iterated_ks.split(",")))
    loop_stats = None if (not a.full or a.no_closed_loop or rank != 0) else closed_loop_leg(torch, ops, dev)

    if rank == 0 and a.no_primary:
        print(json.dumps({"profiling_only": True, "iterated": iter_stats, "configs": config_stats, "closed_loop": loop_stats, "solve": solve_stats}), flush=True)
    elif rank == 0:
        r = results["primary"]
        per_launch_rollouts = B * S
        achieved = bytes_per_rollout * B * K / (r["device_ms"] * 1e-3) / 1e9
        traffic = profiled_traffic(B, N)
        value = world * B * K / r["elapsed"]
        res = {
            "metric": "SE(3) rollouts/sec (N=30, batch=8192) + p95 solve ms, at 1/2/4/8 MI355X",
            "value": value, "unit": "rollouts/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": r["elapsed"] / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "steps_timed": K, "plan": r["plan"], "timed_region_s": r["elapsed"], "full": a.full,
            "ranks_joined": joined, "dist_backend": (backend if world > 1 else None),
            "config": {"workload": f"horizon={N} SE(3) rollout + cost + thrust-gradient (+ fused batch argmin), "
                                   f"batch={B} per GPU per step, {S} independent steps per kernel launch "
                                   f"({'one multi-batch launch = grid.y' if S > 1 else 'one launch per step'}), "
                                   f"ring of {ring} distinct batches in HBM ({ring * slot_bytes / 2 ** 20:.0f} MiB), "
                                   f"{'hipGraph replay' if r['graph'] else 'eager launches'}; the {K} timed steps = {K // S} full launches"
                                   f"{f' + one launch of {K % S}' if K % S else ''}",
                       "horizon": N, "batch_per_gpu": B, "global_batch": world * B, "steps_per_launch": S, "ring": ring,
                       "parallelism": f"batch-sharded x{world}, one bucketed all-reduce(MIN) of the step keys"},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS,
                         "traffic": None if traffic is None else traffic[0] * per_launch_rollouts,
                         "traffic_over_algorithmic": None if traffic is None else traffic[0] / bytes_per_rollout,
                         "traffic_source": None if traffic is None else f"profiles/{traffic[1]} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes; "
                                                                          f"HBM bytes per rollout of this kernel at this launch shape x rollouts per launch)",
                         "kernel": "se3mpc::rollout_kernel<float, 30, REG, SPLIT, GRAD>", "kernel_us": r["launch_ms"] * 1e3,
                         "launches": r["nlaunch"], "rollouts_per_launch": per_launch_rollouts,
                         "bytes_per_launch": bytes_per_rollout * per_launch_rollouts,
                         "note": "achieved = algorithmic bytes (4*(6N+10) B/rollout x rollouts of the timed steps) / device time "
                                 "(HIP events around the launches of the timed region on the launch stream)"},
            "keys_valid": r["keys_valid"],
        }
        if "single_launch" in results:
            q = results["single_launch"]
            g1 = bytes_per_rollout * B / (q["launch_ms"] * 1e-3) / 1e9
            res["single_launch"] = {"what": "ONE kernel launch per 8192-rollout step (sequentially dependent iterations), the same K steps",
                                    "value": world * B * K / q["elapsed"], "ms_per_step": q["elapsed"] / K * 1e3,
                                    "steps_timed": K, "plan": q["plan"],
                                    "kernel_us": q["launch_ms"] * 1e3, "achieved_GB_per_s": g1, "frac": g1 / HBM_PEAK_GBPS,
                                    "keys_valid": q["keys_valid"]}
        if iter_stats is not None:
            res["iterated"] = iter_stats
        if config_stats is not None:
            res["configs"] = config_stats
        if loop_stats is not None:
            res["closed_loop"] = loop_stats
        if solve_stats is not None:
            res["solve"] = solve_stats
        if voxel_stats is not None:
            res["obstacle_source"] = voxel_stats
        if a.full and a.sweep:
            res["sweep"] = sweep(torch, ops, prm, dev, N)
        if dumped is not None:
            res["dump_outputs"] = dumped
        if cpu_stats is not None:
            res["cpu_baseline"] = cpu_stats
            res["vs_cpu_baseline"] = value / cpu_stats["value"]
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def solve_leg(torch, ops, dev, B, N, rank, world):
    """p95 of the per-call wall time (np.percentile convention of the reference's
    tests/test_real_time_latency.py:296-304; >= 200 timed calls after >= 20 warm-ups, device
    synchronised inside the timed region) of (a) ONE hover->waypoint solve through the planner mirror
    (`plan_trajectory`, what the contract test times) and (b) the batched solve of `B` problems in one
    launch.  Every rank runs its own shard; rank 0 reports."""
    import torch.distributed as dist
    from dart_planner_amd.capi import Params
    from dart_planner_amd.common.types import DroneState
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCConfig, SE3MPCPlanner
    out = {}
    for prec in ("f64", "f32"):
        pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=N), precision=prec, device=dev)
        st = DroneState(timestamp=0.0, position=np.array([0.0, 0.0, 1.0]), velocity=np.zeros(3))
        rng = np.random.default_rng(0)
        goals = rng.uniform(-5, 5, (240, 3)); goals[:, 2] = np.abs(goals[:, 2]) + 0.5
        # plan_trajectory returns host arrays: when it returns, the device work behind them is complete (its launch-and-wait call came back on
        # the kernel's completion ticket) -- that is the timed call, as the reference's contract test times it.  The same call followed by a
        # device-wide synchronise (what rounds 1-2 timed) is reported beside it.
        ts, ts_sync = [], []
        for i, g in enumerate(goals):
            t0 = time.perf_counter()
            pl.plan_trajectory(st, g)
            t1 = time.perf_counter()
            if i >= 20:
                ts.append((t1 - t0) * 1e3)
        for i, g in enumerate(goals):
            t0 = time.perf_counter()
            pl.plan_trajectory(st, g)
            torch.cuda.synchronize()
            if i >= 20:
                ts_sync.append((time.perf_counter() - t0) * 1e3)
        out[f"single_{prec}"] = {"horizon": N, "calls": len(ts), "p50_ms": float(np.percentile(ts, 50)),
                                 "p95_ms": float(np.percentile(ts, 95)), "max_ms": float(np.max(ts)),
                                 "p50_ms_with_device_synchronize": float(np.percentile(ts_sync, 50)),
                                 "p95_ms_with_device_synchronize": float(np.percentile(ts_sync, 95))}
    # the drop-in boundary itself: se3mpc_plan_host_* (launch on pinned buffers + completion ticket) called through ctypes with pre-computed addresses --
    # what a C / C++ caller of the library pays per plan; the Python mirror's share is the difference to single_* above
    import ctypes
    for prec, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        prm1 = Params.reference_defaults(horizon=N)
        esz = 4 if prec == "f32" else 8
        h_in = torch.zeros((3, 1, 3), dtype=tdt, pin_memory=True); h_in[0, 0, 2] = 1.0
        h_out = torch.empty((ops.packed_size(1, N, prec),), dtype=torch.uint8, pin_memory=True)
        h_done = torch.zeros((8,), dtype=torch.int64, pin_memory=True)
        o_x, o_acc, o_att, o_rates, o_thr, o_info, _ = ops._packed_offsets(1, N, esz)
        pin, base = h_in.data_ptr(), h_out.data_ptr()
        fn = getattr(ops.lib._dll, f"se3mpc_plan_host_{prec}")
        stream = torch.cuda.current_stream(dev).cuda_stream
        hin_np = h_in.numpy()
        ts = []
        for i, g in enumerate(goals):
            hin_np[2, 0] = g
            t0 = time.perf_counter()
            rc = fn(ctypes.byref(prm1), 1, pin, pin + 3 * esz, pin + 6 * esz, 0, base + o_x, base + o_info, base + o_acc, base + o_att, base + o_rates,
                    base + o_thr, h_done.data_ptr(), i + 1, 2000.0, stream)
            if i >= 20:
                ts.append((time.perf_counter() - t0) * 1e3)
            if rc != 0:
                raise RuntimeError(f"se3mpc_plan_host_{prec}: status {rc}")
        out[f"single_{prec}"].update(c_abi_call_p50_ms=float(np.percentile(ts, 50)), c_abi_call_p95_ms=float(np.percentile(ts, 95)))
    # the shooting-form plan through the same mirror: 8192 thrust samples x 16 iterations in one launch, argmin, rollout + extraction of the winner
    if world == 1:
        pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=N), precision="f64", device=dev)
        ts = []
        for i, g in enumerate(goals[:120]):
            t0 = time.perf_counter()
            pl.plan_shooting(st, g, n_samples=B, iters=16, seed=0)      # one resident sample set (a new seed is a new set and a new graph capture)
            torch.cuda.synchronize()
            if i >= 20:
                ts.append((time.perf_counter() - t0) * 1e3)
        out["shooting_plan_f32"] = {"horizon": N, "samples": B, "iterations": 16, "calls": len(ts), "p50_ms": float(np.percentile(ts, 50)),
                                    "p95_ms": float(np.percentile(ts, 95)), "rollouts_per_plan": B * 17}
        # the same plan around 16 spheres (the obstacle-aware loop, se3mpc_rollout_iterate_obstacles_*): dt = 0.1 s so that the horizon covers metres
        pl = SE3MPCPlanner(SE3MPCConfig(prediction_horizon=N, dt=0.1), precision="f64", device=dev)
        rng_o = np.random.default_rng(3)
        for c in np.round(rng_o.uniform(-2.0, 12.0, (16, 3)) * 2) / 2:
            pl.add_obstacle(c + np.array([0.0, 0.0, 3.0]), 1.0)
        ts = []
        for i, g in enumerate(goals[:120]):
            t0 = time.perf_counter()
            pl.plan_shooting(st, g, n_samples=B, iters=16, seed=0, step=2e-3)
            torch.cuda.synchronize()
            if i >= 20:
                ts.append((time.perf_counter() - t0) * 1e3)
        out["shooting_plan_obstacles_f32"] = {"horizon": N, "samples": B, "iterations": 16, "spheres": 16, "dt": 0.1, "calls": len(ts),
                                              "p50_ms": float(np.percentile(ts, 50)), "p95_ms": float(np.percentile(ts, 95)),
                                              "penalty_left": float(pl.last_result.get("penalty", float("nan")))}
    prm = Params.reference_defaults(horizon=N)
    g = torch.Generator(device=dev); g.manual_seed(100 + rank)
    p0 = torch.rand(B, 3, device=dev, generator=g) * 40 - 20
    v0 = torch.rand(B, 3, device=dev, generator=g) * 10 - 5
    goal = torch.rand(B, 3, device=dev, generator=g) * 40 - 20
    ts = []
    nfev = None
    o = None
    for i in range(220):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = ops.solve(prm, p0, v0, goal, out=o)             # steady state: the previous call's output tensors are written again
        torch.cuda.synchronize()
        if i >= 20:
            ts.append((time.perf_counter() - t0) * 1e3)
    # the same call between two HIP events on its stream (both launches of the two-tier solve, without the host's share of the wall time);
    # horizon 6 -- the reference's default -- beside the named horizon
    def device_us(prm_, reps=100):
        oo = None
        for _ in range(10):
            oo = ops.solve(prm_, p0, v0, goal, out=oo)
        warm_device(torch, lambda: ops.solve(prm_, p0, v0, goal, out=oo), chunk=8)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            oo = ops.solve(prm_, p0, v0, goal, out=oo)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    dev_us, dev_us_h6 = device_us(prm), device_us(Params.reference_defaults(horizon=6))
    info = ops.info_to_host(o["info"])
    mean_ms = float(np.mean(ts))
    agg = torch.tensor([B / (mean_ms * 1e-3)], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(agg)
    out["batch_f32"] = {"horizon": N, "batch_per_gpu": B, "calls": len(ts), "p50_ms": float(np.percentile(ts, 50)),
                        "p95_ms": float(np.percentile(ts, 95)), "solves_per_s": float(agg.item()),
                        "mean_nfev": float(info["nfev"].mean()), "mean_nit": float(info["nit"].mean()),
                        "device_us_per_batch_hip_events": dev_us, "device_us_per_batch_horizon_6": dev_us_h6,
                        "rollouts_inside_solves_per_s": float(agg.item() * info["nfev"].mean())}
    return out


def obstacle_source_leg(torch, ops, dev):
    """The caller side of the path at the sizes of the reference's planning cycle
    (cloud/main_improved_threelayer.py:204-209, 381-398): one 360-ray scan into the device voxel map, then the
    20 m local grid at 0.2 m (10^6 cells) -> 20 obstacle spheres, then the safety check of 8192 30-step plans.
    Device-event times of the kernels with resident inputs; seeded synthetic scene."""
    from dart_planner_amd.perception.explicit_geometric_mapper import ExplicitGeometricMapper
    rng = np.random.default_rng(5)
    m = ExplicitGeometricMapper(resolution=0.2, max_range=50.0, ops=ops)
    for _ in range(8):
        m.add_obstacle(rng.uniform(-8, 8, 3) + [0, 0, 2], float(rng.uniform(0.5, 1.5)))
    n = 360
    ang = 2 * np.pi * np.arange(n) / n
    dirs = np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)
    hit = rng.random(n) < 0.1
    dist = np.where(hit, rng.uniform(2.0, 20.0, n), 50.0)
    org = np.tile([0.3, 0.1, 2.0], (n, 1))

    def dev_ms(fn, reps):
        fn(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    m.map.update_rays(org, dirs, dist, hit.astype(np.int32))          # first scan: creates the voxels, sizes the table
    upd = dev_ms(lambda: m.map.update_rays(org, dirs, dist, hit.astype(np.int32)), 5)
    centre = np.array([0.3, 0.1, 2.0])
    grid = dev_ms(lambda: m.map.local_spheres(centre, 20.0, 0.6, 20, 1.0), 20)
    plans = torch.rand(8192, 30, 3, device=dev, dtype=torch.float32) * 20 - 10
    safe = dev_ms(lambda: m.map.trajectories_safe(plans, margin=1.0, threshold=0.6), 20)
    return {"what": "device voxel map (reference: ExplicitGeometricMapper's dict walk), float64 index arithmetic, bit-exact",
            "update_map_360_rays_ms": upd, "local_grid_1e6_cells_to_spheres_ms": grid, "trajectory_safe_8192x30_ms": safe,
            "voxels": len(m.map), "table_capacity": m.map.capacity}


def profiled_traffic(B, N):
    """HBM bytes PER ROLLOUT of the timed kernel at the timed launch shape, from the newest committed rocprofv3
    PMC passes (profiles/rNN_traffic.json: FETCH_SIZE x2 on gfx950 + WRITE_SIZE, separate passes, same command
    without the graph) -- PMC counters cannot be read from inside this process.  None if no profile of this
    workload is committed.  -> (bytes_per_rollout, file name)"""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json"))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("batch") == B and d.get("horizon") == N and d.get("steps_per_launch", 1) == 64:
            best = (float(d["traffic_bytes_per_launch"]) / float(d["rollouts_per_launch"]), os.path.basename(f))
    return best


def config_legs(torch, ops, dev, min_ms):
    """BASELINE.json configs 2 and 3 as their own legs, each with its own roofline:
      cfg2: batch 1024, horizon 30, rollout + thrust gradient, f32          -- 4*(6N+10) B per rollout
      cfg3: batch 8192, horizon 50, K = 16 mapper spheres fused (cmin, viol) -- 4*(6N+12) B per rollout
    `single` = one launch per batch (what one planner sees), `batched` = 64 independent batches per launch
    (grid.y).  Inputs cycle through a ring of distinct batches larger than the Infinity Cache; launches are
    replayed from a hipGraph; time = HIP events around the replays on the launch stream."""
    from dart_planner_amd.capi import Params
    out = {}
    S = 64
    for name, N, B, nsph in (("cfg2", 30, 1024, 0), ("cfg3", 50, 8192, 16)):
        prm = Params.reference_defaults(horizon=N)
        slot = 4 * B * ((9 + 3 * N) + (1 + 3 * N) + (2 if nsph else 0))
        ring = S * max(2, math.ceil(math.ceil(320 * 2 ** 20 / slot) / S))
        p0, v0, goal, T, cost, grad = make_ring(torch, dev, B, N, ring, seed=21 + N)
        g = torch.Generator(device=dev); g.manual_seed(2)
        sph = None
        if nsph:
            # spheres as the mapper produces them: radius 1.0, centres ~ U(0,15)^3 snapped to 0.5 m
            sph = torch.cat([torch.round(torch.rand(nsph, 3, device=dev, generator=g) * 30) / 2, torch.ones(nsph, 1, device=dev)], 1).contiguous()
            cmin, viol = torch.empty(ring, B, device=dev), torch.empty(ring, B, device=dev)
        bpr = 4 * (6 * N + (12 if nsph else 10))
        legs = {}
        for mode, per_l in (("single", 1), ("batched", S)):
            def one(i0):
                s0 = i0 % ring
                if nsph:
                    if per_l == 1:
                        ops.rollout_obstacles(prm, p0[s0], v0[s0], goal[s0], T[s0], sph, out=(cost[s0], grad[s0], cmin[s0], viol[s0]))
                    else:
                        ops.rollout_obstacles_batched(prm, p0[s0:s0 + per_l], v0[s0:s0 + per_l], goal[s0:s0 + per_l], T[s0:s0 + per_l], sph,
                                                      cost[s0:s0 + per_l], grad[s0:s0 + per_l], cmin[s0:s0 + per_l], viol[s0:s0 + per_l])
                elif per_l == 1:
                    ops.rollout_cost_grad(prm, p0[s0], v0[s0], goal[s0], T[s0], out=(cost[s0], grad[s0]))
                else:
                    ops.rollout_cost_grad_batched(prm, p0[s0:s0 + per_l], v0[s0:s0 + per_l], goal[s0:s0 + per_l], T[s0:s0 + per_l],
                                                  cost[s0:s0 + per_l], grad[s0:s0 + per_l])
            nl = ring // per_l                                   # launches per graph: one sweep of the ring
            nl = min(nl, MAX_GRAPH_NODES)
            body = lambda: [one(i * per_l) for i in range(nl)]
            body(); torch.cuda.synchronize()
            graph = capture(torch, dev, body)
            warm_device(torch, graph.replay, chunk=1)
            ms1 = device_ms(torch, graph.replay, 2)
            reps = max(2, math.ceil(min_ms / max(ms1, 1e-6)))
            ms = device_ms(torch, graph.replay, reps) / nl
            del graph
            gbps = bpr * B * per_l / (ms * 1e-3) / 1e9
            legs[mode] = {"launch_us": ms * 1e3, "rollouts_per_launch": B * per_l, "rollouts_per_s": B * per_l / (ms * 1e-3),
                          "launches_timed": reps * nl,
                          "roofline": {"bound": "hbm", "achieved": gbps, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": gbps / HBM_PEAK_GBPS,
                                       "bytes_per_rollout": bpr}}
        out[name] = {"workload": f"horizon={N}, batch={B}, f32 rollout + cost + thrust gradient" + (f" fused with {nsph} sphere-obstacle residuals (min, violation)" if nsph else ""),
                     "ring": ring, **legs}
        del p0, v0, goal, T, cost, grad
        torch.cuda.empty_cache()
    return out


def iterated_leg(torch, ops, dev, B, N, min_ms, ks=(0, 1, 4, 16, 64)):
    """The on-device iteration loop (se3mpc_rollout_iterate_*): K projected-gradient iterations of the shooting form + one last
    evaluation in ONE launch, thrust sequences resident in registers, against the same K + 1 evaluations issued as one launch each
    (`single_launch` leg).  Same batch (8192 x horizon 30), ring of distinct batches, hipGraph replay, HIP-event time."""
    from dart_planner_amd.capi import Params
    prm = Params.reference_defaults(horizon=N)
    slot = 4 * B * ((9 + 3 * N) + (1 + 6 * N))
    ring = max(128, math.ceil(320 * 2 ** 20 / slot))                 # >= two 64-batch launches on disjoint slots
    p0, v0, goal, T, cost, grad = make_ring(torch, dev, B, N, ring, seed=77)
    Tout = torch.empty_like(T)
    step = 0.9
    out = {"what": f"horizon={N}, batch={B}: K iterations of T <- clip(T - {step} dcost/dT) + a final evaluation per launch; "
                   "K + 1 rollouts per trajectory per launch, HBM traffic of one", "per_K": []}
    base_us = None
    for K in ks:
        nl = min(ring, 256)
        body = lambda: [ops.rollout_iterate(prm, p0[i], v0[i], goal[i], T[i], K, step, out=(Tout[i], cost[i], grad[i])) for i in range(nl)]
        body(); torch.cuda.synchronize()
        graph = capture(torch, dev, body)
        warm_device(torch, graph.replay, chunk=1)
        ms1 = device_ms(torch, graph.replay, 2)
        reps = max(2, math.ceil(min_ms / max(ms1, 1e-6)))
        us = device_ms(torch, graph.replay, reps) / nl * 1e3
        del graph
        if K == 0 or base_us is None:
            base_us = us if K == 0 else None
        hbm = 4 * (9 + 3 * N) + 4 * (1 + 6 * N)                 # per trajectory: read p0, v0, goal, T; write T, gradient, cost
        out["per_K"].append({"K": K, "launch_us": us, "us_per_iteration": None if (K == 0 or base_us is None) else (us - base_us) / K,
                             "rollouts_per_s": B * (K + 1) / (us * 1e-6), "hbm_bytes_per_launch": hbm * B,
                             "hbm_GB_per_s": hbm * B / (us * 1e-6) / 1e9,
                             "rollout_equivalent_GB_per_s": 4 * (6 * N + 10) * B * (K + 1) / (us * 1e-6) / 1e9})
    # the same loop over 64 independent batches per launch (grid.y), K = 16: the chip is full, the bound is VALU issue
    S, K = 64, 16
    if ring >= 2 * S:
        nl = ring // S
        body = lambda: [ops.rollout_iterate(prm, p0[i * S:(i + 1) * S], v0[i * S:(i + 1) * S], goal[i * S:(i + 1) * S], T[i * S:(i + 1) * S], K, step,
                                            out=(Tout[i * S:(i + 1) * S], cost[i * S:(i + 1) * S], grad[i * S:(i + 1) * S])) for i in range(nl)]
        body(); torch.cuda.synchronize()
        graph = capture(torch, dev, body)
        warm_device(torch, graph.replay, chunk=1)
        ms1 = device_ms(torch, graph.replay, 2)
        us = device_ms(torch, graph.replay, max(2, math.ceil(min_ms / max(ms1, 1e-6)))) / nl * 1e3
        del graph
        out["batched_64_K16"] = {"launch_us": us, "rollouts_per_launch": B * S * (K + 1), "rollouts_per_s": B * S * (K + 1) / (us * 1e-6),
                                 "us_per_iteration_per_batch": us / S / (K + 1), "hbm_GB_per_s": (4 * (9 + 3 * N) + 4 * (1 + 6 * N)) * B * S / (us * 1e-6) / 1e9}
    # BASELINE config 3 INSIDE the loop (se3mpc_rollout_iterate_obstacles_*: running cost + obstacle penalty, the build's extension):
    # horizon 50, 8192 trajectories, 16 mapper-style spheres (radius 1.0, 0.5 m grid, margin 1.5), one launch per K
    N3, K3 = 50, 16
    prm3 = Params.reference_defaults(horizon=N3)
    slot3 = 4 * B * ((9 + 3 * N3) + (1 + 6 * N3))
    ring3 = max(32, math.ceil(320 * 2 ** 20 / slot3))
    q0, w0, gl3, T3, cost3, grad3 = make_ring(torch, dev, B, N3, ring3, seed=78)
    q0.mul_(0.1); gl3.mul_(0.1)
    Tout3 = torch.empty_like(T3)
    gs = torch.Generator(device="cpu"); gs.manual_seed(2)
    sph = torch.cat([torch.round(torch.rand(K3, 3, generator=gs) * 30) / 2 - 3.75, torch.ones(K3, 1)], dim=1).to(dev)
    rows, base3 = [], None
    for K in (0, 1, 4, 16):
        nl = min(ring3, 64)
        body = lambda: [ops.rollout_iterate(prm3, q0[i], w0[i], gl3[i], T3[i], K, 1e-3, out=(Tout3[i], cost3[i], grad3[i]), spheres=sph,
                                            obstacle_weight=1000.0, want_penalty=False) for i in range(nl)]
        body(); torch.cuda.synchronize()
        graph = capture(torch, dev, body)
        warm_device(torch, graph.replay, chunk=1)
        ms1 = device_ms(torch, graph.replay, 2)
        us = device_ms(torch, graph.replay, max(2, math.ceil(min_ms / max(ms1, 1e-6)))) / nl * 1e3
        del graph
        base3 = us if K == 0 else base3
        rows.append({"K": K, "launch_us": us, "us_per_iteration": None if K == 0 else (us - base3) / K, "rollouts_per_s": B * (K + 1) / (us * 1e-6),
                     "distance_evaluations_per_s": B * (K + 1) * N3 * K3 / (us * 1e-6)})
    out["cfg3_obstacles"] = {"what": f"horizon={N3}, batch={B}, {K3} spheres: K obstacle-aware iterations + a final evaluation per launch "
                                     f"({N3 * K3} distance evaluations per trajectory and pass; thrusts, states and obstacle gradients stay on chip)",
                             "per_K": rows}
    out["note"] = ("rollout_equivalent_GB_per_s prices every in-register rollout at the 4*(6N+10) B a stand-alone launch would move; it may "
                   "exceed the HBM peak -- the iterations in between touch no memory -- and is NOT a roofline fraction; the bound of this "
                   "kernel is the dependent-instruction latency of the 2N-step sweep per iteration")
    return out


def closed_loop_leg(torch, ops, dev):
    """BASELINE.json config 5's named test shape (reference tests/test_monte_carlo_sim.py: 33 planning cycles of 0.15 s) as a
    receding-horizon Monte-Carlo entirely on the device: per cycle ONE batched solve launch (every run re-plans from its own state)
    and ONE closed-loop launch (15 x plan sample -> geometric controller -> simulator at 100 Hz, plans read in place from the solver's
    outputs).  4096 runs, float32; wall time with one synchronise at the end."""
    from dart_planner_amd.capi import Params
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    S, cycles, substeps, sim_dt = 4096, 33, 15, 0.01
    prm = Params.reference_defaults()
    N = prm.horizon
    cp, sp = ops.lib.controller_default_params(), ops.lib.simulator_default_params()
    g = torch.Generator(device=dev); g.manual_seed(5)
    res = {}
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        p0 = torch.tensor([0.0, 0.0, 2.0], dtype=dtype, device=dev).repeat(S, 1) + 0.2 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
        v0 = 0.3 * torch.randn(S, 3, dtype=dtype, device=dev, generator=g)
        goal = torch.tensor([8.0, 0.0, 5.0], dtype=dtype, device=dev).repeat(S, 1).contiguous()
        wind = torch.randn(S, 3, dtype=dtype, device=dev, generator=g).contiguous()
        mc = ClosedLoopMonteCarlo(ops, prm, cp, sp)

        def run():
            return mc.run(p0, v0, goal, cycles, substeps, sim_dt, wind=wind)["pos"]
        run(); torch.cuda.synchronize()
        warm_device(torch, run, chunk=1)
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pos = run()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        el = float(np.median(ts))
        replay = mc.capture(S, dtype, cycles, substeps, sim_dt)
        replay(p0, v0, goal, wind); torch.cuda.synchronize()
        warm_device(torch, lambda: replay(p0, v0, goal, wind), chunk=1)
        tg = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outg = replay(p0, v0, goal, wind)
            torch.cuda.synchronize()
            tg.append(time.perf_counter() - t0)
        eg = float(np.median(tg))
        # the same Monte-Carlo in ONE launch (se3mpc_monte_carlo_*: same code, same bits; no kernel boundary at which all drones wait for the slowest)
        def run1():
            return mc.run_fused(p0, v0, goal, cycles, substeps, sim_dt, wind=wind)["pos"]
        pos1 = run1(); torch.cuda.synchronize()
        warm_device(torch, run1, chunk=1)
        t1 = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pos1 = run1()
            torch.cuda.synchronize()
            t1.append(time.perf_counter() - t0)
        e1 = float(np.median(t1))
        # the headline keys are the product's own path for this workload (the whole run in ONE launch); the two-launch-per-cycle forms it is
        # bit-identical to stay beside it
        res[name] = {"wall_ms_per_monte_carlo": e1 * 1e3, "runs_per_s": S / e1, "plans_per_s": S * cycles / e1,
                     "control_steps_per_s": S * cycles * substeps / e1, "form": "one launch (se3mpc_monte_carlo_*)",
                     "finite": bool(torch.isfinite(pos1).all()), "equals_two_launch_form": bool(torch.equal(pos1, pos)),
                     "two_launch_wall_ms_per_monte_carlo": el * 1e3, "two_launch_runs_per_s": S / el,
                     "two_launch_hipgraph_wall_ms_per_monte_carlo": eg * 1e3, "two_launch_hipgraph_runs_per_s": S / eg,
                     "two_launch_hipgraph_equals_eager": bool(torch.equal(outg["pos"], pos))}
        del replay
    return {"what": f"{S} closed-loop runs x {cycles} planning cycles x {substeps} control+simulator steps (horizon-6 plans, DI defaults), "
                    "the whole run in ONE launch (wall_ms_per_monte_carlo) beside 2 launches per cycle, eager and as one hipGraph (two_launch_*); no host arithmetic", **res}


def sweep(torch, ops, prm, dev, N):
    """Saturating batches (one launch each, eager): where the HBM roofline is actually reachable."""
    out = []
    for B in (65536, 1 << 20, 1 << 22):
        p0, v0, goal, T, cost, grad = make_ring(torch, dev, B, N, 2, seed=11)
        for _ in range(3):
            ops.rollout_cost_grad(prm, p0[0], v0[0], goal[0], T[0], out=(cost[0], grad[0]))
        torch.cuda.synchronize()
        reps = 40
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            ops.rollout_cost_grad(prm, p0[i & 1], v0[i & 1], goal[i & 1], T[i & 1], out=(cost[i & 1], grad[i & 1]))
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        gbps = 4 * (6 * N + 10) * B / (ms * 1e-3) / 1e9
        out.append({"batch": B, "kernel_us": ms * 1e3, "rollouts_per_s": B / (ms * 1e-3), "GB_per_s": gbps,
                    "frac_of_peak": gbps / HBM_PEAK_GBPS})
        del p0, v0, goal, T, cost, grad
    return out


if __name__ == "__main__":
    main()
