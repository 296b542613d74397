"""Closed-loop MPPI Monte-Carlo probe.  B in {256, 4096} drones, S = 256 samples, 8 iterations, N = 30 at a plan step of
0.1 s, K in {0, 16} spheres, 33 cycles x 15 simulator steps of 0.01 s, f32 and f64, in three forms:
  fused   one se3mpc_mppi_closed_loop_* launch for the whole run
  calls   `cycles` launches of one cycle each
  chain   per cycle, the entry points that existed before se3mpc_mppi_closed_loop_*: transposes of the state, se3mpc_mppi_*,
          se3mpc_rollout_cost_grad_* with states, se3mpc_extract_*, three transposes, se3mpc_closed_loop_*, a host-side shift of the nominal
          (no clearance output: the chain has none).  It uses nothing newer, so `--package-root DIR` can point it at a checkout of an
          earlier commit with that commit's own library: the yardstick.
HIP events around warm runs, 5 warm-ups, median of 20, as tools/gpu_probe_mppi.py.  One form per process, so that a driver can alternate them:
  python tools/gpu_probe_mppi_closed_loop.py fused|calls|chain|planner|outcome [--package-root DIR] [--out FILE] [--only B,K,dtype]
`planner`: se3mpc_mppi_* alone next to the fused kernel with substeps = 0 (what the lower occupancy costs the MPPI phase).
`outcome`: the closed-loop result for SE3MPCPlanner.MPPI_*'s defaults (and for sigma = 3 N, temperature = 200) over 4096 drones (final goal
distance, minimum clearance)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(B, K, dt) for B in (256, 4096) for K in (0, 16) for dt in ("float32", "float64")]
N, S, ITERS, CYCLES, SUBSTEPS, SIM_DT, PLAN_DT, SIGMA, LAM, W_OBS = 30, 256, 8, 33, 15, 0.01, 0.1, 4.0, 100.0, 1000.0


def scene(torch, B, K, dtype, seed=2):
    rng = np.random.default_rng(seed)
    tdt = getattr(torch, dtype)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=tdt, device="cuda:0")
    p0 = rng.uniform(-1, 1, (B, 3)) + [0, 0, 2]
    v0 = rng.uniform(-0.5, 0.5, (B, 3))
    goal = rng.uniform(-4, 4, (B, 3)) + [0, 0, 6]
    sph = None
    if K:
        c = rng.uniform(-4, 4, (K, 3)) + [0, 0, 5]
        sph = dev(np.concatenate([c, np.full((K, 1), 0.5)], axis=1))
    wind = dev(rng.normal(0, 0.5, (B, 3)))
    return dev(p0), dev(v0), dev(goal), sph, wind


def timed(torch, setup, run, reps=20, warmup=5):
    ts = []
    for i in range(warmup + reps):
        state = setup()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(state); e1.record(); e1.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1) * 1e3)
    return dict(us_median=float(np.median(ts)), us_min=float(np.min(ts)), us_max=float(np.max(ts)))


def start(torch, ops, cp, prm, p0, v0, lane_U=False):
    B = p0.shape[0]
    U = torch.zeros(B, N, 3, dtype=p0.dtype, device=p0.device)
    U[:, :, 2] = prm.mass * prm.gravity
    if lane_U:
        U = U.reshape(B, 3 * N).t().contiguous()
    return dict(pos=p0.clone(), vel=v0.clone(), att=torch.zeros_like(p0), om=torch.zeros_like(p0),
                time=torch.zeros(B, dtype=torch.float64, device=p0.device), st=ops.controller_state(cp, B), U=U)


def loop_forms(form, shapes):
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend("cuda:0"))
    cp, sp = ops.lib.controller_default_params(), ops.lib.simulator_default_params()
    prm = Params.reference_defaults(horizon=N, dt=PLAN_DT)
    shift = int(np.floor(SUBSTEPS * SIM_DT / PLAN_DT + 0.5))
    rows = []
    for B, K, dtype in shapes:
        p0, v0, goal, sph, wind = scene(torch, B, K, dtype)
        w = W_OBS if K else 0.0

        def one(s, cycles, base):
            return ops.mppi_closed_loop(prm, cp, sp, s["st"], s["time"], s["pos"], s["vel"], s["att"], s["om"], goal, s["U"], cycles, SUBSTEPS, SIM_DT, S,
                                        ITERS, SIGMA, LAM, seed=1, cycle_base=base, shift=shift, spheres=sph, obstacle_weight=w, wind=wind,
                                        want_trace=False, clearance=s.get("clr"))

        def setup():
            s = start(torch, ops, cp, prm, p0, v0)
            s["clr"] = torch.full((B,), float("inf"), dtype=p0.dtype, device=p0.device) if K else None
            return s

        if form == "fused":
            run = lambda s: one(s, CYCLES, 0)
        else:
            def run(s):
                for c in range(CYCLES):
                    one(s, 1, c)
        r = dict(form=form, B=B, K=K, dtype=dtype, N=N, S=S, iters=ITERS, cycles=CYCLES, substeps=SUBSTEPS, **timed(torch, setup, run))
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def chain_form(shapes):
    """The per-cycle chain of the entry points older than se3mpc_mppi_closed_loop_* (runs on an earlier checkout too)."""
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend("cuda:0"))
    cp, sp = ops.lib.controller_default_params(), ops.lib.simulator_default_params()
    prm = Params.reference_defaults(horizon=N, dt=PLAN_DT)
    shift = int(np.floor(SUBSTEPS * SIM_DT / PLAN_DT + 0.5))
    rows = []
    for B, K, dtype in shapes:
        p0, v0, goal, sph, wind = scene(torch, B, K, dtype)
        w = W_OBS if K else 0.0
        goal_l = goal.t().contiguous()
        k = torch.arange(N, dtype=torch.float64, device="cuda:0")
        tail = torch.zeros(3 * shift, B, dtype=p0.dtype, device="cuda:0")
        tail[2::3] = prm.mass * prm.gravity

        def run(s):
            for c in range(CYCLES):
                p_l, v_l = ops.transpose(s["pos"]), ops.transpose(s["vel"])
                o = ops.mppi(prm, p_l, v_l, goal_l, s["U"], S, ITERS, SIGMA, LAM, seed=1, iter_base=c * ITERS, spheres=sph, obstacle_weight=w,
                             want_trace=False, want_keys=False)
                _, _, P, V = ops.rollout_cost_grad(prm, p_l, v_l, goal_l, o["U"], want_grad=False, want_states=True)
                A = ops.extract(prm, o["U"])[0]
                Pt, Vt, At = ops.transpose(P), ops.transpose(V), ops.transpose(A)
                stamps = (c * SUBSTEPS * SIM_DT) + k * prm.dt
                ops.closed_loop(cp, sp, s["st"], s["time"], s["pos"], s["vel"], s["att"], s["om"], stamps, Pt.view(B, N, 3), Vt.view(B, N, 3),
                                At.view(B, N, 3), nsteps=SUBSTEPS, sim_dt=SIM_DT, wind=wind, stop_at_plan_end=False)
                s["U"] = torch.cat([o["U"][3 * shift:], tail], dim=0)

        r = dict(form="chain", B=B, K=K, dtype=dtype, N=N, S=S, iters=ITERS, cycles=CYCLES, substeps=SUBSTEPS,
                 **timed(torch, lambda: start(torch, ops, cp, prm, p0, v0, lane_U=True), run))
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def planner_part(shapes):
    """se3mpc_mppi_* (four wavefronts per SIMD) next to the fused kernel's plan phase alone (substeps = 0, one cycle)."""
    import torch
    from dart_planner_amd.capi import Params
    from dart_planner_amd.ops import Ops, TorchBackend
    ops = Ops(TorchBackend("cuda:0"))
    cp, sp = ops.lib.controller_default_params(), ops.lib.simulator_default_params()
    prm = Params.reference_defaults(horizon=N, dt=PLAN_DT)
    rows = []
    for B, K, dtype in shapes:
        p0, v0, goal, sph, wind = scene(torch, B, K, dtype)
        w = W_OBS if K else 0.0
        p_l, v_l, goal_l = p0.t().contiguous(), v0.t().contiguous(), goal.t().contiguous()
        a = timed(torch, lambda: start(torch, ops, cp, prm, p0, v0, lane_U=True),
                  lambda s: ops.mppi(prm, p_l, v_l, goal_l, s["U"], S, ITERS, SIGMA, LAM, seed=1, spheres=sph, obstacle_weight=w, want_trace=False, want_keys=False))
        b = timed(torch, lambda: start(torch, ops, cp, prm, p0, v0),
                  lambda s: ops.mppi_closed_loop(prm, cp, sp, s["st"], s["time"], s["pos"], s["vel"], s["att"], s["om"], goal, s["U"], 1, 0, SIM_DT, S, ITERS,
                                                 SIGMA, LAM, seed=1, shift=0, spheres=sph, obstacle_weight=w, want_trace=False, want_clearance=False))
        r = dict(form="planner", B=B, K=K, dtype=dtype, mppi_us=a["us_median"], fused_plan_phase_us=b["us_median"], ratio=b["us_median"] / a["us_median"])
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def outcome_part():
    """SE3MPCPlanner.MPPI_*'s defaults in the loop, 4096 drones, float32.  The reference's simulator applies thrust along world z
    whatever the attitude, so the scene is vertical: drones below a sphere (radius 1 m at z = 5), goals 8 m above their start, the planner's
    thrust box narrowed to near-vertical thrust (max_tilt_angle 0.02 rad), planner / controller / simulator at mass 1 kg."""
    import torch
    from dart_planner_amd.capi import Params, SimulatorParams
    from dart_planner_amd.control.closed_loop import ClosedLoopMonteCarlo
    from dart_planner_amd.ops import Ops, TorchBackend
    from dart_planner_amd.planning.se3_mpc_planner import SE3MPCPlanner as PL
    ops = Ops(TorchBackend("cuda:0"))
    prm = Params.reference_defaults(horizon=N, dt=PLAN_DT, mass=1.0, gravity=9.80665, max_thrust=20.0, max_tilt_angle=0.02)
    mcl = ClosedLoopMonteCarlo(ops, prm, simulator=SimulatorParams.reference_defaults(mass=1.0, gravity=9.80665))
    B = 4096
    rng = np.random.default_rng(7)
    xy = rng.uniform(-1.5, 1.5, (B, 2))
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")
    p0 = dev(np.concatenate([xy, rng.uniform(0.5, 1.5, (B, 1))], axis=1))
    goal = p0 + dev([0.0, 0.0, 8.0])
    sph = dev([[0.0, 0.0, 5.0, 1.0]])
    crossing = np.linalg.norm(xy, axis=1) < 1.0
    rows = []
    for w, (sigma, lam) in [(w, sl) for sl in ((PL.MPPI_SIGMA, PL.MPPI_TEMPERATURE), (3.0, 200.0)) for w in (0.0, W_OBS)]:
        out = mcl.run_mppi_fused(p0, torch.zeros_like(p0), goal, CYCLES, SUBSTEPS, SIM_DT, PL.MPPI_SAMPLES, PL.MPPI_ITERS, sigma, lam,
                                 seed=3, spheres=sph, obstacle_weight=w)
        dist = (out["pos"] - goal).norm(dim=1).cpu().numpy()
        clr = out["clearance"].cpu().numpy()
        pct = lambda a: {f"p{q}": float(np.percentile(a, q)) for q in (0, 5, 50, 95, 100)}
        r = dict(form="outcome", B=B, samples=PL.MPPI_SAMPLES, iters=PL.MPPI_ITERS, sigma=sigma, temperature=lam, obstacle_weight=w,
                 seconds_flown=CYCLES * SUBSTEPS * SIM_DT, start_goal_distance=8.0, drones_whose_line_crosses_the_sphere=int(crossing.sum()),
                 final_goal_distance=pct(dist), final_height_minus_goal=pct((out["pos"] - goal)[:, 2].cpu().numpy()), min_clearance=pct(clr), min_clearance_of_crossing_drones=pct(clr[crossing]),
                 drones_inside_the_sphere=int((clr < 0).sum()), drones_nearer_the_goal=int((dist < 8.0).sum()))
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["fused", "calls", "chain", "planner", "outcome"])
    ap.add_argument("--package-root", default=ROOT, help="checkout whose dart_planner_amd (and library) to drive")
    ap.add_argument("--out", default=None, help="append the rows to this JSON-lines file")
    ap.add_argument("--only", default=None, help="B,K,dtype: one shape")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    shapes = SHAPES
    if a.only:
        B, K, dt = a.only.split(",")
        shapes = [(int(B), int(K), dt)]
    rows = {"fused": lambda: loop_forms("fused", shapes), "calls": lambda: loop_forms("calls", shapes), "chain": lambda: chain_form(shapes),
            "planner": lambda: planner_part(shapes), "outcome": outcome_part}[a.part]()
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(dict(r, package_root=os.path.relpath(os.path.abspath(a.package_root), ROOT))) + "\n")


if __name__ == "__main__":
    main()
