"""Oracle of MPPI around moving spheres -- TEST INFRASTRUCTURE (the product never imports it): a float64 NumPy restatement of the
contract of se3mpc_mppi_moving_* and se3mpc_mppi_closed_loop_moving_* (include/se3mpc.h).  The noise, the samples, the thrust box and the
running cost are those of tests/mppi_oracle.py (imported); only the penalty is restated, against the centres at each step's time, and the
closed loop's clearance rule beside it."""
import numpy as np

import mppi_oracle as mo
from oracle import se3mpc_oracle as orc


def rounded(tau, dtype):
    """tR: the time(s) tau (float64) rounded to the kernel's type."""
    return np.asarray(tau, np.float64).astype(dtype).astype(np.float64)


def step_times(N, dt, sphere_t0, dtype=np.float64, base=0.0):
    """tR_k of the planner: tau_k = sphere_t0 + (base + k dt), base = the plan's first stamp ((double)(C * substeps) * sim_dt in the closed loop,
    0 for the planner entry), in the order the contract writes it."""
    return rounded(sphere_t0 + (base + np.arange(N, dtype=np.float64) * dt), dtype)


def centres(spheres, vel, tR):
    """(..., K, 3): c_j + v_j * tR for every time in tR (...)."""
    sp, vel = np.asarray(spheres, float).reshape(-1, 4), np.asarray(vel, float).reshape(-1, 3)
    return sp[:, :3] + vel * np.asarray(tR, float)[..., None, None]


def residuals(P, spheres, vel, tR, cfg):
    """c_kj = |P_k - centre_j(k)|^2 - (r_j + margin)^2: P (..., N, 3), tR (N,) -> (..., N, K)."""
    d = np.asarray(P, float)[..., :, None, :] - centres(spheres, vel, tR)
    return np.sum(d * d, axis=-1) - (np.asarray(spheres, float).reshape(-1, 4)[:, 3] + cfg.safety_margin) ** 2


def penalty(p0, v0, T, spheres, vel, tR, cfg, obstacle_weight):
    P, _ = orc.rollout(p0, v0, T, cfg)
    h = np.maximum(0.0, -residuals(P, spheres, vel, tR, cfg))
    return obstacle_weight * np.sum(h * h, axis=(-1, -2))


def cost(p0, v0, goal, T, cfg, spheres=None, vel=None, tR=None, obstacle_weight=0.0):
    c = orc.rollout_cost(p0, v0, goal, T, cfg)
    if spheres is not None and len(spheres):
        c = c + penalty(p0, v0, T, spheres, vel, tR, cfg, obstacle_weight)
    return c


def mppi(p0, v0, goal, U, q, S, iters, sigma, temperature, seed, cfg, iter_base=0, spheres=None, vel=None, sphere_t0=0.0, obstacle_weight=0.0,
         dtype=np.float64, base=0.0):
    """mppi_oracle.mppi with the penalty at per-step centres: one problem -> (U (N, 3), cost at U, trace (iters,))."""
    U = np.asarray(U, float).copy()
    lo, hi = mo.thrust_box(cfg)
    tR = step_times(U.shape[0], cfg.dt, sphere_t0, dtype, base)
    trace = []
    for i in range(iters):
        T, _, _ = mo.samples(U, q, iter_base + i, S, sigma, seed, cfg, dtype)
        c = cost(p0, v0, goal, T, cfg, spheres, vel, tR, obstacle_weight)
        m = np.min(c)
        w = np.exp(-(c - m) / temperature)
        U = np.clip(np.einsum("s,sna->na", w, T) / np.sum(w), lo, hi)
        trace.append(m)
    return U, float(cost(p0, v0, goal, U, cfg, spheres, vel, tR, obstacle_weight)), np.array(trace)


def clearance(positions, tau, spheres, vel, dtype=np.float64):
    """The closed loop's rule: positions (n, B, 3) the simulator produced, tau (n,) the time each is measured at (float64, rounded here
    to the kernel's type) -> (B,) min over (step, j) of |pos - centre_j(tau)| - r_j with the raw radii."""
    cen = centres(spheres, vel, rounded(tau, dtype))                                     # (n, K, 3)
    dist = np.linalg.norm(np.asarray(positions, float)[:, :, None, :] - cen[:, None], axis=-1) - np.asarray(spheres, float).reshape(-1, 4)[:, 3]
    return dist.min(axis=(0, 2))
