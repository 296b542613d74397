"""Oracle of MPPI around tracked spheres -- TEST INFRASTRUCTURE (the product never imports it): a float64 NumPy restatement of what
include/se3mpc.h says about se3mpc_mppi_tracks_*: behind the K moving rows of tests/mppi_moving_oracle.py (imported, not edited) come Kt
rows whose centre is given per step of the horizon.  Written from the header comment, not from the kernel."""
import numpy as np

import mppi_moving_oracle as mvo
import mppi_oracle as mo
from oracle import se3mpc_oracle as orc


def track_residuals(P, tracks, cfg):
    """c_kj = |P_k - track[k][j]|^2 - (r_kj + margin)^2: P (..., N, 3), tracks (N, Kt, 4) -> (..., N, Kt)."""
    tr = np.asarray(tracks, float)
    d = np.asarray(P, float)[..., :, None, :] - tr[:, :, :3]
    return np.sum(d * d, axis=-1) - (tr[:, :, 3] + cfg.safety_margin) ** 2


def track_penalty(p0, v0, T, tracks, cfg, obstacle_weight):
    """obstacle_weight * sum_k sum_j max(0, -c_kj)^2 over the tracked rows alone."""
    P, _ = orc.rollout(p0, v0, T, cfg)
    h = np.maximum(0.0, -track_residuals(P, tracks, cfg))
    return obstacle_weight * np.sum(h * h, axis=(-1, -2))


def cost(p0, v0, goal, T, cfg, spheres=None, vel=None, tR=None, tracks=None, obstacle_weight=0.0):
    """mppi_moving_oracle.cost plus the tracked rows' penalty."""
    c = mvo.cost(p0, v0, goal, T, cfg, spheres, vel, tR, obstacle_weight)
    if tracks is not None and np.asarray(tracks).shape[1]:
        c = c + track_penalty(p0, v0, T, tracks, cfg, obstacle_weight)
    return c


def mppi(p0, v0, goal, U, q, S, iters, sigma, temperature, seed, cfg, iter_base=0, spheres=None, vel=None, sphere_t0=0.0, tracks=None,
         obstacle_weight=0.0, dtype=np.float64, base=0.0):
    """mppi_moving_oracle.mppi with the tracked rows in the cost: one problem -> (U (N, 3), cost at U, trace (iters,))."""
    U = np.asarray(U, float).copy()
    lo, hi = mo.thrust_box(cfg)
    tR = mvo.step_times(U.shape[0], cfg.dt, sphere_t0, dtype, base)
    trace = []
    for i in range(iters):
        T, _, _ = mo.samples(U, q, iter_base + i, S, sigma, seed, cfg, dtype)
        c = cost(p0, v0, goal, T, cfg, spheres, vel, tR, tracks, obstacle_weight)
        m = np.min(c)
        w = np.exp(-(c - m) / temperature)
        U = np.clip(np.einsum("s,sna->na", w, T) / np.sum(w), lo, hi)
        trace.append(m)
    return U, float(cost(p0, v0, goal, U, cfg, spheres, vel, tR, tracks, obstacle_weight)), np.array(trace)
