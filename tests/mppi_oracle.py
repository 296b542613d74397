"""MPPI oracle -- TEST INFRASTRUCTURE (the product never imports it): vectorised NumPy Philox4x32-10, Box-Muller, and the MPPI
update of include/se3mpc.h (se3mpc_mppi_*) in float64 on top of oracle.se3mpc_oracle.rollout_cost / obstacle_penalty_grad."""
import numpy as np

from oracle import se3mpc_oracle as orc

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

# Random123's known answers for Philox4x32-10: (counter, key) -> output
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Broadcast uint32 arrays in, four uint32 arrays out."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        a, b = M0 * c[0], M1 * c[2]
        c = [((b >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & MASK, b & MASK, ((a >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & MASK, a & MASK]
    return [x.astype(np.uint32) for x in c]


def raw_words(q, s, g, k, seed):
    """Philox words of counter (q, s, g, k) under the key of `seed`: (4, ...) uint32."""
    return np.stack(philox4x32_10(q, s, g, k, int(seed) & 0xFFFFFFFF, int(seed) >> 32))


def uniforms(x, dtype):
    """u = (x + 0.5) * 2^-32 in the kernel's arithmetic type (float32: the conversion and the add round as on the device)."""
    dt = np.dtype(dtype)
    return ((x.astype(dt) + dt.type(0.5)) * dt.type(2.0 ** -32)).astype(np.float64)


def normals(x, dtype=np.float64):
    """Box-Muller on the (4, ...) words: (..., 3) float64 normals from the kernel-precision uniforms."""
    u = uniforms(x, dtype)
    r01, r23 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([r01 * np.cos(2 * np.pi * u[1]), r01 * np.sin(2 * np.pi * u[1]), r23 * np.cos(2 * np.pi * u[3])], axis=-1)


def thrust_box(cfg):
    txy = cfg.max_thrust * np.sin(cfg.max_tilt_angle)
    return np.array([-txy, -txy, cfg.min_thrust]), np.array([txy, txy, cfg.max_thrust])


def samples(U, q, g, S, sigma, seed, cfg, dtype=np.float64):
    """T_s of problem q at iteration g: U (N, 3) -> (S, N, 3); also returns the (4, S, N) words and (S, N, 3) normals."""
    N = U.shape[0]
    s = np.arange(S, dtype=np.uint64)[:, None]
    k = np.arange(N, dtype=np.uint64)[None, :]
    x = raw_words(q, s, g, k, seed)                                   # (4, S, N)
    n = normals(x, dtype)                                             # (S, N, 3)
    sig = np.where(np.arange(S) == 0, 0.0, sigma)[:, None, None]
    lo, hi = thrust_box(cfg)
    return np.clip(U[None] + sig * n, lo, hi), x, n


def cost(p0, v0, goal, T, cfg, spheres=None, obstacle_weight=0.0):
    c = orc.rollout_cost(p0, v0, goal, T, cfg)
    if spheres is not None and len(spheres):
        c = c + orc.obstacle_penalty_grad(p0, v0, T, spheres, cfg, obstacle_weight)[0]
    return c


def mppi(p0, v0, goal, U, q, S, iters, sigma, temperature, seed, cfg, iter_base=0, spheres=None, obstacle_weight=0.0, dtype=np.float64):
    """One problem: -> (U (N, 3), cost at U, trace (iters,))."""
    U = np.asarray(U, float).copy()
    lo, hi = thrust_box(cfg)
    trace = []
    for i in range(iters):
        T, _, _ = samples(U, q, iter_base + i, S, sigma, seed, cfg, dtype)
        c = cost(p0, v0, goal, T, cfg, spheres, obstacle_weight)
        m = np.min(c)
        w = np.exp(-(c - m) / temperature)
        U = np.clip(np.einsum("s,sna->na", w, T) / np.sum(w), lo, hi)
        trace.append(m)
    return U, float(cost(p0, v0, goal, U, cfg, spheres, obstacle_weight)), np.array(trace)
