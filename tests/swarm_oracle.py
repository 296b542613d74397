"""Oracle of the swarm prologue -- TEST INFRASTRUCTURE (the product never imports it): a NumPy restatement of what include/se3mpc.h says
about se3mpc_mppi_closed_loop_swarm_* and se3mpc_swarm_separation_*: the float64 squared distances on the snapshot, eligibility, the
(d2, index) ranking and the mates' table rows c' = pos - (vel * tR0) in the entry point's type.  Written from the header comment, not
from the kernel.  pos, vel: (B, 3) arrays holding values of the entry point's type; drone b belongs to swarm b // M."""
import numpy as np


def d2_row(pos, b, M):
    """(M,) float64: d2_i = dx*dx + dy*dy + dz*dz, summed left to right, of the mates of drone b (its own slot included, as 0)."""
    base = (b // M) * M
    p = np.asarray(pos)[base:base + M].astype(np.float64)
    own = np.asarray(pos)[b].astype(np.float64)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - own[0], p[:, 1] - own[1], p[:, 2] - own[2]
        return (dx * dx + dy * dy) + dz * dz


def eligible_row(pos, vel, b, M):
    """(M,) bool: mates of drone b whose six values are finite; none when the drone's own row is not finite; never the drone itself."""
    base = (b // M) * M
    fin = np.isfinite(np.asarray(pos, np.float64)).all(axis=1) & np.isfinite(np.asarray(vel, np.float64)).all(axis=1)
    ok = fin[base:base + M].copy()
    ok[b - base] = False
    return ok if fin[b] else np.zeros(M, bool)


def ranked(pos, vel, b, M):
    """The eligible mates of drone b as indices into the B drones, ordered by (d2, index), and their d2."""
    base = (b // M) * M
    d2, ok = d2_row(pos, b, M), eligible_row(pos, vel, b, M)
    idx = np.nonzero(ok)[0]
    order = idx[np.lexsort((idx, d2[idx]))]
    return base + order, d2[order]


def neighbours(pos, vel, M, Kn):
    """(B, Kn) int32: the min(Kn, E) chosen mates of every drone in rank order, -1 behind."""
    B = len(pos)
    out = np.full((B, Kn), -1, np.int32)
    for b in range(B):
        who, _ = ranked(pos, vel, b, M)
        n = min(Kn, len(who))
        out[b, :n] = who[:n]
    return out


def cycle_time(sphere_t0, C, substeps, sim_dt, dtype):
    """tR0 = (R)(sphere_t0 + (double)(C * substeps) * sim_dt): the start of cycle C on the table's clock, in the entry point's type."""
    return dtype(np.float64(sphere_t0) + np.float64(C * substeps) * np.float64(sim_dt))


def mate_rows(pos, vel, who, tR0, mate_radius, dtype):
    """The table rows of the mates `who` (rank order): spheres (n, 4) = (c', mate_radius), velocities (n, 3), both of `dtype`;
    c' = pos - (vel * tR0), each operation rounded to `dtype`."""
    p, v = np.asarray(pos)[who].astype(dtype), np.asarray(vel)[who].astype(dtype)
    back = (v * dtype(tR0)).astype(dtype)
    c = (p - back).astype(dtype)
    sph = np.concatenate([c, np.full((len(who), 1), mate_radius, dtype)], axis=1).astype(dtype)
    return sph, v


def separation(pos, vel, M, dtype, running=None):
    """(B,) of `dtype`: min(running, (R)sqrt(min over the eligible mates of d2)); a drone with no eligible mate keeps its value (+inf)."""
    B = len(pos)
    out = np.full(B, np.inf, dtype) if running is None else np.asarray(running, dtype).copy()
    for b in range(B):
        _, d2 = ranked(pos, vel, b, M)
        if len(d2):
            out[b] = np.minimum(out[b], dtype(np.sqrt(d2[0])))
    return out
