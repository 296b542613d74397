"""Oracle of the swarm's shared plans -- TEST INFRASTRUCTURE (the product never imports it): a NumPy restatement of what include/se3mpc.h
says about se3mpc_swarm_intent_* and the table of se3mpc_mppi_closed_loop_swarm_intent_*: a drone's intent is its nominal rolled out from
its state, row k = the position before step k; the mate of rank r (tests/swarm_oracle.py, imported) fills tracked row r of every step.
Written from the header comment, not from the kernel."""
import numpy as np

import swarm_oracle as so
from oracle import se3mpc_oracle as orc


def intent(pos, vel, U, cfg):
    """(B, N, 3) float64: the positions of the rollout of U (B, N, 3) from (pos, vel) (B, 3); row k = the position BEFORE step k."""
    P, _ = orc.rollout(np.asarray(pos, float), np.asarray(vel, float), np.asarray(U, float), cfg)
    return P


def slab(intents, pos, vel, b, M, Kn, mate_radius, dtype):
    """Drone b's slab (N, Kn_eff, 4) of `dtype` from the intents (B, N, 3) as they stand: column r = the intent of the mate of rank r
    (swarm_oracle.ranked on the snapshot (pos, vel)), radius mate_radius."""
    who, _ = so.ranked(pos, vel, b, M)
    who = who[:Kn]
    I = np.asarray(intents)
    N = I.shape[1]
    out = np.empty((N, len(who), 4), dtype)
    for r, a in enumerate(who):
        out[:, r, :3] = I[a]
        out[:, r, 3] = mate_radius
    return out
