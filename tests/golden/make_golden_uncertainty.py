#!/usr/bin/env python3
"""Golden vectors for the UncertaintyField, produced by RUNNING THE REFERENCE'S OWN CLASS in the build container
(/root/reference/src/dart_planner/neural_scene/uncertainty_field.py, loaded by file path: the module needs only NumPy).  Only inputs and what
the class returned go into the files:

* call sequences on fresh fields of 24 x 20 x 12, 19 x 13 x 11 (an origin off the voxel lattice) and 1 x 1 x 1 voxels: stamps
  (``reduce_uncertainty_around_position``) and point updates (``update_uncertainty_field``) in the order given, then
  ``get_uncertainty_at_position`` at a few positions, ``identify_high_uncertainty_regions``, ``get_exploration_targets`` without and with a
  current position and ``get_statistics``; the two grids after the sequence; the voxel lists the class's flood fill returned, as a label grid
  (label = raster index of the voxel the scan started from);
* stamps: overlapping ones with different factors, a centre outside the bounds, a far centre with an empty window, a window clipped at three
  faces, radius < resolution / 2 (``radius_in_voxels == 0``) and centres on a voxel centre with radius 0.5 and 1.0, where the only voxels
  at ``distance == radius`` are axis-aligned neighbours and every operation is exact in binary;
* point updates: 65 and 130 points with up to 9 hits in one voxel, points outside the bounds, with and without weights.

The generator asserts that every stamp keeps every voxel-centre distance exact by construction or at least 1e-9 away from the radius
(np.linalg.norm goes through a BLAS dot whose fusing is not ours to know), that thresholds and min_volume are 1e-9 away from every value
they are compared with, and that region priorities are exactly equal or at least 1e-9 apart.  Writes uncertainty_cases.npz / .json.
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.environ.get("SE3MPC_GOLDEN_OUT", HERE)
REFERENCE = "/root/reference/src/dart_planner/neural_scene/uncertainty_field.py"
sys.path.insert(0, os.path.dirname(HERE))
import uncertainty_oracle as uo  # noqa: E402

MARGIN = 1e-9
GRIDS = {"g24": ([[-6.0, -5.0, 0.0], [6.0, 5.0, 6.0]], 0.5, (24, 20, 12)),
         "g19": ([[-4.7, -3.2, 0.1], [4.6, 3.1, 5.4]], 0.5, (19, 13, 11)),
         "g1": ([[0.0, 0.0, 0.0], [0.4, 0.4, 0.4]], 0.5, (1, 1, 1))}


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_uncertainty_field", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    mod = load_reference()

    class FrozenTime:                                                              # last_updated / the 5 s rule: not part of the fixtures
        @staticmethod
        def time():
            return 1000.0
    mod.time = FrozenTime
    rng = np.random.default_rng(20261019)
    out, meta = {}, {"margin": MARGIN, "sequences": []}
    worst = {"distance": np.inf, "threshold": np.inf, "volume": np.inf, "priority": np.inf, "exact_hits": 0}

    def check_stamp(orc, op):
        """every voxel-centre distance is exact by construction or MARGIN away from the radius"""
        p, r = np.array(op["position"], float), op["radius"]
        _, d = uo.stamp_distances(orc, p, r)
        if d.size == 0:
            return True
        gap = np.abs(d - r)
        if op.get("exact"):
            # centre on a voxel centre of a lattice in quarters, resolution 0.5, radius 0.5 or 1.0: squares, sums and roots are exact
            assert orc.res == 0.5 and np.all(orc.bounds[0] * 4 == np.round(orc.bounds[0] * 4)) and np.all(p * 4 == np.round(p * 4)) and r in (0.5, 1.0)
            on = gap == 0.0
            worst["exact_hits"] += int(on.sum())
            gap = gap[~on]
        if gap.size and gap.min() < MARGIN:
            return False
        if gap.size:
            worst["distance"] = min(worst["distance"], float(gap.min()))
        return True

    def run(tag, grid, ops, threshold=None, min_volume=1.0, queries=(), target_calls=((5, None),)):
        bounds, res, shape = GRIDS[grid]
        ref = mod.UncertaintyField(np.array(bounds, float), res)
        assert tuple(ref.grid_size) == shape, (tag, ref.grid_size)
        orc = uo.Field(bounds, res)
        key = f"s{len(meta['sequences']):02d}_"
        rec_ops = []
        for n, op in enumerate(ops):
            if op["op"] == "stamp":
                assert check_stamp(orc, op), (tag, n, op)
                ref.reduce_uncertainty_around_position(np.array(op["position"], float), op["radius"], op["factor"])
                uo.stamp(orc, op["position"], op["radius"], op["factor"])
                rec_ops.append(dict(op="stamp", position=[float(v) for v in op["position"]], radius=float(op["radius"]), factor=float(op["factor"]),
                                    radius_voxels=int(op["radius"] / res)))
            else:
                pos, unc, w = op["positions"], op["uncertainties"], op.get("weights")
                ref.update_uncertainty_field(pos, unc, w)
                uo.update_points(orc, pos, unc, w)
                out[f"{key}op{n}_positions"], out[f"{key}op{n}_uncertainties"] = pos, unc
                if w is not None:
                    out[f"{key}op{n}_weights"] = w
                idx = np.floor((pos - np.array(bounds[0])) / res).astype(int)
                valid = np.all((idx >= 0) & (idx < np.array(shape)), axis=1)
                _, hits = np.unique(idx[valid], axis=0, return_counts=True)
                rec_ops.append(dict(op="points", n=int(len(pos)), weights=w is not None, outside=int((~valid).sum()), max_hits=int(hits.max())))
        assert np.array_equal(orc.u, ref.uncertainty_grid) and np.array_equal(orc.c, ref.observation_count), tag
        thr = ref.uncertainty_threshold if threshold is None else threshold
        worst["threshold"] = min(worst["threshold"], float(np.min(np.abs(ref.uncertainty_grid - thr))))
        components = []
        fill = ref._flood_fill

        def recording_fill(mask, visited, start):
            voxels = fill(mask, visited, start)
            components.append(list(voxels))
            return voxels
        ref._flood_fill = recording_fill
        regs = ref.identify_high_uncertainty_regions(threshold, min_volume) if threshold is not None else ref.identify_high_uncertainty_regions(min_volume=min_volume)
        ref._flood_fill = fill
        labels = np.full(shape, -1, np.int32)
        for voxels in components:
            root = np.ravel_multi_index(voxels[0], shape)
            for v in voxels:
                labels[v] = root
            assert root == min(np.ravel_multi_index(v, shape) for v in voxels)
            worst["volume"] = min(worst["volume"], abs(len(voxels) * res ** 3 - min_volume))
        rows = np.array([np.concatenate([r.center, r.bounds[0], r.bounds[1], [r.uncertainty_value, r.volume, r.priority]]) for r in regs]).reshape(-1, 12)
        pri = np.sort(rows[:, 11])
        gaps = np.diff(pri)
        if np.any(gaps > 0):
            worst["priority"] = min(worst["priority"], float(gaps[gaps > 0].min()))
        tgt = []
        for t, (num, pos) in enumerate(target_calls):
            got = ref.get_exploration_targets(num, None if pos is None else np.array(pos, float))
            out[f"{key}targets{t}"] = np.array(got, float).reshape(-1, 3)
            tgt.append(dict(num_targets=num, position=pos))
        stats = ref.get_statistics()
        out[key + "u"], out[key + "c"], out[key + "labels"], out[key + "regions"] = ref.uncertainty_grid, ref.observation_count, labels, rows
        if len(queries):
            q = np.array(queries, float)
            out[key + "query_positions"] = q
            out[key + "query"] = np.array([ref.get_uncertainty_at_position(p) for p in q])
        meta["sequences"].append(dict(key=key, tag=tag, grid=grid, bounds=bounds, resolution=res, grid_size=list(shape), ops=rec_ops,
                                      threshold=float(thr), min_volume=float(min_volume), regions=int(len(regs)), components=len(components),
                                      targets=tgt, statistics={k: v for k, v in stats.items()}))
        return ref

    def stamp(position, radius=2.0, factor=0.5, exact=False):
        return dict(op="stamp", position=list(position), radius=radius, factor=factor, exact=exact)

    def random_stamps(grid, n, radii, factors):
        """stamps at random centres, redrawn until every distance keeps the margin"""
        bounds, res, _ = GRIDS[grid]
        orc = uo.Field(bounds, res)
        ops = []
        while len(ops) < n:
            op = stamp(rng.uniform(np.array(bounds[0]) - 0.5, np.array(bounds[1]) + 0.5), float(rng.choice(radii)), float(rng.choice(factors)))
            if check_stamp(orc, op):
                ops.append(op)
        return ops

    def points(grid, n, weights, repeats):
        """n points: `repeats` groups of up to 9 hits in one voxel scattered through the input, points outside the bounds, the rest anywhere"""
        bounds, res, shape = GRIDS[grid]
        lo, hi = np.array(bounds[0]), np.array(bounds[1])
        pos = rng.uniform(lo - 0.4, hi + 0.4, (n, 3))
        slots = rng.permutation(n)
        at = 0
        for g in range(repeats):
            cell = rng.integers(0, shape)
            hits = 9 if g == 0 else int(rng.integers(2, 7))
            for _ in range(hits):
                pos[slots[at]] = lo + (cell + rng.uniform(0.05, 0.95, 3)) * res
                at += 1
        pos[slots[at]] = lo - np.array([3.0, 0.0, 0.0])
        pos[slots[at + 1]] = hi + np.array([0.0, 0.0, 7.5])
        return dict(op="points", positions=pos, uncertainties=rng.uniform(0.0, 1.0, n), weights=rng.uniform(0.2, 3.0, n) if weights else None)

    # A. the mission planner's call sequence: a stamp per replan along a path (radius and factor of global_mission_planner.py), then the
    # special windows; regions, targets and statistics at the class's defaults
    def settled(grid, op):
        """the stamp, its centre nudged until every distance keeps the margin"""
        orc = uo.Field(GRIDS[grid][0], GRIDS[grid][1])
        while not check_stamp(orc, op):
            op = dict(op, position=[v + float(rng.uniform(-0.03, 0.03)) for v in op["position"]])
        return op

    path = [settled("g24", stamp((-4.13 + 0.837 * s, -3.31 + 0.613 * s, 1.29 + 0.217 * s), 3.0, 0.2)) for s in range(10)]
    special = [stamp((-7.3, 0.2, 1.1), 2.5, 0.5),                                  # a centre outside the bounds, the window reaches in
               stamp((40.0, 0.0, 1.0), 2.0, 0.5),                                  # an empty window
               stamp((-5.8, -4.9, 0.2), 2.0, 0.4),                                 # clipped at three faces
               stamp((5.9, 4.8, 5.9), 1.7, 0.6),                                   # ... and at the three opposite ones
               stamp((1.31, 2.12, 3.17), 0.2, 0.5),                                # radius < resolution / 2: radius_in_voxels == 0, a miss
               stamp((1.26, 2.24, 3.26), 0.2, 0.5),                                # ... and a hit of the voxel's own centre
               stamp((0.25, 0.25, 2.25), 1.0, 0.5, exact=True),                    # distance == radius at the six axis neighbours
               stamp((2.75, -1.25, 4.25), 0.5, 0.2, exact=True),
               stamp((-5.75, -4.75, 0.25), 1.0, 0.2, exact=True)]                  # exact and clipped
    special = [op if op["exact"] else settled("g24", op) for op in special]
    run("path_then_special_windows", "g24", path + special, queries=[(0.0, 0.0, 1.0), (-5.99, -4.99, 0.01), (6.0, 0.0, 1.0), (0.0, 0.0, -0.01), (5.99, 4.99, 5.99)],
        target_calls=((5, None), (3, (4.0, 4.0, 3.0)), (5, (-6.0, -5.0, 0.0))))
    # B. many overlapping stamps with different factors: a field in pockets
    for tag, grid, n, radii in (("pockets_g19", "g19", 250, (0.9, 1.3)), ("pockets_g24", "g24", 400, (0.9, 1.3, 1.6))):
        run(tag, grid, random_stamps(grid, n, radii, (0.1, 0.2, 0.5, 0.9)), min_volume=0.3, target_calls=((5, None), (4, (0.0, 0.0, 2.5)), (2, None)))
    run("pockets_g19_low_threshold", "g19", random_stamps("g19", 250, (0.9, 1.3), (0.2, 0.5)), threshold=0.45, min_volume=0.6,
        target_calls=((8, (1.0, -1.0, 0.5)),))
    # C. point updates
    run("points_65_unweighted", "g19", [points("g19", 65, False, 4)], queries=[(0.0, 0.0, 1.0)])
    run("points_130_weighted_after_stamps", "g24", random_stamps("g24", 12, (1.6, 2.1), (0.5, 0.9)) + [points("g24", 130, True, 8), points("g24", 65, False, 3)],
        threshold=0.6, min_volume=0.5, target_calls=((5, None), (5, (0.0, 0.0, 0.0))))
    # D. one voxel
    run("one_voxel", "g1", [settled("g1", stamp((0.2, 0.2, 0.2), 2.0, 0.1)), points("g1", 65, True, 1)], threshold=0.5, min_volume=0.1,
        queries=[(0.1, 0.1, 0.1), (0.6, 0.1, 0.1)], target_calls=((5, None), (5, (1.0, 1.0, 1.0))))
    run("one_voxel_below_min_volume", "g1", [], target_calls=((5, None),))
    run("one_voxel_region", "g1", [], min_volume=0.1, target_calls=((5, None), (1, (3.0, 0.0, 0.0))))

    meta["worst"] = {k: (v if np.isfinite(v) else None) for k, v in worst.items()}
    assert worst["distance"] >= MARGIN and worst["threshold"] >= MARGIN and worst["volume"] >= MARGIN and worst["priority"] >= MARGIN, worst
    assert worst["exact_hits"] >= 12, worst
    assert max(s["regions"] for s in meta["sequences"]) >= 4 and any(s["components"] > s["regions"] for s in meta["sequences"]), [
        (s["regions"], s["components"]) for s in meta["sequences"]]
    assert max(o.get("max_hits", 0) for s in meta["sequences"] if s["grid"] != "g1" for o in s["ops"]) == 9

    np.savez_compressed(os.path.join(OUT_DIR, "uncertainty_cases.npz"), **out)
    with open(os.path.join(OUT_DIR, "uncertainty_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote uncertainty_cases.npz / .json:", len(meta["sequences"]), "sequences; regions", [s["regions"] for s in meta["sequences"]], "components",
          [s["components"] for s in meta["sequences"]], "worst", worst)


if __name__ == "__main__":
    main()
