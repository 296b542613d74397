"""CPU: tests/uncertainty_oracle.py (the NumPy restatement the kernel checks compare against) is pinned to vectors of the reference's own
UncertaintyField (tests/golden/uncertainty_cases.*): grids, counts, labels and region membership exactly, means and priorities to 1e-11
relative (n <= 6000 summands in [0, 1]: any two summation orders differ by less than n * 2^-52, plus an ulp of the logarithm)."""
import numpy as np

import uncertainty_checks as uc
import uncertainty_oracle as uo


def replay(seq, g):
    f = uo.Field(seq["bounds"], seq["resolution"])
    for n, op in enumerate(seq["ops"]):
        if op["op"] == "stamp":
            uo.stamp(f, op["position"], op["radius"], op["factor"])
        else:
            k = f"{seq['key']}op{n}_"
            uo.update_points(f, g[k + "positions"], g[k + "uncertainties"], g.get(k + "weights"))
    return f


def test_oracle_reproduces_the_reference_s_sequences():
    meta, g = uc.golden()
    assert len(meta["sequences"]) >= 9
    for seq in meta["sequences"]:
        key, tag = seq["key"], seq["tag"]
        f = replay(seq, g)
        assert list(f.n) == seq["grid_size"]
        assert uc.same_bytes(f.u, g[key + "u"]) and uc.same_bytes(f.c, g[key + "c"]), tag
        if key + "query" in g:
            assert uc.same_bytes(uo.query(f, g[key + "query_positions"]), g[key + "query"]), tag
        r = uo.regions(f, seq["threshold"], seq["min_volume"])
        assert np.array_equal(r["labels"], g[key + "labels"]), tag                               # membership of every component, kept or not
        assert r["total"] == seq["regions"] and len(np.unique(r["labels"][r["labels"] >= 0])) == seq["components"], tag
        uc.assert_rows(r["rows"], g[key + "regions"], tag)                                       # the reference's order
        for t, call in enumerate(seq["targets"]):
            assert np.array_equal(uo.targets(r["rows"], call["num_targets"], call["position"]), g[f"{key}targets{t}"]), (tag, t)
        st, want = uo.statistics(f, 0.7), seq["statistics"]
        assert (st["observed"], st["high"], st["min"], st["max"]) == (want["observed_voxels"], want["high_uncertainty_voxels"], want["min_uncertainty"],
                                                                     want["max_uncertainty"]), tag
        assert abs(st["sum"] / want["total_voxels"] - want["average_uncertainty"]) <= uc.REL * want["average_uncertainty"], tag


def test_oracle_labels_are_smallest_raster_indices():
    rng = np.random.default_rng(3)
    for shape in ((24, 20, 12), (19, 13, 11), (1, 1, 1)):
        m = rng.random(shape) < 0.5
        lab = uo.label(m)
        assert np.all(lab[~m] == -1)
        flat = lab.reshape(-1)
        for r in np.unique(flat[flat >= 0]):
            assert r == np.flatnonzero(flat == r).min()
        for ax in range(3):                                                                      # neighbours in the mask share a label
            a, b = np.moveaxis(lab, ax, 0)[1:], np.moveaxis(lab, ax, 0)[:-1]
            both = (a >= 0) & (b >= 0)
            assert np.array_equal(a[both], b[both])
    assert uo.label(uc.serpentine((24, 20, 12))).max() == 0
