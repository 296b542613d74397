"""The checks of the uncertainty-field kernels (dart_planner_amd/csrc/uncertainty_field.hip), shared by the CPU suite (tests/test_emu_uncertainty.py:
the kernels compiled for the host) and the GPU suite (tests/test_gpu_uncertainty.py).  `h` is a parity_checks.Harness (ops, to_dev, to_host).

Grids and counts are compared bit for bit; labels, region membership, counts and the order of the rows exactly; a region's bounds, centre and
volume exactly (integers through the same three operations); means and priorities to REL = 1e-11: with n <= 6000 summands in [0, 1] two
summation orders differ by less than n * 2^-52 = 1.4e-12, the logarithm adds an ulp."""
import json
import os

import numpy as np

from dart_planner_amd import capi

import uncertainty_oracle as uo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-11
GRIDS = {"g24": ([[-6.0, -5.0, 0.0], [6.0, 5.0, 6.0]], 0.5), "g19": ([[-4.7, -3.2, 0.1], [4.6, 3.1, 5.4]], 0.5), "g1": ([[0.0, 0.0, 0.0], [0.4, 0.4, 0.4]], 0.5)}
_cache = {}


def golden():
    if "golden" not in _cache:
        with open(os.path.join(GOLDEN, "uncertainty_cases.json")) as f:
            meta = json.load(f)
        _cache["golden"] = (meta, dict(np.load(os.path.join(GOLDEN, "uncertainty_cases.npz"))))
    return _cache["golden"]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class DeviceField:
    """The two grids of one field on the harness's backend, with the oracle's Field for shapes."""

    def __init__(self, h, bounds, res, max_regions=64):
        self.h, self.ops = h, h.ops
        self.shape = uo.Field(bounds, res)
        self.n = tuple(int(v) for v in self.shape.n)
        self.u, self.c = h.to_dev(np.zeros(self.n)), h.to_dev(np.zeros(self.n))
        self.desc = self.ops.ufield_desc(self.u, self.c, self.shape.bounds[0], res)
        self.ws = self.ops.ufield_workspace(self.n, max_regions)
        self.max_regions = max_regions
        self.ops.ufield_fill(self.desc)

    def load(self, u, c=None):
        self.u, self.c = self.h.to_dev(np.array(u, float)), self.h.to_dev(np.zeros(self.n) if c is None else np.array(c, float))
        self.desc = self.ops.ufield_desc(self.u, self.c, self.shape.bounds[0], self.shape.res)

    def grids(self):
        return np.array(self.h.to_host(self.u)), np.array(self.h.to_host(self.c))

    def stamps(self, ops):
        """a list of stamp dicts (position, radius, factor) in ONE launch"""
        d = self.h.to_dev
        rv = np.array([int(o["radius"] / self.shape.res) for o in ops], np.int32)
        self.ops.ufield_stamp(self.desc, d(np.array([o["position"] for o in ops], float).reshape(-1, 3)), d(np.array([o["radius"] for o in ops], float)),
                              d(rv), d(np.array([o["factor"] for o in ops], float)))

    def points(self, pos, unc, w=None):
        d = self.h.to_dev
        self.ops.ufield_update_points(self.desc, d(np.array(pos, float)), d(np.array(unc, float)), None if w is None else d(np.array(w, float)), 0.1, self.ws)

    def regions(self, threshold=0.7, min_volume=1.0, max_regions=None, ws=None):
        out = self.ops.ufield_regions(self.desc, threshold, min_volume, self.max_regions if max_regions is None else max_regions,
                                      workspace=self.ws if ws is None else ws)
        host = {k: np.array(self.h.to_host(v)) for k, v in out.items()}
        host["dev"] = out
        return host

    def statistics(self, threshold=0.7):
        out = self.ops.ufield_statistics(self.desc, threshold, workspace=self.ws)
        return np.array(self.h.to_host(out["counts"])), np.array(self.h.to_host(out["values"]))


def assert_rows(got, want, what):
    """region rows (R, 12): centre, min, max and volume exactly, mean and priority to REL"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not len(want):
        return
    exact = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]
    assert np.array_equal(got[:, exact], want[:, exact]), (what, np.max(np.abs(got[:, exact] - want[:, exact])))
    err = np.max(np.abs(got[:, [9, 11]] - want[:, [9, 11]]) / np.maximum(np.abs(want[:, [9, 11]]), 1e-300))
    print(f"{what}: {len(want)} regions, mean / priority relative error {err:.3g}")
    assert err <= REL, (what, err)


def assert_regions(r, want, what, max_regions):
    """a device result against uncertainty_oracle.regions(...)"""
    assert np.array_equal(r["labels"], want["labels"]), (what, int(np.sum(r["labels"] != want["labels"])))
    written = min(want["total"], max_regions)
    assert tuple(r["counts"]) == (written, want["total"]), (what, tuple(r["counts"]), written, want["total"])
    assert np.array_equal(r["roots"][:written], want["roots"]), (what, r["roots"][:written], want["roots"])
    assert_rows(r["regions"][:written], want["rows"], what)


# ------------------------------------------------------------------------------------------------ golden sequences
def apply_ops(field, seq, g):
    """the sequence's operations through the C ABI; consecutive stamps go into one launch"""
    batch = []
    for n, op in enumerate(seq["ops"]):
        if op["op"] == "stamp":
            assert op["radius_voxels"] == int(op["radius"] / seq["resolution"])
            batch.append(op)
            continue
        if batch:
            field.stamps(batch)
            batch = []
        k = f"{seq['key']}op{n}_"
        field.points(g[k + "positions"], g[k + "uncertainties"], g.get(k + "weights"))
    if batch:
        field.stamps(batch)


def check_golden_sequences(h):
    meta, g = golden()
    for seq in meta["sequences"]:
        key, tag = seq["key"], seq["tag"]
        field = DeviceField(h, seq["bounds"], seq["resolution"])
        assert list(field.n) == seq["grid_size"]
        apply_ops(field, seq, g)
        u, c = field.grids()
        assert same_bytes(u, g[key + "u"]), (tag, "uncertainty", int(np.sum(u != g[key + "u"])))
        assert same_bytes(c, g[key + "c"]), (tag, "observation_count", int(np.sum(c != g[key + "c"])))
        if key + "query" in g:
            q = np.array(h.to_host(h.ops.ufield_query(field.desc, h.to_dev(g[key + "query_positions"]))))
            assert same_bytes(q, g[key + "query"]), (tag, q, g[key + "query"])
        r = field.regions(seq["threshold"], seq["min_volume"])
        assert np.array_equal(r["labels"], g[key + "labels"]), (tag, "labels")
        assert tuple(r["counts"]) == (seq["regions"], seq["regions"]), (tag, tuple(r["counts"]), seq["regions"])
        assert_rows(r["regions"][:seq["regions"]], g[key + "regions"], tag)                     # the reference's order
        for t, call in enumerate(seq["targets"]):
            tg, n = h.ops.ufield_targets(r["dev"]["regions"], r["dev"]["counts"], call["num_targets"], call["position"])
            want = g[f"{key}targets{t}"]
            n = int(h.to_host(n)[0])
            assert n == len(want), (tag, t, n, len(want))
            assert np.array_equal(np.array(h.to_host(tg))[:n], want), (tag, "targets", t)
        counts, values = field.statistics(0.7)
        st = seq["statistics"]
        assert (int(counts[0]), int(counts[1])) == (st["observed_voxels"], st["high_uncertainty_voxels"]), (tag, counts, st)
        assert values[1] == st["min_uncertainty"] and values[2] == st["max_uncertainty"], (tag, values, st)
        assert abs(values[0] / st["total_voxels"] - st["average_uncertainty"]) <= REL * st["average_uncertainty"], (tag, values[0] / st["total_voxels"], st)


# ------------------------------------------------------------------------------------------------ labelling on masks built to break a merge
def serpentine(n):
    """one path through the whole grid: k-lines at even (i, j), joined at alternating ends; its smallest raster index (0, 0, 0) is one END"""
    m = np.zeros(n, bool)
    flip_k = False
    for a, i in enumerate(range(0, n[0], 2)):
        js = list(range(0, n[1], 2))
        if a % 2:
            js.reverse()
        for b, j in enumerate(js):
            m[i, j, :] = True
            if b + 1 < len(js):
                m[i, (j + js[b + 1]) // 2, 0 if flip_k else n[2] - 1] = True
                flip_k = not flip_k
        if i + 2 < n[0]:
            m[i + 1, js[-1], 0 if flip_k else n[2] - 1] = True
            flip_k = not flip_k
    return m


def mask_case(name, n, rng):
    m = np.zeros(n, bool)
    if name == "serpentine":
        m = serpentine(n)
    elif name == "comb":
        m[:, 0, :] = True
        m[::2, :, ::2] = True
    elif name == "two_cubes":                                                    # an exact priority tie -> raster order; a larger and a smaller one
        m[1:3, 1:3, 1:3] = True
        m[10:12, 9:11, 5:7] = True
        m[5:8, 5:8, 8:11] = True
        m[14:17, 2:4, 0:2] = True
    elif name == "singles":                                                      # single voxels below min_volume around one region
        m[::3, ::3, ::3] = True
        m[7:12, 7:12, 4:8] = True
    elif name == "borders":                                                      # one region that touches every border
        m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True, True, True
    elif name == "empty":
        pass
    elif name == "full":
        m[:] = True
    elif name == "overflow":                                                     # more regions than max_regions
        m[::2, ::2, ::2] = True
    elif name.startswith("random"):
        m = rng.random(n) < float(name[6:])
    else:
        raise KeyError(name)
    return m


MASKS = ["serpentine", "comb", "two_cubes", "singles", "borders", "empty", "full", "overflow", "random0.3", "random0.5", "random0.7"]


def check_labelling(h, grid, name):
    bounds, res = GRIDS[grid]
    rng = np.random.default_rng(sum(map(ord, grid + name)))
    field = DeviceField(h, bounds, res, max_regions=6 if name == "overflow" else 4096)
    m = mask_case(name, field.n, rng)
    if name == "serpentine":
        lab = uo.label(m)
        assert len(np.unique(lab[lab >= 0])) == 1 and m[0, 0, 0] and np.sum(m) > m.size // 5      # one component, discovered at its end
    flat_u = np.where(m, 0.9 if name == "two_cubes" else rng.uniform(0.71, 1.0, field.n), rng.uniform(0.0, 0.69, field.n))
    field.load(flat_u)
    min_volume = 0.1 if name == "overflow" else 1.0
    ref = field.shape.copy()
    ref.u = flat_u.copy()
    want = uo.regions(ref, 0.7, min_volume, field.max_regions)
    r = field.regions(0.7, min_volume)
    assert_regions(r, want, f"{grid}/{name}", field.max_regions)
    if name == "overflow":
        assert want["total"] > field.max_regions and r["counts"][0] == field.max_regions
        assert sorted(r["roots"][:field.max_regions]) == sorted(np.unique(want["labels"][want["labels"] >= 0])[:field.max_regions])
    if name == "two_cubes":
        assert want["rows"][2][11] == want["rows"][3][11] and want["roots"][2] < want["roots"][3]           # the two 2 x 2 x 2 cubes
    if name == "empty":
        assert tuple(r["counts"]) == (0, 0)
    if name == "full":
        assert tuple(r["counts"]) == (1, 1) and r["roots"][0] == 0 and np.all(r["labels"] == 0)


# ------------------------------------------------------------------------------------------------ properties
def pocket_field(h, grid, seed, n=250, max_regions=64):
    bounds, res = GRIDS[grid]
    rng = np.random.default_rng(seed)
    field = DeviceField(h, bounds, res, max_regions)
    lo, hi = np.array(bounds[0]), np.array(bounds[1])
    ops = [dict(position=rng.uniform(lo - 0.5, hi + 0.5), radius=float(rng.choice((0.9, 1.3))), factor=float(rng.choice((0.1, 0.2, 0.5, 0.9)))) for _ in range(n)]
    field.stamps(ops)
    return field, ops


def check_determinism(h):
    field, _ = pocket_field(h, "g19", 5)
    a, b = field.regions(0.7, 0.3), field.regions(0.7, 0.3)
    assert a["counts"][0] >= 3
    for k in ("labels", "counts", "roots", "regions"):
        n = a["counts"][0] if k in ("roots", "regions") else None
        assert same_bytes(a[k][:n], b[k][:n]), k
    s1, s2 = field.statistics(), field.statistics()
    assert same_bytes(s1[0], s2[0]) and same_bytes(s1[1], s2[1])


def check_batched_stamps_equal_single_launches(h):
    """130 stamps in one launch == 130 launches of one stamp, bit for bit, and == the oracle's sequential loop"""
    one, ops = pocket_field(h, "g24", 11, n=130)
    bounds, res = GRIDS["g24"]
    many = DeviceField(h, bounds, res)
    ref = uo.Field(bounds, res)
    for op in ops:
        many.stamps([op])
        uo.stamp(ref, op["position"], op["radius"], op["factor"])
    (u1, c1), (u2, c2) = one.grids(), many.grids()
    assert same_bytes(u1, u2) and same_bytes(c1, c2)
    assert np.array_equal(c1, ref.c) and np.max(c1) >= 3                                        # counts are integers: exact whatever the norm's rounding
    assert np.max(np.abs(u1 - ref.u)[c1 == ref.c]) == 0.0


def check_point_updates(h, n, weighted):
    """n points with repeated voxels and points outside the bounds against the sequential loop, bit for bit"""
    bounds, res = GRIDS["g19"]
    rng = np.random.default_rng(100 + n + weighted)
    field, _ = pocket_field(h, "g19", 3, n=20)
    ref = field.shape.copy()
    ref.u, ref.c = field.grids()
    lo, hi = np.array(bounds[0]), np.array(bounds[1])
    pos = rng.uniform(lo - 0.4, hi + 0.4, (n, 3))
    pos[rng.permutation(n)[:9]] = lo + (np.array([7, 5, 3]) + rng.uniform(0.05, 0.95, (9, 3))) * res       # 9 hits in one voxel
    pos[rng.permutation(n)[:5]] = lo + (np.array([18, 12, 10]) + rng.uniform(0.05, 0.95, (5, 3))) * res    # the last voxel
    unc, w = rng.uniform(0.0, 1.0, n), rng.uniform(0.2, 3.0, n) if weighted else None
    field.points(pos, unc, w)
    uo.update_points(ref, pos, unc, w)
    u, c = field.grids()
    assert same_bytes(u, ref.u) and same_bytes(c, ref.c), (int(np.sum(u != ref.u)), int(np.sum(c != ref.c)))


def check_dirty_workspace(h):
    """a workspace left dirty by a call with a larger max_regions (and one full of 0x7B bytes) changes nothing"""
    big, _ = pocket_field(h, "g19", 5, max_regions=64)
    assert big.regions(0.7, 0.1)["counts"][0] > 3
    small, _ = pocket_field(h, "g19", 6, max_regions=64)
    want = small.regions(0.7, 0.3, max_regions=3, ws=h.ops.ufield_workspace(small.n, 3))
    got = small.regions(0.7, 0.3, max_regions=3, ws=big.ws)
    poison = h.to_dev(np.frombuffer(b"\x7b" * (4 * int(big.ws.shape[0])), np.int32).copy())
    got2 = small.regions(0.7, 0.3, max_regions=3, ws=poison)
    assert want["counts"][1] > 3 and want["counts"][0] == 3
    for k in ("labels", "counts"):
        assert same_bytes(want[k], got[k]) and same_bytes(want[k], got2[k]), k
    for k in ("roots", "regions"):
        assert same_bytes(want[k][:3], got[k][:3]) and same_bytes(want[k][:3], got2[k][:3]), k
    small.ws = poison
    s1 = small.statistics()
    small.ws = h.ops.ufield_workspace(small.n, 3)
    s2 = small.statistics()
    assert same_bytes(s1[0], s2[0]) and same_bytes(s1[1], s2[1])


def check_nan_voxels(h):
    """NaN uncertainties stay in their voxels and do not enter another region's rows"""
    field, _ = pocket_field(h, "g24", 7, n=60)
    u, c = field.grids()
    rng = np.random.default_rng(9)
    holes = rng.random(u.shape) < 0.05
    u[holes] = np.nan
    field.load(u, c)
    ref = field.shape.copy()
    ref.u, ref.c = u.copy(), c.copy()
    want = uo.regions(ref, 0.7, 0.3, field.max_regions)
    r = field.regions(0.7, 0.3)
    assert_regions(r, want, "nan voxels", field.max_regions)
    assert np.all(r["labels"][holes] == -1) and np.all(np.isfinite(r["regions"][:r["counts"][0]]))
    field.stamps([dict(position=(0.1, 0.2, 3.1), radius=4.3, factor=0.5)])
    u2, _ = field.grids()
    assert np.array_equal(np.isnan(u2), holes)
    counts, values = field.statistics()
    assert np.isnan(values).all() and counts[1] == int(np.sum(u2 > 0.7))


def check_invalid_arguments(h):
    lib, be = h.ops.lib, h.ops.be
    field, _ = pocket_field(h, "g19", 5, n=5)
    d, ws, words, st = field.desc, be.ptr(field.ws), int(field.ws.shape[0]), be.stream()
    NULL, SHAPE, PARAM, WORKSPACE = -1, -3, -4, -5
    buf = h.to_dev(np.zeros(64))
    ints = h.to_dev(np.zeros(64, np.int32))
    p, ip = be.ptr(buf), be.ptr(ints)
    before = field.grids()

    def bad(**kw):
        b = capi.UFieldDesc(uncertainty=d.uncertainty, observation_count=d.observation_count, n=d.n, reserved=0, origin=d.origin, resolution=d.resolution)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    assert lib.ufield_workspace(0, 4, 4, 1) == SHAPE and lib.ufield_workspace(4, 4, 4, 0) == SHAPE and lib.ufield_workspace(2048, 2048, 2048, 1) == SHAPE
    assert lib.ufield_workspace(1 << 22, 1 << 22, 1 << 22, 1) == SHAPE and lib.ufield_workspace(1 << 16, 1 << 16, 1, 1) == SHAPE       # products past 2^63 / 2^31
    assert lib.ufield_workspace(1 << 10, 1 << 10, 1 << 10, 1) > 7 << 30 and lib.ufield_workspace(4, 4, 4, (1 << 30) + 1) == SHAPE
    assert lib.ufield_workspace(1, 1, 1, 1) >= 2048
    assert lib.ufield_status("fill", bad(n=(capi.C.c_int32 * 3)(1 << 22, 1 << 22, 1 << 22)), st) == SHAPE
    assert lib.ufield_status("fill", None, st) == NULL
    assert lib.ufield_status("fill", bad(uncertainty=None), st) == NULL
    assert lib.ufield_status("fill", bad(observation_count=None), st) == NULL
    assert lib.ufield_status("fill", bad(n=(capi.C.c_int32 * 3)(19, 0, 11)), st) == SHAPE
    assert lib.ufield_status("fill", bad(resolution=0.0), st) == PARAM
    assert lib.ufield_status("fill", bad(resolution=float("nan")), st) == PARAM
    assert lib.ufield_status("fill", bad(origin=(capi.C.c_double * 3)(0.0, float("inf"), 0.0)), st) == PARAM
    assert lib.ufield_status("stamp", d, p, p, ip, p, -1, st) == SHAPE
    assert lib.ufield_status("stamp", d, p, p, ip, p, (1 << 31) - 1, st) == SHAPE
    assert lib.ufield_status("stamp", d, None, p, ip, p, 1, st) == NULL
    assert lib.ufield_status("stamp", d, None, None, None, None, 0, st) == 0
    assert lib.ufield_status("update_points", d, p, p, None, -1, 0.1, ip, ws, words, st) == SHAPE
    assert lib.ufield_status("update_points", d, p, p, None, 1, float("nan"), ip, ws, words, st) == PARAM
    assert lib.ufield_status("update_points", d, p, None, None, 1, 0.1, ip, ws, words, st) == NULL
    assert lib.ufield_status("update_points", d, p, p, None, 1, 0.1, ip, None, words, st) == NULL
    assert lib.ufield_status("update_points", d, p, p, None, 1, 0.1, ip, ws, 2 * int(np.prod(field.n)) - 1, st) == WORKSPACE
    assert lib.ufield_status("query", d, p, -1, p, st) == SHAPE and lib.ufield_status("query", d, p, (1 << 30) + 1, p, st) == SHAPE
    assert lib.ufield_status("update_points", d, p, p, None, (1 << 30) + 1, 0.1, ip, ws, words, st) == SHAPE
    assert lib.ufield_status("query", d, p, 1, None, st) == NULL
    assert lib.ufield_status("statistics", d, 0.7, None, p, ws, words, st) == NULL
    assert lib.ufield_status("statistics", d, 0.7, ip, p, ws, 2047, st) == WORKSPACE
    assert lib.ufield_status("statistics", d, 0.7, ip, p, ws + 4, words - 1, st) == WORKSPACE            # not 8-byte aligned
    labels = be.ptr(h.to_dev(np.zeros(field.n, np.int32)))
    assert lib.ufield_status("regions", d, 0.7, 1.0, 0, labels, p, None, ip, ws, words, st) == SHAPE
    assert lib.ufield_status("regions", d, 0.7, 1.0, 4, None, p, None, ip, ws, words, st) == NULL
    assert lib.ufield_status("regions", d, 0.7, 1.0, 4, labels, p, None, ip, None, words, st) == NULL
    assert lib.ufield_status("regions", d, 0.7, 1.0, 4, labels, p, None, ip, ws, lib.ufield_workspace(*field.n, 4) - 1, st) == WORKSPACE
    assert lib.ufield_targets_status(p, ip, -1, None, p, ip, st) == SHAPE
    assert lib.ufield_targets_status(p, ip, 1025, None, p, ip, st) == SHAPE
    assert lib.ufield_targets_status(None, ip, 1, None, p, ip, st) == NULL
    after = field.grids()
    assert same_bytes(before[0], after[0]) and same_bytes(before[1], after[1])                       # a refused call launches nothing


def check_behaviour(h):
    """the mirror class along a short path with a wall behind it: coverage rises, no exploration target lies inside the stamped tube, targets
    honour the 2 m floor and the distance order"""
    from dart_planner_amd.neural_scene import UncertaintyField
    bounds, res = np.array([[-6.0, -5.0, 0.0], [6.0, 5.0, 3.0]]), 0.5
    f = UncertaintyField(bounds, res, ops=h.ops, max_regions=64, clock=lambda: 0.0)
    assert list(f.grid_size) == [24, 20, 6] and f.get_statistics()["observation_coverage"] == 0.0
    path = [(np.array([-5.0, -4.0 + s, 1.5]), 2.0) for s in range(9)]                            # along the x = -6 face
    wall = [(np.array([2.0, -5.0 + s, 1.5]), 1.6) for s in range(11)]                            # cuts the rest in two
    coverage = []
    for p, r in path:
        f.reduce_uncertainty_around_position(p, radius=r, reduction_factor=0.5)
        coverage.append(f.get_statistics()["observation_coverage"])
    assert all(b > a for a, b in zip(coverage, coverage[1:])) and 0.0 < coverage[-1] < 1.0
    f.reduce_uncertainty_around_positions(np.array([p for p, _ in wall]), 1.6, 0.5)
    assert f.get_uncertainty_at_position(path[3][0]) < 0.7 and f.get_uncertainty_at_position(np.array([100.0, 0.0, 0.0])) == 1.0
    both = f.get_uncertainty_at_positions(np.array([path[3][0], [5.5, 4.5, 2.5]]))
    assert both[0] < 0.7 and both[1] == 1.0
    here = np.array([5.0, 4.0, 1.5])
    by_priority = f.get_exploration_targets(5)
    targets = f.get_exploration_targets(5, here)
    regions = f.high_uncertainty_regions
    assert len(regions) == 2 and len(targets) == 2 and regions[0].priority > regions[1].priority and regions[0].uncertainty_value > 0.7
    for t in targets:
        assert t[2] == 2.0                                                                       # the regions' centres lie at z = 1.5
        assert f.get_uncertainty_at_position(t) > 0.7 and all(np.linalg.norm(t - p) > r for p, r in path + wall)
    d = [float(np.linalg.norm(t - here)) for t in targets]
    assert d == sorted(d) and np.array_equal(targets[0], by_priority[1]) and np.array_equal(targets[1], by_priority[0])
    batch = UncertaintyField(bounds, res, ops=h.ops, max_regions=64, clock=lambda: 0.0)
    batch.reduce_uncertainty_around_positions(np.array([p for p, _ in path + wall]), np.array([r for _, r in path + wall]), 0.5)
    assert same_bytes(batch.uncertainty_grid, f.uncertainty_grid) and same_bytes(batch.observation_count, f.observation_count)
    box = np.array([[-2.0, -2.0, 1.0], [1.0, 1.0, 3.0]])
    lo, hi = np.floor((box - bounds[0]) / res).astype(int)
    assert np.array_equal(f.get_uncertainty_field_region(box), f.uncertainty_grid[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1])
