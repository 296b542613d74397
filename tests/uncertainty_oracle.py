"""Float64 NumPy restatement of the reference's UncertaintyField (src/dart_planner/neural_scene/uncertainty_field.py, "field.py") -- TEST
INFRASTRUCTURE, pinned to vectors of the reference's own class by tests/test_uncertainty_oracle_golden.py.  Vectorised stamps, ordered point
updates, an iterative labelling whose label is the smallest raster index of a component (the voxel at which the reference's raster scan
discovers it), regions, targets and statistics.  No flood fill: a 6000-voxel grid labels in milliseconds."""
import numpy as np


class Field:
    """scene_bounds (2, 3), resolution -> the two grids of field.py:53-59."""

    def __init__(self, scene_bounds, resolution):
        self.bounds = np.array(scene_bounds, float)
        self.res = float(resolution)
        self.n = np.ceil((self.bounds[1] - self.bounds[0]) / self.res).astype(int)
        self.u = np.ones(self.n)
        self.c = np.zeros(self.n)

    def copy(self):
        o = Field.__new__(Field)
        o.bounds, o.res, o.n, o.u, o.c = self.bounds.copy(), self.res, self.n.copy(), self.u.copy(), self.c.copy()
        return o

    def index(self, p):
        return np.floor((np.asarray(p, float) - self.bounds[0]) / self.res).astype(int)        # field.py:291-295

    def centres(self):
        ax = [(np.arange(self.n[a]) + 0.5) * self.res + self.bounds[0][a] for a in range(3)]   # field.py:297-302
        return np.meshgrid(*ax, indexing="ij")


def stamp_distances(f, p, radius):
    """(window slices, distances of the window's voxel centres to p) of one stamp, field.py:233-251."""
    g = f.index(p)
    rv = int(radius / f.res)
    lo = np.maximum(0, g - rv)
    hi = np.minimum(f.n, g + rv + 1)
    if np.any(hi <= lo):
        return None, np.zeros((0, 0, 0))
    sl = tuple(slice(int(lo[a]), int(hi[a])) for a in range(3))
    X, Y, Z = f.centres()
    dx, dy, dz = X[sl] - p[0], Y[sl] - p[1], Z[sl] - p[2]
    return sl, np.sqrt((dx * dx + dy * dy) + dz * dz)


def stamp(f, p, radius=2.0, factor=0.5):
    p = np.asarray(p, float)
    sl, d = stamp_distances(f, p, radius)
    if sl is None:
        return
    inside = d <= radius
    f.u[sl] = np.where(inside, f.u[sl] * (1.0 - factor), f.u[sl])
    f.c[sl] = np.where(inside, f.c[sl] + 1, f.c[sl])


def update_points(f, positions, uncertainties, weights=None, alpha=0.1):
    if weights is None:
        weights = np.ones(len(positions))
    for p, unc, w in zip(np.asarray(positions, float), uncertainties, weights):                # field.py:107-108: the loop IS the contract
        g = f.index(p)
        if np.all(g >= 0) and np.all(g < f.n):
            t = tuple(g)
            f.u[t] = alpha * unc + (1 - alpha) * f.u[t]
            f.c[t] += w


def query(f, positions):
    out = np.ones(len(positions))
    for b, p in enumerate(np.asarray(positions, float)):
        g = f.index(p)
        if np.all(g >= 0) and np.all(g < f.n):
            out[b] = f.u[tuple(g)]
    return out


def statistics(f, threshold):
    with np.errstate(invalid="ignore"):
        return dict(observed=int(np.sum(f.c > 0)), high=int(np.sum(f.u > threshold)), sum=float(np.sum(f.u)), min=float(np.min(f.u)),
                    max=float(np.max(f.u)))


def label(mask):
    """int32 labels: the smallest raster index of each 6-connected component of mask, -1 outside."""
    mask = np.asarray(mask, bool)
    big = np.iinfo(np.int64).max
    lab = np.where(mask, np.arange(mask.size).reshape(mask.shape), big)
    while True:
        new = lab.copy()
        for ax in range(3):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[ax], b[ax] = slice(1, None), slice(None, -1)
            a, b = tuple(a), tuple(b)
            new[a] = np.minimum(new[a], lab[b])
            new[b] = np.minimum(new[b], lab[a])
        new = np.where(mask, new, big)
        # a shortcut through the label's own voxel: chains halve every sweep
        flat = new.reshape(-1)
        inside = flat != big
        flat[inside] = np.minimum(flat[inside], flat[flat[inside]])
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(mask, lab, -1).astype(np.int32)


def regions(f, threshold, min_volume=1.0, max_regions=None):
    """-> dict(labels, rows (R, 12) sorted as field.py:177 sorts, roots (R,), counts (R,), total): rows = centre 3, min 3, max 3, avg, volume,
    priority.  Only the first max_regions qualifying roots (ascending) are kept, as the device keeps them."""
    with np.errstate(invalid="ignore"):
        mask = f.u > threshold
    lab = label(mask)
    flat = lab.reshape(-1)
    roots, counts = np.unique(flat[flat >= 0], return_counts=True)
    cell = f.res ** 3
    keep = [(int(r), int(c)) for r, c in zip(roots, counts) if c * cell >= min_volume]        # field.py:328
    total = len(keep)
    if max_regions is not None:
        keep = keep[:max_regions]
    rows = []
    for r, c in keep:
        idx = np.argwhere(lab == r)
        lo = (idx.min(axis=0) + 0.5) * f.res + f.bounds[0]
        hi = (idx.max(axis=0) + 0.5) * f.res + f.bounds[0]
        volume = c * cell
        avg = float(np.mean(f.u[lab == r]))
        rows.append(np.concatenate([(lo + hi) / 2, lo, hi, [avg, volume, avg * np.log(1 + volume)]]))
    order = sorted(range(len(keep)), key=lambda s: float(rows[s][11]), reverse=True)           # Python's stable sort, field.py:177
    return dict(labels=lab, rows=np.array([rows[s] for s in order]).reshape(-1, 12), roots=np.array([keep[s][0] for s in order], np.int32),
                counts=np.array([keep[s][1] for s in order], np.int64), total=total)


def targets(rows, num_targets=5, position=None):
    out = []
    for r in rows[:num_targets]:
        t = np.array(r[0:3], float)
        t[2] = max(t[2], 2.0)                                                                  # field.py:211
        out.append(t)
    if position is not None:
        p = np.asarray(position, float)
        out.sort(key=lambda t: float(np.sqrt(((t[0] - p[0]) ** 2 + (t[1] - p[1]) ** 2) + (t[2] - p[2]) ** 2)))
    return np.array(out, float).reshape(-1, 3)
