"""CPU restatement of the radius outlier filter (include/gdf_filter.h), written from its rule and
never from the kernels:

  inside     lower[a] <= p[a] <= upper[a] on all three axes (NaN is outside); points outside are
             dropped and are nobody's neighbour
  distance   dx = xi - xj (dy, dz alike), d2 = (dx*dx + dy*dy) + dz*dz, every operation in binary32
  neighbour  d2 <= r2 with r2 = radius * radius in binary32; i is not its own neighbour
  keep       inside and at least min_neighbors neighbours

Two independent forms, both returning (keep flags [n] bool, neighbour counts [n] uint32; 0 for a
point outside): `brute` compares every pair (n <= 8192), `window` sorts the inside points by x and
gives each only the candidates with |dx| <= 1.01 r before the same exact predicate (a neighbour has
dx*dx <= d2 <= r2, so |dx| <= r (1 + 2^-23) < 1.01 r: the window loses none).
"""
import numpy as np

BRUTE_MAX = 8192


def _f32(pts):
    return np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 4))


def r2_of(radius) -> np.float32:
    r = np.float32(radius)
    return np.float32(r * r)


def inside_mask(pts, lower, upper) -> np.ndarray:
    p = _f32(pts)
    lo, hi = np.asarray(lower, np.float32), np.asarray(upper, np.float32)
    with np.errstate(invalid="ignore"):
        return ((p[:, :3] >= lo) & (p[:, :3] <= hi)).all(axis=1)


def _d2(a, b):
    """d2 of every row of a [m, 3] against every row of b [k, 3] (float32 throughout)."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = a[:, None, 0] - b[None, :, 0]
        dy = a[:, None, 1] - b[None, :, 1]
        dz = a[:, None, 2] - b[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def _finish(n, idx, counts_in, min_neighbors):
    counts = np.zeros(n, np.uint32)
    counts[idx] = counts_in
    keep = np.zeros(n, bool)
    keep[idx] = counts_in >= min_neighbors
    return keep, counts


def brute(pts, lower, upper, radius, min_neighbors, chunk=512):
    p = _f32(pts)
    assert len(p) <= BRUTE_MAX, "brute force is for n <= 8192"
    idx = np.flatnonzero(inside_mask(p, lower, upper))
    q = p[idx, :3]
    r2 = r2_of(radius)
    counts = np.zeros(len(q), np.int64)
    for a in range(0, len(q), chunk):
        near = _d2(q[a:a + chunk], q) <= r2
        counts[a:a + chunk] = near.sum(axis=1) - near[np.arange(near.shape[0]),
                                                      np.arange(a, a + near.shape[0])]
    return _finish(len(p), idx, counts, min_neighbors)


def window(pts, lower, upper, radius, min_neighbors, chunk=256):
    p = _f32(pts)
    idx = np.flatnonzero(inside_mask(p, lower, upper))
    order = np.argsort(p[idx, 0], kind="stable")
    idx = idx[order]
    q = p[idx, :3]
    x = q[:, 0].astype(np.float64)
    w = 1.01 * float(np.float32(radius))
    first = np.searchsorted(x, x - w, side="left")
    last = np.searchsorted(x, x + w, side="right")
    r2 = r2_of(radius)
    counts = np.zeros(len(q), np.int64)
    for a in range(0, len(q), chunk):
        b = min(a + chunk, len(q))
        lo, hi = int(first[a]), int(last[b - 1])      # (x is sorted: the rows' windows nest in it)
        cand = np.arange(lo, hi)
        near = _d2(q[a:b], q[lo:hi]) <= r2
        near &= (cand[None, :] >= first[a:b, None]) & (cand[None, :] < last[a:b, None])
        near &= cand[None, :] != np.arange(a, b)[:, None]
        counts[a:b] = near.sum(axis=1)
    return _finish(len(p), idx, counts, min_neighbors)


def reference(pts, lower, upper, radius, min_neighbors):
    """brute up to 8192 points, window above."""
    f = brute if len(_f32(pts)) <= BRUTE_MAX else window
    return f(pts, lower, upper, radius, min_neighbors)


def apply(pts, keep) -> np.ndarray:
    """The filter's output: the kept points in input order, all four words."""
    return _f32(pts)[np.asarray(keep, bool)]
