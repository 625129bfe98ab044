"""The per-object moments rule (include/gdf_segment.h) in two forms: vectorised numpy
(f32 t, u64 sums) and a plain loop over Python ints; and the shape helper (centroid, covariance,
world bounds) in Python floats and ints.  Inputs are the grouped rows [total, 4], obj_start
[nobj + 1] and the grid of computeVoxelCoords: lower[3], cell[3] (f32), gs[3]."""
import numpy as np

S = 256  # GDF_OBJ_SUBDIV
MAX_GRID = 65536
DTYPE = np.dtype([("count", "<u4"), ("outside", "<u4"), ("qmin", "<u4", 3), ("qmax", "<u4", 3),
                  ("sum", "<u8", 3), ("sum2", "<u8", 6)])
SHAPE_DTYPE = np.dtype([("centroid", "<f8", 3), ("cov", "<f8", 6), ("min_world", "<f8", 3),
                        ("max_world", "<f8", 3)])
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx xy xz yy yz zz
assert DTYPE.itemsize == 104 and SHAPE_DTYPE.itemsize == 120


def sums_fit(gs, n_cap: int) -> bool:
    """(256 max gs - 1)^2 n_cap < 2^64: below it no sum of an n_cap-row call can wrap."""
    m = S * max(int(g) for g in gs) - 1
    return m * m * int(n_cap) < 2**64


def measure(points, lower, cell, gs):
    """(measured [n] bool, q [n, 3] u32; q is 0 on an axis that is out of range)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 4)[:, :3]
    lo, cs = np.asarray(lower, np.float32).reshape(3), np.asarray(cell, np.float32).reshape(3)
    g = np.asarray(gs, np.uint32).reshape(3)
    with np.errstate(all="ignore"):
        t = (p - lo) / cs
        assert t.dtype == np.float32
        ok = (np.float32(0) <= t) & (t <= g.astype(np.float32))  # NaN fails both
        scaled = np.where(ok, t * np.float32(S), np.float32(0))   # exact: t <= 65536
        assert scaled.dtype == np.float32
    q = np.minimum(scaled.astype(np.int64), S * g.astype(np.int64) - 1).astype(np.uint32)
    return ok.all(axis=1), q


def empty(nobj: int) -> np.ndarray:
    m = np.zeros(nobj, DTYPE)
    m["qmin"] = 0xFFFFFFFF
    return m


def moments(points, obj_start, lower, cell, gs) -> np.ndarray:
    start = np.asarray(obj_start, np.int64)
    nobj = len(start) - 1
    total = int(start[-1])
    measured, q = measure(np.asarray(points).reshape(-1, 4)[:total], lower, cell, gs)
    obj = np.repeat(np.arange(nobj), np.diff(start))
    assert len(obj) == total
    m = empty(nobj)
    m["outside"] = np.bincount(obj[~measured], minlength=nobj)
    o, q = obj[measured], q[measured].astype(np.uint64)
    m["count"] = np.bincount(o, minlength=nobj)
    for a in range(3):
        np.minimum.at(m["qmin"][:, a], o, q[:, a].astype(np.uint32))
        np.maximum.at(m["qmax"][:, a], o, q[:, a].astype(np.uint32))
        np.add.at(m["sum"][:, a], o, q[:, a])
    for k, (a, b) in enumerate(PAIRS):
        np.add.at(m["sum2"][:, k], o, q[:, a] * q[:, b])
    return m


def moments_loop(points, obj_start, lower, cell, gs) -> np.ndarray:
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    lo = [np.float32(x) for x in lower]
    cs = [np.float32(x) for x in cell]
    g = [int(x) for x in gs]
    start = [int(x) for x in obj_start]
    m = empty(len(start) - 1)
    with np.errstate(all="ignore"):
        for o in range(len(start) - 1):
            count = outside = 0
            qmin, qmax, s1, s2 = [0xFFFFFFFF] * 3, [0] * 3, [0] * 3, [0] * 6
            for j in range(start[o], start[o + 1]):
                t = [(pts[j, a] - lo[a]) / cs[a] for a in range(3)]
                assert all(type(x) is np.float32 for x in t)
                if not all(np.float32(0) <= t[a] and t[a] <= np.float32(g[a]) for a in range(3)):
                    outside += 1
                    continue
                q = [min(int(t[a] * np.float32(S)), S * g[a] - 1) for a in range(3)]
                count += 1
                for a in range(3):
                    qmin[a], qmax[a], s1[a] = min(qmin[a], q[a]), max(qmax[a], q[a]), s1[a] + q[a]
                for k, (a, b) in enumerate(PAIRS):
                    s2[k] += q[a] * q[b]
            assert max(s2) < 2**64
            m[o] = (count, outside, qmin, qmax, np.array(s1, np.uint64), np.array(s2, np.uint64))
    return m


def shapes(m, lower, cell) -> np.ndarray:
    """gdf_obj_shapes_from_moments in Python floats (IEEE doubles) and ints, in the header's order."""
    m = np.asarray(m, DTYPE).reshape(-1)
    out = np.zeros(len(m), SHAPE_DTYPE)
    c = [float(np.float32(x)) / 256.0 for x in cell]
    lo = [float(np.float32(x)) for x in lower]
    for o, r in enumerate(m):
        N = int(r["count"])
        if N == 0:
            for k in SHAPE_DTYPE.names:
                out[o][k] = float("nan")
            continue
        s1 = [int(x) for x in r["sum"]]
        s2 = [int(x) for x in r["sum2"]]
        for a in range(3):
            out[o]["centroid"][a] = lo[a] + c[a] * (float(s1[a]) / float(N) + 0.5)
            out[o]["min_world"][a] = lo[a] + c[a] * float(int(r["qmin"][a]))
            out[o]["max_world"][a] = lo[a] + c[a] * float(int(r["qmax"][a]) + 1)
        for k, (a, b) in enumerate(PAIRS):
            num = N * s2[k] - s1[a] * s1[b]  # exact; float(int) rounds once, to nearest even
            out[o]["cov"][k] = ((float(num) / (float(N) * float(N))) * c[a]) * c[b]
    return out


# ---- a cloud with every edge of the rule in it ------------------------------------------------------
# Grid (7, 5, 3); every face is an exact f32 and (face - lower) / cell is exact.  lower[0] is +0.0,
# so x = -0.0 gives t = -0.0 (measured, q = 0), and one ulp below that face is the smallest negative
# denormal; the lower faces of y and z are not zero, so there an ulp is a step of a normal number.
# One ulp beyond each of the six faces: five of the rows are unmeasured.  The sixth, above the upper
# face of y (1.0), is measured: 1.0 + 2^-23 - (-1.5) lies halfway between 2.5 and 2.5 + 2^-22 and
# rounds to the even 2.5, so t == gs[1] exactly and q clamps; two ulps above it t exceeds gs[1].
GRID = dict(lower=np.array([0.0, -1.5, 2.25], np.float32), cell=np.array([0.25, 0.5, 0.125], np.float32),
            gs=np.array([7, 5, 3], np.uint32))
CLASSES = ("nan", "pos_inf", "neg_inf", "minus_zero", "lower", "upper", "above_x", "below_x",
           "above_y", "above_y_2ulp", "below_y", "above_z", "below_z")


def special_cloud(rng, n: int):
    """n rows on GRID: about one in eight unmeasured; every 8th row is one of CLASSES in turn.
    Returns (points [n, 4] f32, {class: row indices})."""
    lo, cs, gs = GRID["lower"], GRID["cell"], GRID["gs"]
    hi = lo + cs * gs.astype(np.float32)
    assert np.array_equal((hi - lo) / cs, gs.astype(np.float32))
    span = (hi - lo).astype(np.float32)
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = lo + span * rng.uniform(-0.015, 1.0, (n, 3)).astype(np.float32)
    p[:, 3] = rng.standard_normal(n).astype(np.float32)
    rows = {k: [] for k in CLASSES}
    inf = np.float32(np.inf)
    for i in range(3, n, 8):
        k = CLASSES[(i // 8) % len(CLASSES)]
        rows[k].append(i)
        p[i, :3] = lo + span * rng.uniform(0.1, 0.9, 3).astype(np.float32)  # inside, then one edge
        if k == "nan":
            p[i, 0] = np.float32(np.nan)
        elif k == "pos_inf":
            p[i, 1] = inf
        elif k == "neg_inf":
            p[i, 2] = -inf
        elif k == "minus_zero":
            p[i, 0] = np.float32(-0.0)
        elif k == "lower":
            p[i, :3] = lo
        elif k == "upper":
            p[i, :3] = hi
        elif k == "above_x":
            p[i, 0] = np.nextafter(hi[0], inf)
        elif k == "below_x":
            p[i, 0] = np.nextafter(lo[0], -inf)   # the smallest negative denormal
        elif k == "above_y":
            p[i, 1] = np.nextafter(hi[1], inf)
        elif k == "above_y_2ulp":
            p[i, 1] = np.nextafter(np.nextafter(hi[1], inf), inf)
        elif k == "below_y":
            p[i, 1] = np.nextafter(lo[1], -inf)
        elif k == "below_z":
            p[i, 2] = np.nextafter(lo[2], -inf)
        elif k == "above_z":
            p[i, 2] = np.nextafter(hi[2], inf)
    return p, {k: np.array(v, np.int64) for k, v in rows.items()}


def check_special_classes(p, rows):
    """Every class occurs and the rule treats it as the issue states."""
    measured, q = measure(p, GRID["lower"], GRID["cell"], GRID["gs"])
    top = (S * GRID["gs"].astype(np.int64) - 1).astype(np.uint32)
    for k in CLASSES:
        assert len(rows[k]) > 0, k
    for k in ("nan", "pos_inf", "neg_inf", "above_x", "below_x", "above_y_2ulp", "below_y", "above_z",
              "below_z"):
        assert not measured[rows[k]].any(), k
    assert (p[rows["above_y"], 1] > np.float32(1.0)).all()
    assert measured[rows["above_y"]].all() and (q[rows["above_y"], 1] == top[1]).all()
    assert np.signbit(p[rows["minus_zero"], 0]).all()
    assert measured[rows["minus_zero"]].all() and not q[rows["minus_zero"], 0].any()
    assert measured[rows["lower"]].all() and not q[rows["lower"]].any()
    assert measured[rows["upper"]].all() and (q[rows["upper"]] == top).all()
    frac = 1.0 - measured.mean()
    assert 0.05 < frac < 0.25, frac


def assert_equal(got, want):
    """Every record bit for bit, on u32 views."""
    a = np.ascontiguousarray(got, DTYPE).reshape(-1)
    b = np.ascontiguousarray(want, DTYPE).reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    ua, ub = a.view(np.uint32).reshape(-1, 26), b.view(np.uint32).reshape(-1, 26)
    bad = np.flatnonzero((ua != ub).any(axis=1))
    assert bad.size == 0, (bad[:8], a[bad[:2]], b[bad[:2]])
