"""Scenes of the radius outlier filter tests, shared by the CPU tests of the restatement
(test_radius_ref.py) and the GPU tests of the kernels (test_gpu_radius_filter.py).  A scene is a
dict: name, pts ([n, 4] float32, w carried), lower, upper, radius, mins (min_neighbors values),
plus scene-specific keys.  Everything is seeded: the same points on every run and machine."""
import numpy as np

PLAN_EXTREMES = {
    # name: (lower, upper, radius, the plan's cells)
    "radius_over_box": ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), 3.0, (1, 1, 1)),
    "flat_axis": ((-1, -1, 0.25), (1, 1, 0.25), 0.1, (19, 19, 1)),
    "both_caps": ((-1000, -1000, -1000), (1000, 1000, 1000), 0.01, (128, 128, 256)),
}


def plan_py(lower, upper, radius):
    """The cell plan of include/gdf_filter.h restated in Python doubles: (cells, edge)."""
    r = float(np.float32(radius))
    ext = [float(np.float32(u)) - float(np.float32(l)) for l, u in zip(lower, upper)]
    cells = [int(min(max(1, np.floor(e / (r * (1 + 2.0 ** -10)))), 1024)) for e in ext]
    while cells[0] * cells[1] * cells[2] > 2 ** 22:
        m = max(range(3), key=lambda a: (cells[a], -a))
        cells[m] = (cells[m] + 1) // 2
    return tuple(cells), [e / c for e, c in zip(ext, cells)]


def _w(n, rng):
    return rng.uniform(-5, 5, n).astype(np.float32)


def _scene(name, xyz, lower, upper, radius, mins, rng, **kw):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    pts = np.concatenate([xyz, _w(len(xyz), rng)[:, None]], axis=1).astype(np.float32)
    return dict(name=name, pts=pts, lower=tuple(float(v) for v in lower),
                upper=tuple(float(v) for v in upper), radius=float(np.float32(radius)),
                mins=list(mins), **kw)


# ---- micro clouds -------------------------------------------------------------------------------
def micro_scenes():
    rng = np.random.default_rng(11)
    lo, hi, r = (-1, -1, -1), (1, 1, 1), 0.1
    out = []
    for n, xyz in ((0, np.zeros((0, 3))), (1, [[0.2, 0.1, -0.3]]),
                   (2, [[0.2, 0.1, -0.3], [0.25, 0.1, -0.3]]),
                   (3, [[0.0, 0.0, 0.0], [0.08, 0.0, 0.0], [0.16, 0.0, 0.0]])):
        out.append(_scene(f"micro_n{n}", xyz, lo, hi, r, [0, 1, 2, n + 1], rng))
    out.append(_scene("micro_coincident70", np.tile([[0.3, -0.7, 0.9]], (70, 1)), lo, hi, r,
                      [0, 1, 69, 70, 71], rng))
    return out


# ---- threshold ladder ---------------------------------------------------------------------------
def _ord(a):
    """float32 -> int64 keys ordered like the floats (one step = one ulp)."""
    b = np.asarray(a, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, 0x80000000 - (b & 0x7FFFFFFF) - 1, b + 0x80000000 - 1)


def _unord(k):
    k = np.asarray(k, np.int64)
    b = np.where(k >= 0x80000000 - 1, k - 0x80000000 + 1, (0x80000000 - 1 - k) | 0x80000000)
    return b.astype(np.uint32).view(np.float32)


def _d2(a, b):
    dx, dy, dz = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1], a[:, 2] - b[:, 2]
    return (dx * dx + dy * dy) + dz * dz


def ladder_scene(radius, pairs=4096, seed=5):
    """`pairs` isolated pairs.  Each base point sits within 2 ulp of a cell face of the plan (on one
    axis, or on all three: a corner), on either side; its partner lies across that face at a
    computed d2 of exactly r2's predecessor, r2 or r2's successor (cls 0 / 1 / 2)."""
    rng = np.random.default_rng(seed)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    half = float(np.float32(40.5 * float(r)))       # ~80 cells per axis
    lower, upper = (-half,) * 3, (half,) * 3
    cells, edge = plan_py(lower, upper, r)
    site = 4                                         # a pair per 4 x 4 x 4 cells: no pair sees another
    per = (min(cells) - 4) // site
    assert per ** 3 >= pairs
    ids = rng.permutation(per ** 3)[:pairs]
    cell = np.stack([ids % per, ids // per % per, ids // per // per], axis=1) * site + 2
    kind = np.arange(pairs) % 4                      # 0..2: a face of that axis, 3: a corner
    axis = np.where(kind < 3, kind, np.arange(pairs) // 4 % 3)
    ulps = (np.arange(pairs) // 12 % 5) - 2          # -2 .. 2 ulp off the face: both sides
    cls = np.arange(pairs) // 4 % 3
    lo32 = np.float32(lower[0])
    face = (np.float64(lo32) + cell * np.asarray(edge)[None, :]).astype(np.float32)
    mid = (np.float64(lo32) + (cell + rng.uniform(0.3, 0.7, (pairs, 3))) * np.asarray(edge)[None, :])
    base = mid.astype(np.float32)
    for a in range(3):
        on = (axis == a) | (kind == 3)
        base[on, a] = _unord(_ord(face[on, a]) + ulps[on])
    # the partner goes to the other side of the face: below it for a base at or above the face
    away = np.where(ulps >= 0, -1, 1)
    target = np.where(cls == 0, np.nextafter(r2, np.float32(0)),
                      np.where(cls == 1, r2, np.nextafter(r2, np.float32(np.inf)))).astype(np.float32)
    partner = base.copy()
    todo = np.ones(pairs, bool)
    rows = np.arange(pairs)
    def search(d2_of, lo_k, hi_k):                   # smallest k with d2_of(k) >= target (monotone)
        while (lo_k < hi_k).any():
            k = (lo_k + hi_k) // 2
            ge = d2_of(k)
            hi_k = np.where(ge, k, hi_k)
            lo_k = np.where(ge, lo_k, k + 1)
        return lo_k

    for _ in range(100):
        if not todo.any():
            break
        t = np.flatnonzero(todo)
        ar, ax, ay, az = np.arange(len(t)), axis[t], (axis[t] + 1) % 3, (axis[t] + 2) % 3
        p = base[t].copy()
        # small offsets on the other two axes; the second one then tunes the sum ulp by ulp
        p[ar, az] = base[t, az] + rng.uniform(-2e-2, 2e-2, len(t)).astype(np.float32) * r
        p[ar, ay] = base[t, ay] + rng.uniform(2e-3, 4e-3, len(t)).astype(np.float32) * r
        c0 = _ord(base[t, ax] + away[t].astype(np.float32) * r)
        y0 = _ord(p[ar, ay])

        def at_x(k):
            p[ar, ax] = _unord(c0 + away[t] * k)
            return _d2(base[t], p) >= target[t]

        def at_y(k):
            p[ar, ay] = _unord(y0 + k)
            return _d2(base[t], p) >= target[t]

        k = search(at_x, np.full(len(t), -(1 << 16)), np.full(len(t), 1 << 16))
        at_x(k)
        exact = _d2(base[t], p) == target[t]
        at_x(np.where(exact, k, k - 1))              # one step short of the target: y closes the gap
        k2 = search(at_y, np.zeros(len(t), np.int64), np.full(len(t), 1 << 20))
        at_y(k2)
        hit = _d2(base[t], p) == target[t]
        partner[t[hit]] = p[hit]
        todo[t[hit]] = False
    assert not todo.any(), "ladder: a pair's distance could not be placed"
    assert (_d2(base, partner) == target).all() and (_d2(partner, base) == target).all()
    xyz = np.empty((2 * pairs, 3), np.float32)
    order = rng.permutation(2 * pairs)               # bases and partners interleaved at random
    xyz[order[:pairs]] = base
    xyz[order[pairs:]] = partner
    return _scene(f"ladder_r{float(r):.4g}", xyz, lower, upper, r, [1], rng,
                  base_idx=order[:pairs], partner_idx=order[pairs:], cls=cls, rows=rows,
                  base_side=ulps, kind=kind)


def ladder_scenes():
    return [ladder_scene(r) for r in (0.05, np.float32(0.1), 1.0 / 3.0)]


# ---- wave and tile edges ------------------------------------------------------------------------
WAVE_NS = (63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191)

BAD_ROWS = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0],
                     [0, -np.inf, 0], [0, 0, np.inf], [np.nan, np.nan, np.nan],
                     [-np.inf, np.inf, 0]], np.float32)


def wave_scene(n, half=1.0, center=(0.0, 0.0, 0.0), seed=0):
    """n rows: uniform in the box grown by 10 % (about a quarter outside) with 8 NaN / inf rows
    among them; the radius gives about 4 mean neighbours at the inside density."""
    rng = np.random.default_rng(1000 + n + seed)
    c = np.asarray(center, np.float64)
    n_in = int(round(0.75 * (n - 8)))                # a quarter of the finite rows in the shell
    u = rng.uniform(-1.1, 1.1, (8 * n + 64, 3))
    shell = u[np.abs(u).max(axis=1) > 1.0][:n - 8 - n_in]
    u = np.concatenate([rng.uniform(-1, 1, (n_in, 3)), shell, np.zeros((8, 3))])
    assert len(u) == n
    xyz = (c + half * u).astype(np.float32)
    xyz[n - 8:] = BAD_ROWS
    xyz = xyz[rng.permutation(n)]
    density = (n - 8) / (2.2 * half) ** 3
    radius = (4.0 / (4.0 / 3.0 * np.pi * density)) ** (1.0 / 3.0)
    lower, upper = tuple(c - half), tuple(c + half)
    return _scene(f"wave_n{n}_h{half:g}", xyz, lower, upper, radius, [0, 1, 4, n], rng)


def wave_scenes():
    return [wave_scene(n) for n in WAVE_NS]


# ---- crowded cell -------------------------------------------------------------------------------
def crowded_scene():
    """3000 points in a ball of diameter 0.09 < r inside one cell (cell 9 of 19 per axis spans
    +-0.0526 around 0), and 3000 spread points none of which comes within r of the ball."""
    rng = np.random.default_rng(77)
    r = 0.1
    v = rng.normal(size=(3000, 3))
    v *= (0.045 * rng.uniform(0, 1, 3000) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    spread = rng.uniform(-1, 1, (6000, 3))
    spread = spread[np.linalg.norm(spread, axis=1) > 0.3][:3000]
    xyz = np.concatenate([v, spread])[rng.permutation(6000)]
    s = _scene("crowded", xyz, (-1, -1, -1), (1, 1, 1), r, [2999, 3000], rng)
    s["cluster"] = np.linalg.norm(s["pts"][:, :3].astype(np.float64), axis=1) < 0.05
    return s


# ---- plan extremes ------------------------------------------------------------------------------
def extreme_scenes():
    rng = np.random.default_rng(31)
    out = []
    lo, hi, r, _ = PLAN_EXTREMES["radius_over_box"]
    xyz = rng.uniform(-0.6, 0.6, (300, 3))
    xyz[:8] = [[sx * 0.5, sy * 0.5, sz * 0.5] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    out.append(_scene("extreme_radius_over_box", xyz, lo, hi, r, [1, 150, 10 ** 6], rng))
    lo, hi, r, _ = PLAN_EXTREMES["flat_axis"]
    xyz = rng.uniform(-1.05, 1.05, (3000, 3))
    xyz[:, 2] = np.where(rng.uniform(size=3000) < 0.7, 0.25, rng.uniform(0.2, 0.3, 3000))
    xyz[:4] = [[1, 1, 0.25], [1, -1, 0.25], [-1, 1, 0.25], [1, 0.95, 0.25]]   # the clamped last cells
    out.append(_scene("extreme_flat_axis", xyz, lo, hi, r, [1, 4], rng))
    lo, hi, r, _ = PLAN_EXTREMES["both_caps"]
    # clusters of points a few radii wide around corners, faces and interior sites of the 2 km box
    # (f32 steps are 6e-5 m at 1000 m: ~160 steps per radius)
    sites = [(1000, 1000, 1000), (1000, 1000, -1000), (-1000, 1000, 1000), (1000, -250.0, 999.99),
             (999.995, 999.995, 999.995), (0, 0, 0), (15.625, 15.625, 7.8125), (-1000, -1000, -1000),
             (984.375, 984.375, 992.1875), (500.0, 1000, 1000)]
    xyz = np.concatenate([np.asarray(s) + rng.uniform(-0.02, 0.02, (60, 3)) for s in sites])
    xyz[:3] = [[1000, 1000, 1000], [1000, 1000, 1000 - 0.006], [1000 - 0.005, 1000, 1000]]
    out.append(_scene("extreme_both_caps", xyz, lo, hi, r, [1, 3], rng))
    return out


# ---- more than one block of every kernel --------------------------------------------------------
def multiblock_scene():
    rng = np.random.default_rng(65537)
    xyz = rng.uniform((0, 0, 0), (8, 8, 1), (65537, 3))
    return _scene("multiblock_65537", xyz, (0, 0, 0), (8, 8, 1), 0.1, [4], rng)


def reuse_scenes():
    """One engine, in this order: different sizes, boxes and radii."""
    return [wave_scene(8191), micro_scenes()[3], wave_scene(4097, half=3.0, center=(5, -2, 1), seed=9)]


def small_scenes():
    """Every scene of the GPU tests that the brute-force form can take (n <= 8192)."""
    return (micro_scenes() + ladder_scenes() + wave_scenes() + [crowded_scene()] + extreme_scenes() +
            reuse_scenes()[2:])


MICRO_NAMES = ["micro_n0", "micro_n1", "micro_n2", "micro_n3", "micro_coincident70"]
LADDER_NAMES = ["ladder_r0.05", "ladder_r0.1", "ladder_r0.3333"]
WAVE_NAMES = [f"wave_n{n}_h1" for n in WAVE_NS]
EXTREME_NAMES = ["extreme_" + k for k in PLAN_EXTREMES]
REUSE_NAMES = ["wave_n8191_h1", "micro_n3", "wave_n4097_h3"]
SMALL_NAMES = MICRO_NAMES + LADDER_NAMES + WAVE_NAMES + ["crowded"] + EXTREME_NAMES + REUSE_NAMES[2:]

_built = {}


def get(name):
    """A scene by name, built on first use (collection builds nothing)."""
    if not _built:
        for s in small_scenes():
            _built[s["name"]] = s
        assert sorted(_built) == sorted(SMALL_NAMES)
    if name == "multiblock_65537" and name not in _built:
        _built[name] = multiblock_scene()
    return _built[name]
