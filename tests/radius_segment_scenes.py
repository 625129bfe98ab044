"""Compositions of the segmented radius filter tests (test_radius_segments_ref.py on the CPU,
test_gpu_radius_filter_segments.py on the GPU).  A composition is a dict: name, pts ([n_cap, 4]
float32), starts (nseg + 1 row indices, starts[-1] <= n_cap), lower, upper, radius, mins (the
first is the one at which the answer is mixed), plus scene-specific keys.  All seeded."""
import numpy as np

import radius_scenes as S
from radius_segments_ref import plan_sparse_py

EDGE_LENGTHS = [0, 1, 63, 0, 65, 255, 1025, 0]
# a box whose dense plan is halved (303 x 303 x 59 cells at r 0.05 exceed 2^22)
LADDER_BOX = ((-7.6, -7.6, -1.5), (7.6, 7.6, 1.5))


def _comp(name, pts, starts, lower, upper, radius, mins, **kw):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    return dict(name=name, pts=pts, starts=np.asarray(starts, np.uint32),
                lower=tuple(float(v) for v in lower), upper=tuple(float(v) for v in upper),
                radius=float(np.float32(radius)), mins=list(mins), **kw)


def one_segment(name):
    """A scene of radius_scenes as one segment."""
    s = S.get(name)
    return _comp("one_" + name, s["pts"], [0, len(s["pts"])], s["lower"], s["upper"], s["radius"],
                 s["mins"])


def twin():
    """wave_n257 twice: in the flattened array every point has its coincident twin as a
    neighbour, per segment it has not."""
    s = S.get("wave_n257_h1")
    n = len(s["pts"])
    return _comp("twin", np.concatenate([s["pts"], s["pts"]]), [0, n, 2 * n], s["lower"], s["upper"],
                 s["radius"], [1, 4, 0])


def edges():
    """One cloud cut into segments of 0, 1, 63, 0, 65, 255, 1025 and 0 rows; behind start[nseg]
    NaN rows and copies of the cloud's last 256 rows (read, they would be neighbours)."""
    n = sum(EDGE_LENGTHS)
    s = S.wave_scene(n, seed=3)
    tail = np.concatenate([np.full((24, 4), np.nan, np.float32), s["pts"][n - 256:]])
    starts = np.concatenate([[0], np.cumsum(EDGE_LENGTHS)])
    return _comp("edges", np.concatenate([s["pts"], tail]), starts, s["lower"], s["upper"],
                 s["radius"], [1, 2, 0])


def many_segments(nseg):
    """nseg segments of 1, 2 or 3 rows, every segment at the same place: a row of points 0.08
    apart at r 0.1 (min 1 drops the lone points, min 2 keeps the middle of three only)."""
    rng = np.random.default_rng(100 + nseg)
    row = np.array([[0.0, 0.0, 0.0], [0.08, 0.0, 0.0], [0.16, 0.0, 0.0]], np.float32)
    lengths = 1 + np.arange(nseg) % 3
    xyz = np.concatenate([row[:k] for k in lengths])
    pts = np.concatenate([xyz, rng.uniform(-5, 5, (len(xyz), 1)).astype(np.float32)], axis=1)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    return _comp(f"many_{nseg}", pts, starts, (-1, -1, -1), (1, 1, 1), 0.1, [1, 2, 0], lengths=lengths)


def ladder_in_box(radius, lower, upper, pairs=1024, seed=6):
    """The threshold ladder as radius_scenes.ladder_scene builds it (isolated pairs, the base
    within 2 ulp of a cell face on either side, the partner across the face at a d2 of r2's
    predecessor, r2 or r2's successor), placed against the faces of the SPARSE plan of the box."""
    rng = np.random.default_rng(seed)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    cells, edge = plan_sparse_py(lower, upper, r)
    site = 4
    per = [(c - 4) // site for c in cells]
    assert per[0] * per[1] * per[2] >= pairs
    ids = rng.permutation(per[0] * per[1] * per[2])[:pairs]
    cell = np.stack([ids % per[0], ids // per[0] % per[1], ids // per[0] // per[1]], axis=1) * site + 2
    kind = np.arange(pairs) % 4
    axis = np.where(kind < 3, kind, np.arange(pairs) // 4 % 3)
    ulps = (np.arange(pairs) // 12 % 5) - 2
    cls = np.arange(pairs) // 4 % 3
    lo32 = np.asarray(lower, np.float32).astype(np.float64)
    face = (lo32[None, :] + cell * np.asarray(edge)[None, :]).astype(np.float32)
    mid = lo32[None, :] + (cell + rng.uniform(0.3, 0.7, (pairs, 3))) * np.asarray(edge)[None, :]
    base = mid.astype(np.float32)
    for a in range(3):
        on = (axis == a) | (kind == 3)
        base[on, a] = S._unord(S._ord(face[on, a]) + ulps[on])
    away = np.where(ulps >= 0, -1, 1)
    target = np.where(cls == 0, np.nextafter(r2, np.float32(0)),
                      np.where(cls == 1, r2, np.nextafter(r2, np.float32(np.inf)))).astype(np.float32)
    partner = base.copy()
    todo = np.ones(pairs, bool)

    def search(d2_of, lo_k, hi_k):
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
        p[ar, az] = base[t, az] + rng.uniform(-2e-2, 2e-2, len(t)).astype(np.float32) * r
        p[ar, ay] = base[t, ay] + rng.uniform(2e-3, 4e-3, len(t)).astype(np.float32) * r
        c0 = S._ord(base[t, ax] + away[t].astype(np.float32) * r)
        y0 = S._ord(p[ar, ay])

        def at_x(k):
            p[ar, ax] = S._unord(c0 + away[t] * k)
            return S._d2(base[t], p) >= target[t]

        def at_y(k):
            p[ar, ay] = S._unord(y0 + k)
            return S._d2(base[t], p) >= target[t]

        k = search(at_x, np.full(len(t), -(1 << 16)), np.full(len(t), 1 << 16))
        at_x(k)
        exact = S._d2(base[t], p) == target[t]
        at_x(np.where(exact, k, k - 1))
        k2 = search(at_y, np.zeros(len(t), np.int64), np.full(len(t), 1 << 20))
        at_y(k2)
        hit = S._d2(base[t], p) == target[t]
        partner[t[hit]] = p[hit]
        todo[t[hit]] = False
    assert not todo.any(), "ladder: a pair's distance could not be placed"
    assert (S._d2(base, partner) == target).all() and (S._d2(partner, base) == target).all()
    xyz = np.empty((2 * pairs, 3), np.float32)
    order = rng.permutation(2 * pairs)
    xyz[order[:pairs]] = base
    xyz[order[pairs:]] = partner
    w = rng.uniform(-5, 5, (2 * pairs, 1)).astype(np.float32)
    return dict(pts=np.concatenate([xyz, w], axis=1), base_idx=order[:pairs],
                partner_idx=order[pairs:], cls=cls, base_side=ulps, kind=kind, cells=cells)


def ladder():
    """Three segments: the ladder's base points alone, the ladder, its partners alone.  Alone every
    point is isolated; flattened, each would find its coincident copy."""
    lower, upper = LADDER_BOX
    L = ladder_in_box(0.05, lower, upper)
    pts, n = L["pts"], len(L["pts"])
    first, last = pts[L["base_idx"]], pts[L["partner_idx"]]
    starts = [0, len(first), len(first) + n, len(first) + n + len(last)]
    return _comp("ladder", np.concatenate([first, pts, last]), starts, lower, upper, 0.05, [1],
                 ladder=L, middle=(starts[1], starts[2]))


def lattice():
    """8191 points, one per cell: a 32 x 16 x 16 lattice at 1.5 r spacing; in the rows of even j
    every second point along x stands 0.55 r nearer to its predecessor (0.95 r: a neighbour in the
    next cell).  One segment: 8191 distinct keys in a table of 16384 slots."""
    r = 0.1
    i, j, k = np.meshgrid(np.arange(32), np.arange(16), np.arange(16), indexing="ij")
    x = (0.5 + 1.5 * i - 0.55 * ((i % 2 == 1) & (j % 2 == 0))) * r
    xyz = np.stack([x, (0.5 + 1.5 * j) * r, (0.5 + 1.5 * k) * r], axis=-1).reshape(-1, 3)[:8191]
    rng = np.random.default_rng(8191)
    xyz = xyz[rng.permutation(8191)]
    pts = np.concatenate([xyz, rng.uniform(-5, 5, (8191, 1))], axis=1).astype(np.float32)
    return _comp("lattice", pts, [0, 8191], (0, 0, 0), (48.1 * r, 24.05 * r, 24.05 * r), r, [1, 0])


def crowded():
    """micro_n3 (same box and radius) as a first segment, then `crowded`: 3000 points in one cell."""
    a, b = S.get("micro_n3"), S.get("crowded")
    assert (a["lower"], a["upper"], a["radius"]) == (b["lower"], b["upper"], b["radius"])
    na, nb = len(a["pts"]), len(b["pts"])
    return _comp("crowded2", np.concatenate([a["pts"], b["pts"]]), [0, na, na + nb], b["lower"],
                 b["upper"], b["radius"], [2999, 3000, 2], cluster=b["cluster"])


def reuse_wave():
    """wave_n4097_h3 (another box and radius) cut in two."""
    s = S.get("wave_n4097_h3")
    return _comp("reuse_wave", s["pts"], [0, 1500, 4097], s["lower"], s["upper"], s["radius"], [2])


BUILDERS = {"twin": twin, "edges": edges, "many_16": lambda: many_segments(16),
            "many_64": lambda: many_segments(64), "ladder": ladder, "lattice": lattice,
            "crowded2": crowded, "reuse_wave": reuse_wave}
NAMES = list(BUILDERS)
REUSE_NAMES = ["lattice", "many_16", "reuse_wave", "twin"]   # sizes 8191, 31, 4097, 514

_built = {}


def get(name):
    """A composition by name, built on first use."""
    if name not in _built:
        _built[name] = one_segment(name[4:]) if name.startswith("one_") else BUILDERS[name]()
    return _built[name]
