"""The voxelize rule on the CPU - TEST INFRASTRUCTURE for tests/voxel_lists.py.

A (point, key) list is sorted stably by key; every voxel (maximal group of equal keys) gives one
row, in key order:
  * average: the reference's sequential f32 chain per component over the voxel's points in list
    order (inc/voxelize.h:29-35); x, y, z divided by float32(count), w the undivided sum;
  * corners: the voxel's lower corner (float32(g) * cell_size + lower, 0) per axis, the product
    rounded before the sum (GridMeta::worldCoord; gdf_kernels.hip group_corner).

Two forms of the average: a plain Python loop over spec_sum_model.sequential_sum and a
vectorised one (np.cumsum with dtype float32 down each group: accumulate is sequential).
tests/test_voxel_lists.py proves them equal bit for bit and ties them to the C oracle.
"""
import numpy as np

from spec_sum_model import sequential_sum

f32 = np.float32


class Grid:
    """Voxel grid as the engine derives it (gdf_engine.cpp set_grid): cells per axis
    ceil((upper - lower) / cell_size) in float32."""

    def __init__(self, lower, upper, cell_size):
        self.lo = np.asarray(lower, f32)
        self.hi = np.asarray(upper, f32)
        self.cs = np.asarray(cell_size, f32)
        self.gs = tuple(int(np.ceil((self.hi[a] - self.lo[a]) / self.cs[a])) for a in range(3))
        self.ncells = self.gs[0] * self.gs[1] * self.gs[2]
        self.key_bits = 0 if self.ncells <= 1 else int(self.ncells - 1).bit_length()
        self.mark_words = (self.ncells + 31) // 32

    def corners(self, keys):
        k = np.asarray(keys, np.uint64)
        g = np.stack([k % self.gs[0], (k // self.gs[0]) % self.gs[1],
                      k // (self.gs[0] * self.gs[1])], 1)
        out = np.zeros((len(k), 4), f32)
        prod = (g.astype(f32) * self.cs[None, :]).astype(f32)  # rounded: no FMA
        out[:, :3] = (prod + self.lo[None, :]).astype(f32)
        return out


def _groups(keys):
    """(order, starts): the stable sort of the keys and the group borders in it (starts[G] = n)."""
    keys = np.asarray(keys, np.uint32)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    n = len(sk)
    if n == 0:
        return order, sk, np.zeros(1, np.int64)
    lead = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    return order, sk, np.concatenate([lead, [n]]).astype(np.int64)


def _means_loop(p, starts):
    rows = np.empty((len(starts) - 1, 4), f32)
    for g in range(len(starts) - 1):
        t = p[starts[g]:starts[g + 1]]
        c = f32(len(t))
        s = [sequential_sum(t[:, a]) for a in range(4)]
        with np.errstate(all="ignore"):
            rows[g] = (s[0] / c, s[1] / c, s[2] / c, s[3])
    return rows


def _means_vector(p, starts):
    G = len(starts) - 1
    rows = np.empty((G, 4), f32)
    size = np.diff(starts)
    with np.errstate(all="ignore"):
        one = np.flatnonzero(size == 1)  # 0 + x, then x / 1
        rows[one] = (f32(0.0) + p[starts[:-1][one]]).astype(f32)
        for g in np.flatnonzero(size > 1):
            t = p[starts[g]:starts[g + 1]]
            s = np.cumsum(t, axis=0, dtype=f32)[-1]
            rows[g] = s
            rows[g, :3] = s[:3] / f32(len(t))
    return rows


def voxelize_ref(keys, pts, average=True, grid=None, form="vector"):
    """(distinct_keys, rows) of the list; form: "vector" or "loop" (average only)."""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 4)
    order, sk, starts = _groups(keys)
    distinct = sk[starts[:-1]] if len(sk) else sk
    if not average:
        return distinct, grid.corners(distinct)
    p = pts[order]
    return distinct, (_means_loop if form == "loop" else _means_vector)(p, starts)


def runs_of(keys):
    """The list's maximal runs of equal keys: (run_keys, run_starts), run_starts[R] = n."""
    keys = np.asarray(keys, np.uint32)
    n = len(keys)
    if n == 0:
        return keys.copy(), np.zeros(1, np.uint32)
    lead = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return keys[lead].copy(), np.concatenate([lead, [n]]).astype(np.uint32)


def cut_runs(run_keys, run_starts, cuts):
    """The runs split further at the point positions `cuts` (those inside a run make two adjacent
    runs of one key - legal, and what a compaction produces at its wave-word borders)."""
    run_keys = np.asarray(run_keys, np.uint32)
    run_starts = np.asarray(run_starts, np.uint32)
    n = int(run_starts[-1])
    cuts = np.asarray(cuts, np.int64)
    cuts = cuts[(cuts > 0) & (cuts < n)]
    starts = np.union1d(run_starts[:-1].astype(np.int64), cuts)
    owner = np.searchsorted(run_starts[:-1].astype(np.int64), starts, side="right") - 1
    return run_keys[owner].copy(), np.concatenate([starts, [n]]).astype(np.uint32)


def expand_runs(run_keys, run_starts):
    """The per-point keys of a run list."""
    return np.repeat(np.asarray(run_keys, np.uint32), np.diff(np.asarray(run_starts, np.int64)))


def marks_ref(distinct_keys, words):
    """The occupancy bitmask: bit (key & 31) of word (key >> 5) for every voxel."""
    m = np.zeros(words, np.uint32)
    k = np.asarray(distinct_keys, np.uint32)
    np.bitwise_or.at(m, k >> np.uint32(5), np.uint32(1) << (k & np.uint32(31)))
    return m
