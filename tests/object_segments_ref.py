"""The segmented partition and the segmented voxel table (include/gdf_segment.h, "the object layer
per segment") in numpy, each in two forms: vectorised and a plain Python loop.

Segments: seg_start[nseg + 1], made non-decreasing and clamped to n_cap on read; row i lies in
segment s iff start'[s] <= i < start'[s + 1]; a row in no segment is neither read nor written.
The *_by_slices forms state the defining properties: a segment's part of the result is the
unsegmented rule (tests/object_points_ref.py, tests/voxel_table_ref.py) on its rows alone, shifted."""
import numpy as np

import object_points_ref as opr
import voxel_table_ref as vtr

NONE = 0xFFFFFFFF
GROUP_KEYS = ("points", "index", "obj_start", "seg_out_start")
TABLE_KEYS = ("vox_cells", "vox_counts", "point_voxel", "vox_seg_start")


def clamp_starts(seg_start, n_cap: int) -> np.ndarray:
    """start'[s] = min(max(seg_start[0..s]), n_cap)"""
    st = np.asarray(seg_start, np.uint32).astype(np.int64)
    return np.minimum(np.maximum.accumulate(st), int(n_cap))


def clamp_starts_loop(seg_start, n_cap: int) -> list:
    out, m = [], 0
    for v in (int(x) for x in np.asarray(seg_start, np.uint32)):
        m = max(m, v)
        out.append(min(m, int(n_cap)))
    return out


def row_segments(st, n: int) -> np.ndarray:
    """The segment of rows 0..n-1, -1 for a row in no segment (st: clamped starts)."""
    st = np.asarray(st, np.int64)
    i = np.arange(n, dtype=np.int64)
    s = np.searchsorted(st, i, side="right") - 1       # the last s with st[s] <= i
    s[(s < 0) | (i >= st[-1])] = -1
    return s


# ---- the partition ------------------------------------------------------------------------------------
def group(points, ids, seg_start, nobj: int, keep=None) -> dict:
    ids = np.asarray(ids, np.uint32)
    n_cap, nseg = len(ids), len(seg_start) - 1
    st = clamp_starts(seg_start, n_cap)
    s = row_segments(st, n_cap)
    kept = (s >= 0) & (ids < nobj)
    if keep is not None:
        kept &= np.asarray(keep, np.uint8)[np.minimum(ids, nobj - 1)] != 0
    keys = np.full(n_cap, NONE, np.uint32)
    keys[kept] = (s[kept] * nobj + ids[kept]).astype(np.uint32)
    r = opr.group(points, keys, nseg * nobj, None)
    r.update(nobj=int(nobj), nseg=nseg, n=int(st[-1]),
             seg_out_start=r["obj_start"][::nobj][:nseg + 1].copy())
    return r


def group_loop(points, ids, seg_start, nobj: int, keep=None) -> dict:
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    ids = [int(x) for x in np.asarray(ids, np.uint32)]
    nseg = len(seg_start) - 1
    st = clamp_starts_loop(seg_start, len(ids))
    index, starts, seg_out = [], [0], [0]
    for s in range(nseg):
        buckets = [[] for _ in range(nobj)]
        for i in range(st[s], st[s + 1]):
            o = ids[i]
            if o < nobj and (keep is None or keep[o]):
                buckets[o].append(i)
        for b in buckets:
            index += b
            starts.append(len(index))
        seg_out.append(len(index))
    idx = np.array(index, np.int64)
    return {"nobj": int(nobj), "nseg": nseg, "n": st[-1], "total": len(index), "points": pts[idx].copy(),
            "index": idx.astype(np.uint32), "obj_start": np.array(starts, np.uint32),
            "seg_out_start": np.array(seg_out, np.uint32)}


def group_by_slices(points, ids, seg_start, nobj: int, keep=None, slice_rule=opr.group) -> dict:
    """The defining property: every segment through the unsegmented rule (slice_rule(points, ids,
    nobj, keep) -> dict) on its rows alone, index shifted by start'[s], obj_start by seg_out_start[s]."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    ids = np.asarray(ids, np.uint32)
    nseg = len(seg_start) - 1
    st = clamp_starts(seg_start, len(ids))
    P, I, starts, seg_out = [np.zeros((0, 4), np.float32)], [np.zeros(0, np.uint32)], [np.zeros(1, np.uint32)], [0]
    for s in range(nseg):
        a, b = int(st[s]), int(st[s + 1])
        r = slice_rule(pts[a:b], ids[a:b], nobj, keep)
        P.append(r["points"])
        I.append((r["index"].astype(np.int64) + a).astype(np.uint32))
        starts.append((r["obj_start"][1:].astype(np.int64) + seg_out[-1]).astype(np.uint32))
        seg_out.append(seg_out[-1] + r["total"])
    return {"nobj": int(nobj), "nseg": nseg, "n": int(st[-1]), "total": seg_out[-1],
            "points": np.concatenate(P), "index": np.concatenate(I), "obj_start": np.concatenate(starts),
            "seg_out_start": np.array(seg_out, np.uint32)}


def assert_group_equal(got: dict, want: dict, keys=GROUP_KEYS):
    """Every array bit for bit (u32 views, so NaN payloads and -0.0 count)."""
    for k in ("nobj", "total"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in keys:
        a = np.ascontiguousarray(got[k]).view(np.uint32)
        b = np.ascontiguousarray(want[k]).view(np.uint32)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(a, b), (k, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8])


# ---- the table --------------------------------------------------------------------------------------
def table(cells, seg_start, C: int, fill: int = NONE) -> dict:
    """point_voxel holds n = start'[nseg] rows; a row before the first segment is not written by the
    library: it holds `fill` here."""
    cells = np.asarray(cells, np.uint32).reshape(-1)
    n_cap, nseg = len(cells), len(seg_start) - 1
    st = clamp_starts(seg_start, n_cap)
    n = int(st[-1])
    s = row_segments(st, n)
    inside = (s >= 0) & (cells[:n].astype(np.int64) < int(C))
    comp = s[inside] * int(C) + cells[:n][inside].astype(np.int64)
    vox, inv, cnt = np.unique(comp, return_inverse=True, return_counts=True)
    pv = np.full(n, NONE, np.uint32)
    pv[s < 0] = fill
    pv[inside] = inv.reshape(-1).astype(np.uint32)
    return {"num_voxels": int(vox.size), "n": n, "nseg": nseg, "vox_cells": (vox % int(C)).astype(np.uint32),
            "vox_counts": cnt.astype(np.uint32), "point_voxel": pv,
            "vox_seg_start": np.searchsorted(vox, np.arange(nseg + 1, dtype=np.int64) * int(C)).astype(np.uint32)}


def table_loop(cells, seg_start, C: int, fill: int = NONE) -> dict:
    cs = [int(c) for c in np.asarray(cells, np.uint32).reshape(-1)]
    nseg = len(seg_start) - 1
    st = clamp_starts_loop(seg_start, len(cs))
    vox_cells, counts, seg_first = [], [], [0]
    pv = [fill] * st[0] + [NONE] * (st[-1] - st[0])
    for s in range(nseg):
        marked = sorted({cs[i] for i in range(st[s], st[s + 1]) if cs[i] < C})
        place = {c: len(vox_cells) + g for g, c in enumerate(marked)}
        vox_cells += marked
        counts += [0] * len(marked)
        for i in range(st[s], st[s + 1]):
            if cs[i] < C:
                counts[place[cs[i]]] += 1
                pv[i] = place[cs[i]]
        seg_first.append(len(vox_cells))
    return {"num_voxels": len(vox_cells), "n": st[-1], "nseg": nseg, "vox_cells": np.array(vox_cells, np.uint32),
            "vox_counts": np.array(counts, np.uint32), "point_voxel": np.array(pv, np.uint32),
            "vox_seg_start": np.array(seg_first, np.uint32)}


def table_by_slices(cells, seg_start, C: int, fill: int = NONE, slice_rule=vtr.table) -> dict:
    """The defining property: every segment through the unsegmented rule (slice_rule(cells, C) ->
    dict) on its rows alone, voxel indices shifted by vox_seg_start[s]."""
    cells = np.asarray(cells, np.uint32).reshape(-1)
    nseg = len(seg_start) - 1
    st = clamp_starts(seg_start, len(cells))
    z = np.zeros(0, np.uint32)
    vc, cn, pv, first = [z], [z], [np.full(int(st[0]), fill, np.uint32)], [0]
    for s in range(nseg):
        t = slice_rule(cells[int(st[s]):int(st[s + 1])], C)
        p = t["point_voxel"].copy()
        p[p != NONE] += np.uint32(first[-1])
        vc.append(t["vox_cells"])
        cn.append(t["vox_counts"])
        pv.append(p)
        first.append(first[-1] + t["num_voxels"])
    return {"num_voxels": first[-1], "n": int(st[-1]), "nseg": nseg, "vox_cells": np.concatenate(vc),
            "vox_counts": np.concatenate(cn), "point_voxel": np.concatenate(pv),
            "vox_seg_start": np.array(first, np.uint32)}


def assert_table_equal(got: dict, want: dict, keys=TABLE_KEYS):
    for k in ("num_voxels", "n"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == np.uint32 and a.shape == b.shape, (k, a.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (k, np.flatnonzero(a != b)[:8])


# ---- the stage calls on a batch --------------------------------------------------------------------
def object_points_batch(seg: dict, points, coords, point_start, min_voxels: int = 0) -> dict:
    """gdf_seg_object_points_batch: §12's ids, voxels and keep on all frames' coords, the points
    grouped by (frame, object)."""
    ids = opr.point_ids(seg, coords)
    vox = opr.object_voxels(seg)
    r = group(points, ids, point_start, int(seg["num_objects"]), opr.keep_of(vox, min_voxels))
    r.update(ids=ids, voxels=vox)
    return r


def object_voxels_batch(seg: dict, coords, point_start, vox_rows, min_voxels: int = 0) -> dict:
    """gdf_seg_object_voxels_batch: the segmented table of the batch's coords, the ids of vox_cells,
    the voxelized rows grouped by (frame of the voxel, object) and their weights."""
    L, H, W = np.asarray(seg["labels"]).shape
    t = table(coords, point_start, W * H * L)
    vox_rows = np.ascontiguousarray(vox_rows, np.float32).reshape(-1, 4)
    assert len(vox_rows) == t["num_voxels"], (len(vox_rows), t["num_voxels"])
    r = object_points_batch(seg, vox_rows, t["vox_cells"], t["vox_seg_start"], min_voxels)
    r.pop("n")
    r.update(t)
    r["weights"] = t["vox_counts"][r["index"]]
    return r
