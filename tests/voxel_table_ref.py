"""The voxel-table rule (include/gdf_segment.h) in numpy, in two forms: vectorised
(np.unique) and a plain Python loop.

Inputs: cells[n] (u32) and the cell count C.  A row with cells[i] >= C is outside: it marks nothing,
counts nowhere and gets point_voxel[i] = NONE.  vox_cells holds the distinct cells below C in
ascending order, point_voxel[i] the place of cells[i] in it, vox_counts[g] the rows of voxel g.
All integers: every comparison is np.array_equal.

object_voxels() restates gdf_seg_object_voxels on top of object_points_ref: the ids of vox_cells,
the voxelized rows grouped by those ids, and the grouped rows' weights."""
import numpy as np

import object_points_ref as opr
import voxel_ref
from spec_sum_model import sequential_sum

NONE = 0xFFFFFFFF
KEYS = ("vox_cells", "vox_counts", "point_voxel")


def table(cells, num_cells: int) -> dict:
    cells = np.asarray(cells, np.uint32).reshape(-1)
    inside = cells.astype(np.uint64) < int(num_cells)
    vox, inv, cnt = np.unique(cells[inside], return_inverse=True, return_counts=True)
    pv = np.full(cells.size, NONE, np.uint32)
    pv[inside] = inv.reshape(-1).astype(np.uint32)
    return {"num_voxels": int(vox.size), "n": int(cells.size), "vox_cells": vox.astype(np.uint32),
            "vox_counts": cnt.astype(np.uint32), "point_voxel": pv}


def table_loop(cells, num_cells: int) -> dict:
    cs = [int(c) for c in np.asarray(cells, np.uint32).reshape(-1)]
    marked = set()
    for c in cs:
        if c < num_cells:
            marked.add(c)
    vox = sorted(marked)
    place = {}
    for g, c in enumerate(vox):
        place[c] = g
    counts = [0] * len(vox)
    pv = []
    for c in cs:
        if c < num_cells:
            counts[place[c]] += 1
            pv.append(place[c])
        else:
            pv.append(NONE)
    return {"num_voxels": len(vox), "n": len(cs), "vox_cells": np.array(vox, np.uint32),
            "vox_counts": np.array(counts, np.uint32), "point_voxel": np.array(pv, np.uint32)}


def assert_equal(got: dict, want: dict, keys=KEYS):
    assert got["num_voxels"] == want["num_voxels"] and got["n"] == want["n"], \
        (got["num_voxels"], want["num_voxels"], got["n"], want["n"])
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == np.uint32 and a.shape == b.shape, (k, a.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (k, np.flatnonzero(a != b)[:8])


def chain_means(points, point_voxel, num_voxels: int, form="vector") -> np.ndarray:
    """Row g: the voxelize's sequential f32 chain (tests/voxel_ref.py) over the points with
    point_voxel == g, in input order; x, y, z divided by float32(count), w the undivided sum.
    form: "vector" (np.cumsum down each group) or "loop" (spec_sum_model.sequential_sum)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    pv = np.asarray(point_voxel, np.uint32)
    order = np.argsort(pv, kind="stable")            # (stable: input order inside a voxel)
    starts = np.searchsorted(pv[order], np.arange(num_voxels + 1, dtype=np.uint32)).astype(np.int64)
    p = pts[order]
    if form == "vector":
        return voxel_ref._means_vector(p, starts)
    rows = np.empty((num_voxels, 4), np.float32)
    with np.errstate(all="ignore"):
        for g in range(num_voxels):
            t = p[starts[g]:starts[g + 1]]
            c = np.float32(len(t))
            s = [sequential_sum(t[:, a]) for a in range(4)]
            rows[g] = (s[0] / c, s[1] / c, s[2] / c, s[3])
    return rows


def object_voxels(seg: dict, coords, vox_rows, min_voxels: int = 0) -> dict:
    """gdf_seg_object_voxels: {table..., ids [G], voxels, points / index / obj_start of the grouped
    voxelized rows, weights}.  seg: a labelling as Segmenter.results() gives it; vox_rows: the
    engine's voxelized rows [G, 4]."""
    L, H, W = np.asarray(seg["labels"]).shape
    t = table(coords, W * H * L)
    vox_rows = np.ascontiguousarray(vox_rows, np.float32).reshape(-1, 4)
    assert len(vox_rows) == t["num_voxels"], (len(vox_rows), t["num_voxels"])
    r = opr.object_points(seg, vox_rows, t["vox_cells"], min_voxels)
    r.update(t)
    r["weights"] = t["vox_counts"][r["index"]]
    return r
