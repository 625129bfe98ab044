"""The object-points rule (include/gdf_segment.h) in numpy, in two forms: vectorised
(np.argsort(kind="stable")) and a plain Python loop.  Inputs are a labelling as Segmenter.results()
/ oracle.object_segmentation_front give it (labels [L, H, W], num_labels, stats, merged,
num_objects), the points [n, 4] and one u32 cell index per point."""
import numpy as np

NONE = 0xFFFFFFFF


def lstart_of(num_labels):
    nl = np.asarray(num_labels, np.int64)
    return np.concatenate([[0], np.cumsum(nl)[:-1]]).astype(np.int64)


def point_ids(seg: dict, cells) -> np.ndarray:
    labels = np.asarray(seg["labels"])
    L, H, W = labels.shape
    cells = np.asarray(cells, np.uint32).astype(np.int64)
    lstart = lstart_of(seg["num_labels"])
    merged = np.asarray(seg["merged"], np.uint32)
    ids = np.full(cells.size, NONE, np.uint32)
    inside = cells < W * H * L
    c = cells[inside]
    lab = labels.reshape(-1)[c].astype(np.int64)
    fg = lab != 0
    got = np.full(c.size, NONE, np.uint32)
    got[fg] = merged[lstart[c[fg] // (W * H)] + lab[fg]]
    ids[inside] = got
    return ids


def object_voxels(seg: dict) -> np.ndarray:
    lstart = lstart_of(seg["num_labels"])
    merged = np.asarray(seg["merged"], np.int64)
    area = np.asarray(seg["stats"], np.int64).reshape(-1, 5)[:, 4].copy()
    area[lstart] = 0  # the background label of every layer
    vox = np.zeros(int(seg["num_objects"]), np.int64)
    np.add.at(vox, merged, area)
    return vox.astype(np.uint32)


def keep_of(voxels, min_voxels: int) -> np.ndarray:
    return (np.asarray(voxels, np.int64) >= max(int(min_voxels), 1)).astype(np.uint8)


def group(points, ids, nobj: int, keep=None) -> dict:
    """Step 4 alone: the stable partition of the kept points by id."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    ids = np.asarray(ids, np.uint32)
    kept = ids < nobj
    if keep is not None:
        k = np.asarray(keep, np.uint8)
        kept &= k[np.minimum(ids, nobj - 1)] != 0
    src = np.flatnonzero(kept)
    order = src[np.argsort(ids[src], kind="stable")]
    counts = np.bincount(ids[src].astype(np.int64), minlength=nobj)
    return {"nobj": int(nobj), "total": int(order.size),
            "points": pts[order].copy(), "index": order.astype(np.uint32),
            "obj_start": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)}


def object_points(seg: dict, points, cells, min_voxels: int = 0) -> dict:
    ids = point_ids(seg, cells)
    vox = object_voxels(seg)
    r = group(points, ids, int(seg["num_objects"]), keep_of(vox, min_voxels))
    r["ids"] = ids
    r["voxels"] = vox
    return r


# ---- the same rule as a plain loop -------------------------------------------------------------
def object_points_loop(seg: dict, points, cells, min_voxels: int = 0) -> dict:
    labels = np.asarray(seg["labels"])
    L, H, W = labels.shape
    flat = labels.reshape(-1).tolist()
    nl = [int(x) for x in seg["num_labels"]]
    lstart = [sum(nl[:z]) for z in range(L)]
    merged = [int(x) for x in seg["merged"]]
    nobj = int(seg["num_objects"])
    stats = np.asarray(seg["stats"]).reshape(-1, 5).tolist()
    voxels = [0] * nobj
    for k in range(len(merged)):
        if k not in lstart:
            voxels[merged[k]] += stats[k][4]
    keep = [v >= max(int(min_voxels), 1) for v in voxels]
    ids = []
    for c in [int(x) for x in np.asarray(cells, np.uint32)]:
        if c >= W * H * L or flat[c] == 0:
            ids.append(NONE)
        else:
            ids.append(merged[lstart[c // (W * H)] + flat[c]])
    return dict(group_loop(points, ids, nobj, keep), ids=np.array(ids, np.uint32),
                voxels=np.array(voxels, np.uint32))


def group_loop(points, ids, nobj: int, keep=None) -> dict:
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    buckets = [[] for _ in range(nobj)]
    for i, o in enumerate(int(x) for x in ids):
        if o != NONE and o < nobj and (keep is None or keep[o]):
            buckets[o].append(i)
    index, starts = [], [0]
    for b in buckets:
        index += b
        starts.append(len(index))
    idx = np.array(index, np.int64)
    return {"nobj": int(nobj), "total": len(index), "points": pts[idx].copy(),
            "index": idx.astype(np.uint32), "obj_start": np.array(starts, np.uint32)}


KEYS = ("ids", "voxels", "points", "index", "obj_start")


def assert_equal(got: dict, want: dict, keys=KEYS):
    """Every array bit for bit (u32 views, so NaN payloads and -0.0 count)."""
    assert got["nobj"] == want["nobj"] and got["total"] == want["total"], \
        (got["nobj"], want["nobj"], got["total"], want["total"])
    for k in keys:
        if k not in want:
            continue
        a = np.ascontiguousarray(got[k]).view(np.uint32)
        b = np.ascontiguousarray(want[k]).view(np.uint32)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(a, b), (k, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8])
