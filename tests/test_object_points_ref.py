"""tests/object_points_ref.py against itself: the vectorised form and the plain loop agree on random
inputs, and a hand-computed case matches literally."""
import numpy as np
import pytest

import object_points_ref as opr

NONE = opr.NONE


def random_seg(rng, L, H, W, max_labels=6):
    """A labelling-shaped dict (not a real segmentation: the rule only reads the tables)."""
    nl = rng.integers(1, max_labels + 1, L)
    labels = np.zeros((L, H, W), np.uint16)
    for z in range(L):
        labels[z] = rng.integers(0, nl[z], (H, W))
    T = int(nl.sum())
    lstart = opr.lstart_of(nl)
    nobj = int(rng.integers(1, T + 1))
    merged = rng.integers(0, nobj, T).astype(np.uint32)
    merged[rng.permutation(T)[:nobj]] = np.arange(nobj)  # every object has a label
    merged[lstart] = 0  # background merges with background only: object 0 is all background
    fg = np.ones(T, bool)
    fg[lstart] = False
    merged[fg & (merged == 0)] = np.uint32(nobj - 1) if nobj > 1 else 0
    stats = rng.integers(0, 50, (T, 5)).astype(np.int32)
    if nobj == 1:
        stats[:, 4] = 0
    return {"labels": labels, "num_labels": nl.astype(np.uint32), "stats": stats, "merged": merged,
            "num_objects": nobj}


@pytest.mark.parametrize("seed", range(8))
def test_vectorised_and_loop_agree(seed):
    rng = np.random.default_rng(seed)
    L, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 9)), int(rng.integers(1, 12))
    seg = random_seg(rng, L, H, W)
    n = int(rng.integers(0, 200))
    cells = rng.integers(0, W * H * L + 3, n).astype(np.uint32)
    if n > 2:
        cells[0], cells[1] = 0xFFFFFFFF, W * H * L
    pts = rng.standard_normal((n, 4)).astype(np.float32)
    for mv in (0, 1, 20, 2**31):
        a = opr.object_points(seg, pts, cells, mv)
        b = opr.object_points_loop(seg, pts, cells, mv)
        opr.assert_equal(a, b)


@pytest.mark.parametrize("seed", range(4))
def test_group_forms_agree(seed):
    rng = np.random.default_rng(100 + seed)
    n, nobj = int(rng.integers(0, 300)), int(rng.integers(1, 40))
    ids = rng.integers(0, nobj + 5, n).astype(np.uint32)
    ids[::7] = NONE
    keep = rng.integers(0, 2, nobj).astype(np.uint8)
    pts = rng.standard_normal((n, 4)).astype(np.float32)
    for k in (None, keep):
        opr.assert_equal(opr.group(pts, ids, nobj, k), opr.group_loop(pts, ids, nobj, k))


def test_hand_computed_case():
    # W = 4, H = 2, L = 2.  Global labels: 0 bg of layer 0, 1, 2, 3 bg of layer 1, 4, 5.
    labels = np.array([[[1, 1, 0, 2],
                        [1, 0, 0, 0]],
                       [[1, 0, 0, 0],
                        [0, 0, 2, 2]]], np.uint16)
    stats = np.array([[0, 0, 4, 2, 4], [0, 0, 2, 2, 3], [3, 0, 1, 1, 1],
                      [0, 0, 4, 2, 5], [0, 0, 1, 1, 1], [2, 1, 2, 1, 2]], np.int32)
    seg = {"labels": labels, "num_labels": np.array([3, 3], np.uint32), "stats": stats,
           "merged": np.array([0, 1, 2, 0, 1, 3], np.uint32), "num_objects": 4}
    # cells x + 4 y + 8 z: object 1, object 2, a background cell, object 3, out of range,
    # object 1 (layer 1), object 3, object 1
    cells = np.array([0, 3, 2, 15, 16, 8, 14, 4], np.uint32)
    pts = np.array([[i, i + 0.5, -i, 1] for i in range(8)], np.float32)
    for f in (opr.object_points, opr.object_points_loop):
        r = f(seg, pts, cells, min_voxels=2)  # object 2 has one voxel: dropped
        assert r["ids"].tolist() == [1, 2, NONE, 3, NONE, 1, 3, 1]
        assert r["voxels"].tolist() == [0, 4, 1, 2]
        assert r["nobj"] == 4 and r["total"] == 5
        assert r["index"].tolist() == [0, 5, 7, 3, 6]
        assert r["obj_start"].tolist() == [0, 0, 3, 3, 5]
        assert r["points"].tolist() == pts[[0, 5, 7, 3, 6]].tolist()
        r0 = f(seg, pts, cells, min_voxels=0)  # every foreground object
        assert r0["ids"].tolist() == r["ids"].tolist()
        assert r0["index"].tolist() == [0, 5, 7, 1, 3, 6]
        assert r0["obj_start"].tolist() == [0, 0, 3, 4, 6]
