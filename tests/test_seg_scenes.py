"""The scenes of tests/seg_scenes.py hold the cases they were built for (no GPU): every scene is
built, the C oracle's result equals the Python restatement's (seg_ref.front_end), and the scene's
content assertion - a condition on the input or on the scan's census - holds.  The GPU tests
(test_gpu_segment_shapes.py) run exactly these scenes; a scene that lost its case would leave them
passing and testing nothing.  The whole file takes about 2 s (the sparse 157/158 x 1022 layers of
lds_limit cost the pure-Python restatement 0.2 s each, wide_merge's label matrices 0.4 s)."""
import numpy as np
import pytest
from scipy import ndimage

import seg_ref
import seg_scenes as S
from test_segment_kat import assert_same

EIGHT = np.ones((3, 3))


def parts(mask):
    """(label image, count) of the 8-connected components of a boolean mask (scipy)."""
    return ndimage.label(mask, structure=EIGHT)


@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_equals_python_restatement(name):
    g = S.get(name)
    assert g.dtype == np.uint8 and g.ndim == 3 and g.any()
    assert_same(S.oracle(name), seg_ref.front_end(g))


def test_census_hook_changes_nothing():
    g = S.get("rings_across_step")[0]
    a = seg_ref.external_contours(g)
    b = seg_ref.external_contours(g, census={})
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_tile_diagonals():
    g = S.get("tile_diagonals")
    assert g.shape == (8, 70, 70)
    assert S.oracle("tile_diagonals")["num_labels"].tolist() == [2] * 8
    for z in range(8):
        assert g[z].sum() == 20 and parts(g[z])[1] == 1
        tiles = S.tiles_of(g[z])
        if z in (0, 3):  # dx == dy of direction 0: through the corner itself, a two-tile link
            assert g[z, 31, 31] and g[z, 32, 32] and tiles == {(0, 0), (1, 1)}
        else:
            assert len(tiles) >= 3, z
    # the up-right links of direction 1 cross y = 32 away from the tile's last block column
    for z in range(4, 8):
        (x,) = np.flatnonzero(g[z, 32])
        assert g[z, 31, x + 1] and (x // 2) % 16 != 0 and (x // 2) % 16 != 15


def test_tile_corner_antidiagonals():
    g = S.get("tile_corner_antidiagonals")
    assert S.oracle("tile_corner_antidiagonals")["num_labels"].tolist() == [2] * 4
    assert g[0, 31, 32] and g[0, 32, 31] and S.tiles_of(g[0]) == {(0, 1), (1, 0)}
    for z in range(4):
        assert g[z].sum() == 20 and parts(g[z])[1] == 1
    assert all(len(S.tiles_of(g[z])) == 3 for z in (1, 2))


def test_tile_near_misses():
    g = S.get("tile_near_misses")
    assert g.shape == (1, 70, 70) and g.sum() == 8
    r = S.oracle("tile_near_misses")
    assert r["num_labels"].tolist() == [9] and r["contours_per_layer"].tolist() == [8]
    for a, b in S.NEAR_MISS_PAIRS:
        assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 2
        assert (a[0] // S.TILE, a[1] // S.TILE) != (b[0] // S.TILE, b[1] // S.TILE)


def test_serpentine():
    g = S.get("serpentine")
    assert g.shape == (2, 67, 97) and np.array_equal(g[1], g[0, ::-1])
    r = S.oracle("serpentine")
    assert r["num_labels"].tolist() == [2, 2]
    assert r["contour_sizes"].tolist() == [6594, 6594]
    every = {(ty, tx) for ty in range(3) for tx in range(4)}
    assert S.tiles_of(g[0]) == every and S.tiles_of(g[1]) == every


def test_combs():
    g = S.get("combs")
    assert g.shape == (2, 70, 131)
    assert S.oracle("combs")["num_labels"].tolist() == [2, 2]
    # the tile rows away from the join hold 16 tile-local pieces per (full) tile
    for z, rows in ((0, slice(0, 32)), (1, slice(32, 64))):
        for tx in range(4):
            assert parts(g[z, rows, 32 * tx:32 * tx + 32])[1] >= 16


def test_interlocked_combs():
    g = S.get("interlocked_combs")
    assert g.shape == (1, 40, 131)
    r = S.oracle("interlocked_combs")
    assert r["num_labels"].tolist() == [3]
    lab = r["labels"][0]
    assert lab[0, 0] == 1 and lab[39, 1] == 2
    for y in range(3, 37):  # A, 0, B, 0 along every wave
        assert np.array_equal(lab[y], np.resize([1, 0, 2, 0], 131))


@pytest.mark.parametrize("H,W", S.ROOT_SHAPES)
def test_every_block_a_root(H, W):
    r = S.oracle(f"every_block_a_root_{H}x{W}")
    blocks = S.root_blocks(H, W)
    assert blocks == {(64, 64): 1024, (64, 66): 1056, (1, 2050): 1025, (2, 2049): 1025}[(H, W)]
    assert r["num_labels"].tolist() == [blocks + 1]
    assert np.array_equal(r["labels"][0], S.root_labels(H, W))


@pytest.mark.parametrize("W", S.BAR_WIDTHS)
def test_wave_bars(W):
    g = S.get(f"wave_bars_{W}")
    assert g.shape == (1, 17, W)
    r = S.oracle(f"wave_bars_{W}")
    assert r["num_labels"].tolist() == [3]
    assert (r["labels"][0, 7:9] == 1).all() and (r["labels"][0, 15] == 2).all()
    assert (r["labels"][0, 16, :W // 2] == 2).all() and not r["labels"][0, 16, W // 2:].any()
    stats, cent = S.wave_bars_closed_form(W)
    assert np.array_equal(r["stats"], stats) and np.array_equal(r["centroids"], cent)


def test_rings_across_step():
    g = S.get("rings_across_step")
    assert g.shape == (1, 40, 300)
    r = S.oracle("rings_across_step")
    assert r["num_labels"].tolist() == [8] and r["contours_per_layer"].tolist() == [1]
    c = S.census(g[0])
    assert c["taken"] == 1 and c["skipped"] > 100
    assert c["skipped_lnbd_earlier_step"] >= 100


def test_thick_ring_across_step():
    g = S.get("thick_ring_across_step")
    r = S.oracle("thick_ring_across_step")
    assert r["num_labels"].tolist() == [3] and r["contours_per_layer"].tolist() == [1]
    assert r["labels_to_contours"].tolist() == [-1, 0, -1]
    c = S.census(g[0])
    # the hole's 10 rows: the right wall's start on each, the island's on two of them
    assert c["taken"] == 1 and c["skipped"] == 12
    assert c["skipped_lnbd_run_start_earlier_step"] == 12
    # one-pixel walls never leave the decision to the value cached where the run begins
    assert S.census(S.get("rings_across_step")[0])["skipped_lnbd_run_start_earlier_step"] == 0


@pytest.mark.parametrize("right", [True, False])
def test_mouth_islands(right):
    name = "mouth_islands_right" if right else "mouth_islands_left"
    g = S.get(name)
    assert g.shape == (1, 30, 300)
    r = S.oracle(name)
    assert r["num_labels"].tolist() == [4] and r["contours_per_layer"].tolist() == [3]
    assert (r["labels_to_contours"][1:] >= 0).all()
    c = S.census(g[0])
    assert c["taken"] == 3 and c["start_at_step_edge"][255] >= 1
    if right:
        assert c["taken_lnbd_earlier_step"] >= 1
    assert c["skipped"] == 0   # a mouth is no hole: nothing in it may be skipped


def test_step_edge_pixels():
    g = S.get("step_edge_pixels")
    assert g.shape == (2, 12, 600)
    r = S.oracle("step_edge_pixels")
    assert r["num_labels"].tolist() == [14, 15]
    assert r["contours_per_layer"].tolist() == [13, 14]
    for z in range(2):
        c = S.census(g[z])
        assert all(c["start_at_step_edge"][k] >= 2 for k in (255, 0, 1)), c
        assert c["skipped"] == 0
    c = S.census(g[1])
    assert c["second_start_stale_lnbd"] >= 1
    assert c["taken_lnbd_earlier_step"] >= 9
    assert S.census(g[0])["taken_lnbd_earlier_step"] == 0


def test_row_flag_steps():
    g = S.get("row_flag_steps")
    assert g.shape == (1, 131, 40)
    assert np.flatnonzero(g[0].any(axis=1)).tolist() == S.ROW_FLAG_ROWS
    padded = [y + 1 for y in S.ROW_FLAG_ROWS]
    for edge in (S.ROW_FLAGS, 2 * S.ROW_FLAGS):   # the ballots cover padded rows 1..64, 65..128, ...
        assert edge in padded and edge + 1 in padded
    r = S.oracle("row_flag_steps")
    n = int(r["contours_per_layer"][0])
    assert n == 10 and r["num_labels"].tolist() == [11]
    ends = np.cumsum(r["contour_sizes"])
    firsts = [tuple(r["contour_points"][e - k][::-1]) for e, k in zip(ends, r["contour_sizes"])]
    assert firsts == sorted(firsts, reverse=True) and len(set(y for y, _ in firsts)) == 7


def test_lds_limit():
    sizes = [S.contour_image_bytes(W, H) for H, W in S.LDS_SHAPES]
    assert sizes == [162976, 164000] and sizes[0] <= S.LDS_MAX < sizes[1]
    for H, W in S.LDS_SHAPES:
        g = S.get(f"lds_limit_{H}")
        assert g.shape == (2, H, W) and g[0, :, W - 1].any() and g[0, H - 1, 0]
        r = S.oracle(f"lds_limit_{H}")
        assert r["contours_per_layer"][0] == r["contours_per_layer"][1] > 40
        for z in range(2):
            c = S.census(g[z])
            assert c["skipped_lnbd_earlier_step"] >= 100 and c["taken_lnbd_earlier_step"] >= 10
            assert c["skipped_lnbd_run_start_earlier_step"] >= 6
            # (flipped, the two-pixel row is the one on which the column itself starts: lnbd 0)
            assert c["second_start_stale_lnbd"] >= (1 if z == 0 else 0)
            assert all(c["start_at_step_edge"][k] >= 2 for k in (255, 0, 1))
            # starts judged in every step of the row, the last one included
            xs = r["contour_points"][np.cumsum(r["contour_sizes"]) - r["contour_sizes"], 0]
            assert set(((xs + 1) // S.SCAN_STEP).tolist()) == {0, 1, 2, 3}


def test_zigzag_layers():
    g = S.get("zigzag_layers")
    assert g.shape == (6, 4, 40)
    r = S.oracle("zigzag_layers")
    assert r["num_labels"].tolist() == [7] * 6
    assert r["num_objects"] == 5
    # the full closure: in-plane 8-connectivity plus the straight vertical link
    st = np.zeros((3, 3, 3))
    st[1] = 1
    st[0, 1, 1] = st[2, 1, 1] = 1
    closed = ndimage.label(g > 0, structure=st)[1] + 1   # + the background
    assert closed == 2 and r["num_objects"] > closed


def test_wide_merge():
    g = S.get("wide_merge")
    assert g.shape == (3, 66, 66)
    r = S.oracle("wide_merge")
    assert r["num_labels"].tolist() == [1090, 529, 1090]
    assert min(r["num_labels"][0], r["num_labels"][2]) > S.MERGE_CHUNK
    assert int(r["num_labels"].sum()) > 2 * S.MERGE_CHUNK
    # 528 bridges (two cells above, two below, the bar), 2 x 33 lone cells, the background
    assert r["num_objects"] == 528 + 66 + 1
    assert np.bincount(r["merged"]).max() == 5


def test_many_layers():
    g = S.get("many_layers")
    assert g.shape == (300, 5, 6) and g.shape[0] > S.PACK_THREADS
    filled = g.reshape(300, -1).any(axis=1)
    full = g.reshape(300, -1).all(axis=1)
    for lo, hi in ((0, 256), (257, 300)):
        z = np.arange(lo + 1, hi - 1)
        assert (~filled[z] & filled[z - 1] & filled[z + 1]).any()   # an empty layer between two
        assert full[lo:hi].any()
    r = S.oracle("many_layers")
    assert (r["contours_per_layer"] > 0).tolist() == filled.tolist()
    assert r["contours_per_layer"][:256].sum() > 0 and len(set(r["contours_per_layer"].tolist())) >= 3
    starts = np.cumsum(r["num_labels"]) - r["num_labels"]
    assert (r["stats"][starts[full], 4] == 0).all()   # empty background labels


def test_cell_values():
    g = S.get("cell_values")
    assert g.shape == (2, 9, 20)
    assert {127, 128, 200, 255} <= set(np.unique(g).tolist())
    import oracle as oracle_mod
    r = S.oracle("cell_values")
    assert_same(r, oracle_mod.object_segmentation_front((g > 0).astype(np.uint8)))
    assert r["num_labels"].tolist() == [5, 4]


def test_label_limit_grids():
    import oracle as oracle_mod
    assert parts(S.label_limit(False)[0])[1] == 65536
    r = oracle_mod.object_segmentation_front(S.label_limit(True))
    assert r["num_labels"].tolist() == [65536] and r["labels"].max() == 65535
