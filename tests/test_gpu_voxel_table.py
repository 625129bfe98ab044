"""The voxel table and the object ids of the voxelized cloud on the GPU (include/gdf_segment.h, "the
voxel table") against the CPU restatement of the rule (tests/voxel_table_ref.py).
All outputs are integers (the grouped rows are copies): every comparison is bit for bit, and every
output buffer is painted before the call so that nothing is written behind a result's end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import object_moments_ref as omr
import object_points_ref as opr
import voxel_ref
import voxel_table_ref as vtr
from drive import run_batch
from test_gpu_object_points import d2h, dev, h2d, hiprt, label_grid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ros_gpu_depthmap_fusion_amd", "lib")
FIX = os.path.join(ROOT, "tests", "golden", "facade")
NONE = vtr.NONE
CANARY = 0xC0FFEE11
ARG, STATE, CAPACITY = -1, -2, -5
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099)
ROW = 2048           # cells per counted bitmap row: 32 * kVtRowWords of csrc/gdf_voxel_table.hpp
SCAN_ONE = 8192      # rows the scan of gdf_scan.hip takes in one launch (8 tiles of 1024 words)
MAX_CELLS = 1 << 28  # kVtMaxCells


@pytest.fixture(scope="module")
def seg(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import Segmenter
    s = Segmenter(0)
    yield s
    s.close()


def run_table(seg, cells, C):
    """voxel_table over a host array, its outputs painted first: the downloaded result."""
    cells = np.asarray(cells, np.uint32)
    n_cap = len(cells)
    d_cells = dev(cells) if n_cap else hiprt().DeviceArray(4)
    args = (d_cells.ptr, n_cap, C)
    seg.voxel_table(*args)                                   # sizes the workspace
    seg.voxel_table_counts()
    d = seg.voxel_table_device()
    for k in vtr.KEYS:
        h2d(d[k], np.full(max(n_cap, 1), CANARY, np.uint32))
    seg.voxel_table(*args)
    got = seg.voxel_table_results()
    d2 = seg.voxel_table_device()
    assert all(d2[k] == d[k] for k in vtr.KEYS)              # (grow-only: not moved)
    assert d2["weights"] == 0 and "weights" not in got       # the stand-alone call computes none
    G, n = got["num_voxels"], got["n"]
    assert d2h(d2["count"], np.uint32, 1)[0] == G
    raw = {k: d2h(d2[k], np.uint32, max(n_cap, 1)) for k in vtr.KEYS}
    for k, m in (("vox_cells", G), ("vox_counts", G), ("point_voxel", n)):
        assert np.array_equal(raw[k][:m], got[k]), k
        assert (raw[k][m:] == CANARY).all(), (k, m, np.flatnonzero(raw[k][m:] != CANARY)[:8] + m)
    return got


def check_table(seg, cells, C, what=""):
    cells = np.asarray(cells, np.uint32)
    want = vtr.table(cells, C)
    got = run_table(seg, cells, C)
    try:
        vtr.assert_equal(got, want)
    except AssertionError as e:
        raise AssertionError(f"{what} n {len(cells)} C {C}: {e}") from None
    return want


def run_lengths(rng, n):
    """Run lengths of 1 to 130 rows that sum to n, with borders at rows 63|64 and 255|256 inside
    runs and at them."""
    out, left = [], n
    while left > 0:
        r = min(int(rng.integers(1, 131)), left)
        out.append(r)
        left -= r
    return np.array(out, np.int64)


def patterns(rng, n, C):
    """name -> cells"""
    rnd = rng.integers(0, C, n).astype(np.uint32)
    if 0 < n <= C:  # distinct and ascending, from a random first cell to the grid's end
        first = int(rng.integers(0, C - n + 1))
        asc = (first + np.arange(n, dtype=np.uint64) * ((C - first) // n)).astype(np.uint32)
    else:
        asc = (np.arange(n, dtype=np.uint64) % C).astype(np.uint32)
    lens = run_lengths(rng, n)
    runs = np.repeat(rng.integers(0, C, len(lens)), lens).astype(np.uint32)
    # runs that cross lane 63|64 and thread 255|256: one cell from row 60 to 69 and from 250 to 262
    cross = runs.copy()
    cross[60:70] = C - 1
    cross[250:263] = 0
    third = rnd.copy()
    third[::3] = rng.choice(np.array([C, C + 1, 1 << 31, NONE], np.uint64), len(third[::3])).astype(np.uint32)
    return {"one_cell": np.full(n, C // 2, np.uint32), "ascending": asc, "descending": asc[::-1].copy(),
            "random": rnd, "runs": runs, "runs_crossing": cross, "third_outside": third,
            "all_outside": np.full(n, C, np.uint32)}


# ---- the stand-alone table ------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4099 * 3, 3_360_000])
def test_sizes_and_patterns(seg, C):
    rng = np.random.default_rng(C)
    some = outside = False
    for n in SIZES:
        for name, cells in patterns(rng, n, C).items():
            want = check_table(seg, cells, C, what=name)
            some |= want["num_voxels"] > 1
            outside |= bool((want["point_voxel"] == NONE).any())
            if name == "one_cell" and n:
                assert want["num_voxels"] == 1 and want["vox_counts"].tolist() == [n]
            if name == "ascending" and n:
                assert (np.diff(cells.astype(np.int64)) > 0).all()
                assert want["num_voxels"] == n and (want["vox_counts"] == 1).all()
            if name == "all_outside":
                assert want["num_voxels"] == 0
    assert some and outside


@pytest.mark.parametrize("n,count", [(4099, 4099), (4099, 2048), (1025, 63), (65, 0), (64, 200), (257, 256)])
def test_device_count_below_the_capacity(seg, n, count):
    """Rows at and beyond n = min(*count, n_cap) are neither read (they hold in-range cells that are
    nowhere else) nor written."""
    C, pad = 50000, 37
    rng = np.random.default_rng(n + count)
    m = min(count, n + pad)
    cells = patterns(rng, n + pad, C - 100)["runs"]
    cells[m:] = C - 1 - np.arange(n + pad - m, dtype=np.uint32) % 50   # poison: cells of no read row
    d_cells, d_cnt = dev(cells), dev(np.array([count], np.uint32))
    seg.voxel_table(d_cells.ptr, n + pad, C, d_cnt.ptr)
    seg.voxel_table_counts()
    d = seg.voxel_table_device()
    for k in vtr.KEYS:
        h2d(d[k], np.full(n + pad, CANARY, np.uint32))
    seg.voxel_table(d_cells.ptr, n + pad, C, d_cnt.ptr)
    got, want = seg.voxel_table_results(), vtr.table(cells[:m], C)
    vtr.assert_equal(got, want)
    assert got["n"] == m and not (got["vox_cells"] >= C - 100).any()
    G = want["num_voxels"]
    for k, e in (("vox_cells", G), ("vox_counts", G), ("point_voxel", m)):
        assert (d2h(d[k], np.uint32, n + pad)[e:] == CANARY).all(), k


@pytest.mark.parametrize("C", [1, 31, 32, 33, 511, 512, 513])
def test_small_grids(seg, C):
    rng = np.random.default_rng(C)
    for n in (1, 65, 257, 1025):
        every = np.resize(np.arange(C, dtype=np.uint32), max(n, C))         # every cell, 0 and C - 1 too
        want = check_table(seg, every, C, what="every cell")
        assert want["num_voxels"] == C and want["vox_cells"].tolist() == list(range(C))
        ends = np.resize(np.array([C - 1, 0], np.uint32), max(n, 2))
        want = check_table(seg, ends, C, what="ends")
        assert want["vox_cells"].tolist() == sorted({0, C - 1})
        for name, cells in patterns(rng, n, C).items():
            check_table(seg, cells, C, what=name)


def test_word_and_row_borders(seg):
    """Bits 0 and 31 of one word; the last word of one counted row and the first of the next (words
    63 and 64: the library counts rows of 64 words, not the 16 of the first shape, whose borders
    stay in the list); the words around a 256-word block of k_vt_rows / k_vt_expand."""
    C, RW = 40 * ROW, ROW // 32
    edges = []
    for w in (0, 1, 15, 16, 17, 31, 32, RW - 1, RW, RW + 1, 255, 256, 257, RW * 39 + RW - 1):
        edges += [32 * w, 32 * w + 31]
    edges = np.array(edges, np.uint32)
    want = check_table(seg, np.repeat(edges, 3)[::-1].copy(), C, what="edges")
    assert np.array_equal(want["vox_cells"], np.sort(edges)) and (want["vox_counts"] == 3).all()
    for pair in ((15 * 32 + 31, 16 * 32), (ROW - 1, ROW), (256 * 32 - 1, 256 * 32), (39 * ROW - 1, 39 * ROW)):
        want = check_table(seg, np.array(pair[::-1], np.uint32), C, what="pair")
        assert want["vox_cells"].tolist() == list(pair) and want["point_voxel"].tolist() == [1, 0]
    rng = np.random.default_rng(16)
    full = rng.permutation(C).astype(np.uint32)                              # every bit of every word
    want = check_table(seg, full, C, what="full")
    assert want["num_voxels"] == C and np.array_equal(want["point_voxel"], full)


@pytest.mark.parametrize("C", [SCAN_ONE * ROW, SCAN_ONE * ROW + 1])
def test_both_sides_of_the_scan_switch(seg, C):
    """8192 counted rows are scanned by one block in one launch, 8193 take three launches; cells in
    the first and the last row on either side."""
    assert (-(-C // ROW) <= SCAN_ONE) == (C == SCAN_ONE * ROW)
    rng = np.random.default_rng(C)
    cells = np.concatenate([rng.integers(0, ROW, 300), rng.integers(C - min(ROW, C % ROW or ROW), C, 300),
                            rng.integers(0, C, 2000), [0, C - 1, C, C + 1]]).astype(np.uint32)
    rng.shuffle(cells)
    want = check_table(seg, cells, C, what="scan switch")
    assert want["vox_cells"][0] == 0 and want["vox_cells"][-1] == C - 1
    assert (want["point_voxel"] == NONE).sum() == 2


def test_one_voxel_of_70000_rows(seg):
    C, n = 3_360_000, 70000
    want = check_table(seg, np.full(n, 1234567, np.uint32), C, what="one counter")
    assert want["vox_counts"].tolist() == [n]
    mixed = np.full(n, 1234567, np.uint32)
    mixed[::1000] = np.arange(70, dtype=np.uint32) * 17
    want = check_table(seg, mixed, C, what="one big counter among small ones")
    assert want["vox_counts"].max() == n - 70 and want["num_voxels"] == 71


def test_4099_voxels_of_one_row(seg):
    C = 3_360_000
    cells = np.random.default_rng(3).choice(C, 4099, replace=False).astype(np.uint32)
    want = check_table(seg, cells, C, what="one row each")
    assert want["num_voxels"] == 4099 and (want["vox_counts"] == 1).all()


def test_a_small_call_after_a_large_one(gpu_engine_factory):
    """One segmenter: a large table, then a small one.  No bit, rank or count of the first survives,
    and the grown workspace needs no cleaning by the caller."""
    from ros_gpu_depthmap_fusion_amd.gdf import Segmenter
    s = Segmenter(0)
    try:
        rng = np.random.default_rng(8)
        big_c = SCAN_ONE * ROW + 1
        check_table(s, rng.integers(0, big_c, 70000).astype(np.uint32), big_c, what="large")
        for n, C in ((63, 33), (5, big_c), (257, 513), (0, 7), (1, 1), (4099, 3_360_000)):
            for name in ("random", "runs", "third_outside"):
                check_table(s, patterns(rng, n, C)[name], C, what=f"small {name}")
        check_table(s, rng.integers(0, big_c, 70000).astype(np.uint32), big_c, what="large again")
    finally:
        s.close()


def test_argument_checks(seg):
    from ros_gpu_depthmap_fusion_amd.gdf import GDFError
    rng = np.random.default_rng(1)
    cells = rng.integers(0, 1000, 300).astype(np.uint32)
    good = check_table(seg, cells, 1000, what="good")
    d_cells = dev(cells)
    for args in ((0, 300, 1000), (d_cells.ptr, 300, 0), (d_cells.ptr, 300, MAX_CELLS + 1)):
        with pytest.raises(GDFError) as e:
            seg.voxel_table(*args)
        assert e.value.status == ARG, args
        vtr.assert_equal(seg.voxel_table_results(), good)    # the earlier result is still readable
    with pytest.raises(GDFError) as e:                       # the stand-alone call computes no weights
        seg._check(seg._lib.gdf_seg_download_voxel_table(seg._h, None, None, 0, None, 0,
                                                         good["vox_cells"].ctypes.data, 1000))
    assert e.value.status == STATE
    with pytest.raises(GDFError) as e:
        seg._check(seg._lib.gdf_seg_download_voxel_table(seg._h, good["vox_cells"].ctypes.data, None,
                                                         good["num_voxels"] - 1, None, 0, None, 0))
    assert e.value.status == CAPACITY
    seg.voxel_table(d_cells.ptr, 0, 1000)                    # n_cap == 0: G = 0
    r = seg.voxel_table_results()
    assert r["num_voxels"] == 0 and r["n"] == 0
    seg.voxel_table(d_cells.ptr, 300, MAX_CELLS)             # the bound itself is served
    vtr.assert_equal(seg.voxel_table_results(), good)


# ---- with an engine ---------------------------------------------------------------------------------
def dense_params():
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    return ComponentParams()


def dense_frame(eng, p, W, H, f=0, cams=1):
    from ros_gpu_depthmap_fusion_amd import synth
    eng.clear()
    for k in range(cams):
        cam = synth.make_camera(k, W, H)
        eng.addDepthmap(synth.dense_frame(cam, f, k), *cam.intrinsics(), cam.T_world, cam.T_crop)
    eng.processFrame(p)


def fixture_frame(eng, f, average):
    """Frame f of the facade fixture's inputs (a 160 x 120 depth map and a 64 x 48 point sequence
    that the rollbuffer window selects) through gdf_process_frame."""
    if os.path.join(ROOT, "tests", "golden") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_facade_golden as g
    p = g.params()
    p.voxel_average = average
    cam, lidar, depth, cloud, sec, nsec, Tm = g.inputs(f)
    eng.clear()
    eng.addPointSequence(cloud, sec, nsec, Tm)
    eng.addDepthmap(depth, *cam.intrinsics(), cam.T_world, cam.T_crop)
    eng.processFrame(p, T_world_move=lidar.T_world, T_crop_move=lidar.T_crop)
    return p


def grid_of(p):
    return voxel_ref.Grid(p.voxel_min, p.voxel_max, p.voxel_size)


def check_object_voxels(seg, eng, p, min_voxels, cap):
    """gdf_seg_object_voxels on the engine's frame against the rule on the downloaded frame, and
    the table against the engine's own voxelized rows.  cap: the frame's depth pixels, which the
    frame's capacity is not below; every output of the call is painted up to it (the per-voxel ones
    up to min(cap, the grid's cells), which is what the library sizes them by at least), and behind
    its end (G, n or the kept total) the paint must survive.  Returns the expected result."""
    segres = seg.results(contours=False)
    pts, coords, vox = eng.downloadPoints(), eng.downloadVoxelCoords(), eng.downloadVoxelizedPoints()
    want = vtr.object_voxels(segres, coords, vox, min_voxels)
    seg.object_voxels(eng, min_voxels)                       # sizes the workspace
    seg.object_points_counts()                               # (waits)
    vc = min(cap, eng.grid_size()[1])
    assert len(coords) <= cap and len(vox) <= vc
    dt, do = seg.voxel_table_device(), seg.object_points_device()
    painted = {"vox_cells": (dt, vc), "vox_counts": (dt, vc), "point_voxel": (dt, cap),
               "weights": (dt, vc), "ids": (do, vc), "index": (do, vc)}
    for k, (d, m) in painted.items():
        assert d[k], k
        h2d(d[k], np.full(m, CANARY, np.uint32))
    seg.object_voxels(eng, min_voxels)
    got = seg.object_points_results()
    got.update(seg.voxel_table_results())
    opr.assert_equal(got, want)
    vtr.assert_equal(got, want)
    assert np.array_equal(got["weights"], want["weights"])
    dt2, do2 = seg.voxel_table_device(), seg.object_points_device()
    ends = {"vox_cells": want["num_voxels"], "vox_counts": want["num_voxels"], "point_voxel": want["n"],
            "weights": want["total"], "ids": want["num_voxels"], "index": want["total"]}
    for k, (d, m) in painted.items():
        d2 = dt2 if d is dt else do2
        assert d2[k] == d[k], k                              # (grow-only: not moved)
        raw = d2h(d2[k], np.uint32, m)
        assert np.array_equal(raw[:ends[k]], got[k]), k
        assert (raw[ends[k]:] == CANARY).all(), (k, ends[k], np.flatnonzero(raw[ends[k]:] != CANARY)[:8])
    G = got["num_voxels"]
    assert G == eng.voxelized_count() == len(got["ids"]) and got["n"] == len(coords) == eng.point_count()
    assert np.array_equal(got["vox_cells"], np.unique(coords))
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    if p.voxel_average:
        assert np.array_equal(bits(vox), bits(vtr.chain_means(pts, got["point_voxel"], G)))
    else:
        assert np.array_equal(bits(vox), bits(grid_of(p).corners(got["vox_cells"])))
    return want


def check_against_object_points(seg, eng, want, min_voxels, first_frame=False):
    """The same frame, labelling and min_voxels through gdf_seg_object_points."""
    seg.object_points(eng, min_voxels)
    raw = seg.object_points_results()
    pv = want["point_voxel"]
    inside = pv != NONE
    assert len(raw["ids"]) == len(pv) and inside.any()
    assert np.array_equal(want["ids"][pv[inside]], raw["ids"][inside])   # a point has its voxel's id
    assert (raw["ids"][~inside] == NONE).all()
    assert np.array_equal(raw["voxels"], want["voxels"])
    wsum = np.add.reduceat(np.concatenate([want["weights"], [0]]).astype(np.int64),
                           want["obj_start"][:-1].astype(np.int64))
    nrows = np.diff(want["obj_start"].astype(np.int64))
    wsum[nrows == 0] = 0
    assert np.array_equal(wsum, np.diff(raw["obj_start"].astype(np.int64)))
    if first_frame:  # a fresh grid: an object's voxels are this frame's voxels
        kept = opr.keep_of(want["voxels"], min_voxels) != 0
        assert kept.any() and np.array_equal(nrows[kept], want["voxels"][kept])
        assert not nrows[~kept].any()


def stage_cases(seg, eng, p, first_frame, cap, varied=True):
    """min_voxels 0, a middle value and one above every object; then the tie to §12.  varied: the
    frame has objects of different sizes, so the middle value keeps some and drops some."""
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS
    seg.label_engine_grid(eng, SEG_CONNECTIONS)
    w0 = check_object_voxels(seg, eng, p, 0, cap)
    G = w0["num_voxels"]
    assert G > 100 and w0["total"] == G and not (w0["ids"] == NONE).any()
    assert int(w0["weights"].sum()) == w0["n"] and w0["weights"].max() > 1
    sizes = w0["voxels"][w0["voxels"] > 0]
    varied = varied or sizes.min() < sizes.max()
    assert len(sizes) >= 1 and (not varied or sizes.min() < sizes.max())
    mid = int(sizes.min()) + max((int(sizes.max()) - int(sizes.min())) // 2, 1) if varied else int(sizes.max())
    wm = check_object_voxels(seg, eng, p, mid, cap)
    assert 0 < wm["total"] <= G and (wm["total"] < G) == varied and np.array_equal(wm["ids"], w0["ids"])
    wb = check_object_voxels(seg, eng, p, int(sizes.max()) + 1, cap)
    assert wb["total"] == 0 and not wb["obj_start"].any() and len(wb["weights"]) == 0
    check_against_object_points(seg, eng, w0, 0, first_frame)
    check_against_object_points(seg, eng, wm, mid, first_frame)
    # the moments of the grouped voxelized rows (unweighted: every row counts once)
    seg.object_voxels(eng, mid)
    gs, _ = eng.grid_size()
    grid = dict(lower=np.asarray(p.voxel_min, np.float32), cell=np.asarray(p.voxel_size, np.float32),
                gs=np.array(gs, np.uint32))
    omr.assert_equal(seg.object_moments(grid["lower"], grid["cell"], grid["gs"]),
                     omr.moments(wm["points"], wm["obj_start"], **grid))
    return w0


@pytest.mark.parametrize("average", [True, False])
def test_fixture_frames(seg, gpu_engine_factory, average):
    """The 160 x 120 fixture frames; frames 1 and 2 carry the rollbuffer's selected clouds."""
    eng = gpu_engine_factory(0)
    try:
        depth_only = None
        for f in range(3):
            p = fixture_frame(eng, f, average)
            w = stage_cases(seg, eng, p, first_frame=(f == 0), cap=160 * 120, varied=False)
            if average:  # the fixture's own frame (its voxelized rows are means)
                assert np.array_equal(eng.downloadVoxelCoords(),
                                      np.fromfile(os.path.join(FIX, f"coords{f}.bin"), "<u4")), f
                assert w["num_voxels"] == (560, 563, 593)[f]
            depth_only = w["n"] if f == 0 else depth_only
        assert w["n"] > depth_only                              # the selected sequence points are in
    finally:
        eng.close()


@pytest.mark.parametrize("runs,average", [(False, True), (False, False), (True, True), (True, False)])
def test_dense_vga_frame(seg, gpu_engine_factory, monkeypatch, runs, average):
    """One dense 640 x 480 frame on the launch-default grid (3.36 M cells), the voxelize sorting
    points and - forced, as tests/test_gpu_round2.py forces it - runs of equal keys."""
    if runs:
        monkeypatch.setenv("GDF_FORCE_RUNS", "1")
    eng = gpu_engine_factory(0)
    try:
        p = dense_params()
        p.voxel_average = average
        dense_frame(eng, p, 640, 480)
        assert eng.last_sort_items()[1] == runs
        w = stage_cases(seg, eng, p, first_frame=True, cap=640 * 480)
        assert w["n"] > 100000 and eng.grid_size()[1] == 3_360_000
    finally:
        eng.close()


def test_two_cameras_second_frame(seg, gpu_engine_factory):
    """Two 320 x 240 cameras, the second frame of an engine: the grid holds cells of frame 0 that
    frame 1 does not touch, so objects have more voxels than grouped rows."""
    eng = gpu_engine_factory(0)
    try:
        p = dense_params()
        dense_frame(eng, p, 320, 240, f=0, cams=2)
        dense_frame(eng, p, 320, 240, f=5, cams=2)
        w = stage_cases(seg, eng, p, first_frame=False, cap=2 * 320 * 240)
        assert int(w["voxels"].sum()) > w["num_voxels"]
    finally:
        eng.close()


def test_refusals_and_invalidation(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd import synth
    from ros_gpu_depthmap_fusion_amd.gdf import (SEG_CONNECTIONS, SEG_CONTOURS, GDFError, Segmenter)
    eng, s = gpu_engine_factory(0), Segmenter(0)

    def refused(f, *a, status=STATE, text=""):
        with pytest.raises(GDFError) as e:
            f(*a)
        assert e.value.status == status and text in str(e.value), (a, e.value)

    def cam(W, H, k=0):
        c = synth.make_camera(0, W, H)
        return (synth.dense_frame(c, 0, k), *c.intrinsics(), c.T_world, c.T_crop)

    try:
        p = dense_params()
        eng.clear()
        eng.addDepthmap(*cam(160, 120))
        eng.processFrame(p)
        refused(s.object_voxels, eng)                        # no labelling
        refused(s.voxel_table_results)                       # no table either
        s.label_engine_grid(eng, SEG_CONTOURS)               # a labelling without connections
        refused(s.object_voxels, eng)
        g = label_grid(s, np.ones((2, 5, 7), np.uint8))      # not the engine's grid size
        refused(s.object_voxels, eng)
        s.label_engine_grid(eng, SEG_CONNECTIONS)
        good = check_object_voxels(s, eng, p, 0, 160 * 120)
        assert good["total"] == good["num_voxels"] > 100

        def still_good():
            got = s.object_points_results()
            got.update(s.voxel_table_results())
            opr.assert_equal(got, good)
            vtr.assert_equal(got, good)
            assert np.array_equal(got["weights"], good["weights"])

        eng.clear()
        refused(s.object_voxels, eng, text="compaction")     # before the frame's compaction
        eng.addDepthmap(*cam(160, 120))
        eng.processFrame(p, synchronous=True, defer_occupancy_grid=True, defer_voxelize=True)
        refused(s.object_voxels, eng, text="before the frame's voxelize")
        still_good()
        run_batch(eng, p, [[cam(160, 120, 0)], [cam(160, 120, 1)]])
        refused(s.object_voxels, eng, text="multi-frame batch")
        nparts, cap = 3, 160 * 120
        h = hiprt()
        sp, srk, srs = h.DeviceArray(16 * cap), h.DeviceArray(4 * cap), h.DeviceArray(4 * cap)
        cnt = h.DeviceArray(8 * nparts)
        eng.clear()
        eng.addDepthmap(*cam(160, 120))
        eng.set_emit_partition(nparts, sp.ptr, srk.ptr, srs.ptr, cap, cnt.ptr)
        eng.processFrame(p, synchronous=True, defer_occupancy_grid=True, defer_voxelize=True)
        # (this frame is not voxelized either: the text says which refusal it was)
        refused(s.object_voxels, eng, text="emit partition")
        still_good()                                         # refusals launched nothing
        # the grouped result is the segmenter's: object_points replaces it, the table stays
        eng.clear()
        eng.addDepthmap(*cam(160, 120))
        eng.processFrame(p)
        s.label_engine_grid(eng, SEG_CONNECTIONS)
        w = check_object_voxels(s, eng, p, 0, 160 * 120)
        s.object_points(eng, 0)
        r = s.voxel_table_results()
        vtr.assert_equal(r, w)
        assert "weights" not in r and s.voxel_table_device()["weights"] == 0
        # a stand-alone table replaces the table and leaves the grouped points alone
        s.object_voxels(eng, 0)
        d_cells = dev(np.arange(10, dtype=np.uint32))
        s.voxel_table(d_cells.ptr, 10, 10)
        assert "weights" not in s.voxel_table_results()
        opr.assert_equal(s.object_points_results(), w)
        # a labelling after the call invalidates the table and the grouped result
        s.object_voxels(eng, 0)
        s.label_engine_grid(eng, SEG_CONNECTIONS)
        refused(s.voxel_table_results)
        refused(s.object_points_results)
        refused(s.voxel_table_device)
        check_object_voxels(s, eng, p, 0, 160 * 120)         # ... and the next valid call is correct
        del g
    finally:
        s.close()
        eng.close()


def test_profiled_calls_report_their_passes(seg, gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, GDFError
    eng = gpu_engine_factory(0)
    try:
        p = dense_params()
        dense_frame(eng, p, 160, 120)
        seg.label_engine_grid(eng, SEG_CONNECTIONS)
        seg.set_profiling(True)
        want = check_object_voxels(seg, eng, p, 0, 160 * 120)  # profiled: the same result
        ms = seg.voxel_table_times()
        assert len(ms) == 8 and (ms >= 0).all() and ms.sum() > 0
        d_cells = dev(np.arange(100, dtype=np.uint32))
        seg.voxel_table(d_cells.ptr, 100, 1000)
        assert len(seg.voxel_table_times()) == 5
        seg.set_profiling(False)
        seg.object_voxels(eng, 0)
        with pytest.raises(GDFError):
            seg.voxel_table_times()
        got = seg.object_points_results()
        got.update(seg.voxel_table_results())
        opr.assert_equal(got, want)
    finally:
        seg.set_profiling(False)
        eng.close()


# ---- facade -----------------------------------------------------------------------------------------
def test_facade_object_voxels(tmp_path, seg):
    import oracle as oracle_mod
    exe = tmp_path / "facade_object_voxels"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "facade_object_voxels.cpp"), "-L", LIB, "-lgdf",
           "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    outd = tmp_path / "out"
    outd.mkdir()
    mv = 3
    r = subprocess.run([str(exe), FIX, str(outd), str(mv)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    frames = int(open(os.path.join(FIX, "manifest.txt")).readline().split()[1])
    for f in range(frames):
        rd = lambda name, dt: np.fromfile(outd / f"{name}{f}.bin", dt)
        gx, gy, gz = (int(v) for v in open(outd / f"gridsize{f}.txt").read().split())
        grid = rd("grid", "u1").reshape(gz, gy, gx)
        coords, vox = rd("coords", "<u4"), rd("voxelized", "<f4").reshape(-1, 4)
        got = {"vox_cells": rd("vcells", "<u4"), "vox_counts": rd("vcounts", "<u4"),
               "point_voxel": rd("pvoxel", "<u4"), "ids": rd("vids", "<u4"),
               "points": rd("vopoints", "<f4").reshape(-1, 4), "index": rd("voindex", "<u4"),
               "obj_start": rd("vostarts", "<u4"), "weights": rd("voweights", "<u4")}
        got["num_voxels"], got["n"] = len(got["vox_cells"]), len(got["point_voxel"])
        got["nobj"], got["total"] = len(got["obj_start"]) - 1, len(got["index"])
        o = oracle_mod.object_segmentation_front(grid)
        want = vtr.object_voxels(o, coords, vox, mv)
        assert want["num_voxels"] == (560, 563, 593)[f] and want["total"] > 0, f
        vtr.assert_equal(got, want)
        opr.assert_equal(got, want, keys=("ids", "points", "index", "obj_start"))
        assert np.array_equal(got["weights"], want["weights"]), f
        assert np.array_equal(np.ascontiguousarray(vox[:, :3]).view(np.uint32),
                              np.fromfile(os.path.join(FIX, f"voxelized{f}.bin"), "<u4").reshape(-1, 3))
        # the Python binding's stand-alone table on the same coords
        d_cells = dev(coords)
        seg.voxel_table(d_cells.ptr, len(coords), gx * gy * gz)
        vtr.assert_equal(seg.voxel_table_results(), got)
