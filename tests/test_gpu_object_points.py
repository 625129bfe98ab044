"""Object ids per point and the points grouped by object on the GPU (include/gdf_segment.h, "object
id per point") against the CPU restatement of the rule (tests/object_points_ref.py).  Every output
is compared bit for bit on u32 views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import object_points_ref as opr
import oracle as oracle_mod
from drive import run_batch
from test_segment_kat import blobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ros_gpu_depthmap_fusion_amd", "lib")
FIX = os.path.join(ROOT, "tests", "golden", "facade")
NONE = opr.NONE
TILE = 2048  # kOpTile of csrc/gdf_object_points.hpp: the items of one partition tile
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 4099)
NOBJS = (1, 2, 255, 256, 257, 65536, 65537)  # 1 / 2 / 3 passes, both sides of each boundary
CANARY = 0xC0FFEE11


@pytest.fixture(scope="module")
def seg(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import Segmenter
    s = Segmenter(0)
    yield s
    s.close()


def hiprt():
    from ros_gpu_depthmap_fusion_amd import hiprt as h
    return h


def dev(a):
    return hiprt().DeviceArray.from_numpy(np.ascontiguousarray(a))


def d2h(ptr, dtype, count):
    h = hiprt()
    out = np.empty(count, dtype)
    if out.nbytes:
        h.check(h.hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, h.D2H),
                "hipMemcpy D2H")
    return out


def h2d(ptr, a):
    h = hiprt()
    a = np.ascontiguousarray(a)
    h.check(h.hip().hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, h.H2D),
            "hipMemcpy H2D")


def odd_points(rng, n):
    """n float4 rows of distinct random bit patterns, with NaNs (payloads), -0.0 and denormals."""
    p = rng.integers(0, 2**32, (n, 4), dtype=np.uint64).astype(np.uint32)
    p[:, 3] = (np.arange(n, dtype=np.uint64) * 2654435761 % 2**32).astype(np.uint32)  # distinct rows
    if n:
        p[0::5, 0] = 0x80000000   # -0.0
        p[1::5, 1] = 0x7FC00123   # a quiet NaN with a payload
        p[2::5, 2] = 0xFF800001   # a signalling NaN
        p[3::5, 0] = 0x00000001   # the smallest denormal
    return p.view(np.float32)


def run_group(seg, pts, ids, nobj, keep=None):
    """group_points over host arrays: the downloaded result"""
    n_cap = len(ids)
    d_pts = dev(pts) if n_cap else hiprt().DeviceArray(16)
    d_ids = dev(ids) if n_cap else hiprt().DeviceArray(4)
    d_keep = dev(keep) if keep is not None else None
    seg.group_points(d_pts.ptr, d_ids.ptr, n_cap, nobj, d_keep.ptr if d_keep else 0)
    return seg.object_points_results()


def id_patterns(rng, n, nobj):
    """name -> (ids, keep or None)"""
    rnd = rng.integers(0, nobj, n).astype(np.uint32)
    step = max(nobj // max(n, 1), 1)
    asc = (np.arange(n, dtype=np.uint64) * step).astype(np.uint32)  # distinct; >= nobj past the end
    third = rnd.copy()
    third[::3] = NONE
    over = rng.integers(0, nobj + 3, n).astype(np.uint32)
    over[1::4] = rng.choice(np.array([nobj, 1 << 24, 1 << 31, NONE - 1], np.uint32), len(over[1::4]))
    mask = rng.integers(0, 2, nobj).astype(np.uint8)
    return {
        "all_equal": (np.full(n, nobj - 1, np.uint32), None),
        "ascending": (asc, None),
        "descending": (asc[::-1].copy(), None),
        "random": (rnd, None),
        "third_none": (third, None),
        "over_nobj": (over, None),
        "keep_mask": (rnd, mask),
        "all_dropped": (rnd, np.zeros(nobj, np.uint8)),
        "all_none": (np.full(n, NONE, np.uint32), None),
    }


# ---- the partition alone ------------------------------------------------------------------------
@pytest.mark.parametrize("nobj", NOBJS)
def test_partition_sizes_and_patterns(seg, nobj):
    rng = np.random.default_rng(nobj)
    kept_any = False
    for n in SIZES:
        pts = odd_points(rng, n)
        for name, (ids, keep) in id_patterns(rng, n, nobj).items():
            want = opr.group(pts, ids, nobj, keep)
            got = run_group(seg, pts, ids, nobj, keep)
            try:
                opr.assert_equal(got, want)
            except AssertionError as e:
                raise AssertionError(f"n {n} nobj {nobj} {name}: {e}") from None
            kept_any |= want["total"] > 0
            if name in ("all_dropped", "all_none"):
                assert got["total"] == 0 and not got["obj_start"].any()
            if name == "all_equal":
                assert got["total"] == n and got["index"].tolist() == list(range(n))
    assert kept_any


@pytest.mark.parametrize("n,words", [(32 * TILE, 8192), (32 * TILE + 1, 8448)])
def test_partition_on_both_sides_of_the_scan_switch(seg, n, words):
    """The digit table of an n-point call has 256 words per tile.  Up to 8 scan tiles of 1024 words
    (32 partition tiles) one block scans it alone; from 33 partition tiles on the scan takes three
    launches (tile sums, their scan, apply).  Two passes (nobj 257) on either side of the switch."""
    assert 256 * -(-n // TILE) == words and (words <= 8 * 1024) == (n == 32 * TILE)
    nobj = 257
    rng = np.random.default_rng(n)
    pts = odd_points(rng, n)
    pats = id_patterns(rng, n, nobj)
    for name in ("random", "keep_mask"):
        ids, keep = pats[name]
        want = opr.group(pts, ids, nobj, keep)
        got = run_group(seg, pts, ids, nobj, keep)
        try:
            opr.assert_equal(got, want)
        except AssertionError as e:
            raise AssertionError(f"n {n} nobj {nobj} {name}: {e}") from None
        assert want["total"] > 0


@pytest.mark.parametrize("n,count", [(4099, 4099), (4099, 2048), (1025, 63), (65, 0), (64, 200)])
def test_device_count_and_canary_rows(seg, n, count):
    """A device count below n_cap: the rows behind it are neither read nor written, and nothing
    is written behind the kept total."""
    nobj, pad = 300, 37
    rng = np.random.default_rng(n + count)
    m = min(count, n + pad)  # the rows the call may read
    ids = rng.integers(0, nobj + 2, n + pad).astype(np.uint32)
    pts = odd_points(rng, n + pad)
    ids[m:] = 7                                              # canaries: would land in object 7
    pts[m:] = np.full(4, CANARY, np.uint32).view(np.float32)
    want = opr.group(pts[:m], ids[:m], nobj)
    assert (n == 65) == (want["total"] == 0)
    # size the result buffers, paint them, then run the call under test on the same capacity
    run_group(seg, pts, ids, nobj)
    seg.object_points_counts()
    d = seg.object_points_device()
    assert d["ids"] == 0 and d["voxels"] == 0               # group_points computes neither
    h2d(d["points"], np.full((n + pad, 4), CANARY, np.uint32))
    h2d(d["index"], np.full(n + pad, CANARY, np.uint32))
    d_pts, d_ids, d_cnt = dev(pts), dev(ids), dev(np.array([count], np.uint32))
    seg.group_points(d_pts.ptr, d_ids.ptr, n + pad, nobj, 0, d_cnt.ptr)
    got = seg.object_points_results()
    opr.assert_equal(got, want)
    d2 = seg.object_points_device()
    assert d2["points"] == d["points"] and d2["index"] == d["index"]  # (grow-only: not moved)
    assert d2h(d2["count"], np.uint32, 1)[0] == want["total"]
    t = want["total"]
    out = d2h(d2["points"], np.uint32, 4 * (n + pad)).reshape(-1, 4)
    idx = d2h(d2["index"], np.uint32, n + pad)
    assert np.array_equal(out[:t], want["points"].view(np.uint32))
    assert (out[t:] == CANARY).all() and (idx[t:] == CANARY).all()
    assert not (want["points"].view(np.uint32) == CANARY).all(axis=1).any()


def test_one_segmenter_reused_across_sizes(gpu_engine_factory):
    """Workspace growth and hygiene: large -> small -> large, nobj up and down, one segmenter."""
    from ros_gpu_depthmap_fusion_amd.gdf import Segmenter
    s = Segmenter(0)
    try:
        rng = np.random.default_rng(5)
        for n, nobj in ((4099, 65537), (63, 2), (TILE + 1, 257), (1, 1), (4099, 65537), (0, 5),
                        (1025, 256), (3 * TILE + 5, 70000), (64, 65536), (4099, 3)):
            pts = odd_points(rng, n)
            ids = rng.integers(0, nobj + 1, n).astype(np.uint32)
            keep = rng.integers(0, 2, nobj).astype(np.uint8)
            for k in (None, keep):
                opr.assert_equal(run_group(s, pts, ids, nobj, k), opr.group(pts, ids, nobj, k))
    finally:
        s.close()


def test_argument_checks(seg):
    from ros_gpu_depthmap_fusion_amd.gdf import GDFError
    pts, ids = dev(odd_points(np.random.default_rng(0), 8)), dev(np.arange(8, dtype=np.uint32))
    for args in ((0, ids.ptr, 8, 4), (pts.ptr, 0, 8, 4), (pts.ptr, ids.ptr, 8, 0),
                 (pts.ptr, ids.ptr, 8, (1 << 24) + 1)):
        with pytest.raises(GDFError) as e:
            seg.group_points(*args)
        assert e.value.status == -1, args
    seg.group_points(pts.ptr, ids.ptr, 0, 4)                 # n_cap == 0: empty results
    r = seg.object_points_results()
    assert r["total"] == 0 and r["nobj"] == 4 and r["obj_start"].tolist() == [0] * 5
    seg.group_points(pts.ptr, ids.ptr, 8, 1 << 24)           # the cap itself is served
    r = seg.object_points_results()
    assert r["total"] == 8 and r["index"].tolist() == list(range(8))
    assert r["obj_start"][:10].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8] and r["obj_start"][-1] == 8


# ---- ids alone ----------------------------------------------------------------------------------
def label_grid(seg, g, flags=None):
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS
    L, H, W = g.shape
    d = dev(np.ascontiguousarray(g, np.uint8))
    seg.label_layers(d.ptr, W, H, L, SEG_CONNECTIONS if flags is None else flags)
    return d


@pytest.mark.parametrize("shape,seed", [((1, 9, 11), 1), ((2, 33, 35), 2), ((3, 70, 64), 3),
                                         ((2, 1, 77), 6)])
def test_point_ids_on_blob_grids(seg, shape, seed):
    rng = np.random.default_rng(seed)
    g = blobs(rng, *shape, 0.45)
    L, H, W = shape
    ncells = W * H * L
    n = 3000
    cells = rng.integers(0, ncells, n).astype(np.uint32)
    cells[:4] = (ncells - 1, ncells, 0xFFFFFFFF, 0)
    cells[4:20] = rng.integers(ncells, 2**32, 16, dtype=np.uint64).astype(np.uint32)
    keep_grid = label_grid(seg, g)
    d_cells = dev(cells)
    d_ids = dev(np.full(n + 5, CANARY, np.uint32))
    d_cnt = dev(np.array([n - 100], np.uint32))
    seg.point_object_ids(d_cells.ptr, n, d_ids.ptr)           # before results(): it merges itself
    r = seg.results(contours=False)
    got = d_ids.to_numpy(np.uint32, n + 5)
    o = oracle_mod.object_segmentation_front(g)
    want = opr.point_ids(r, cells)
    assert np.array_equal(want, opr.point_ids(o, cells))
    flat = g.reshape(-1)
    inside = cells < ncells
    assert (want[inside] == NONE).tolist() == (flat[cells[inside]] == 0).tolist()
    assert (want[~inside] == NONE).all() and 0 < (want != NONE).sum() < n
    assert np.array_equal(got[:n], want) and (got[n:] == CANARY).all()
    # a device count: the ids behind it are left alone
    h2d(d_ids.ptr, np.full(n + 5, CANARY, np.uint32))
    seg.point_object_ids(d_cells.ptr, n, d_ids.ptr, d_cnt.ptr)
    seg.merge_labels()                                        # (waits for the stream)
    got = d_ids.to_numpy(np.uint32, n + 5)
    assert np.array_equal(got[:n - 100], want[:n - 100]) and (got[n - 100:] == CANARY).all()
    del keep_grid


# ---- engine stage -------------------------------------------------------------------------------
def dense_frames(eng, p, frames=3, sequence=False):
    from ros_gpu_depthmap_fusion_amd import synth
    eye = np.eye(4, dtype=np.float32)
    lidar = synth.make_camera(1, 96, 64)
    for f in range(frames):
        eng.clear()
        if sequence and f == frames - 1:
            eng.addPointSequence(synth.back_project(lidar, synth.dense_frame(lidar, 1, f)), 5000, 0, eye)
        for k in range(2):
            cam = synth.make_camera(k, 320, 240)
            eng.addDepthmap(synth.dense_frame(cam, f, k), *cam.intrinsics(), cam.T_world, cam.T_crop)
        if sequence:
            eng.processFrame(p, T_world_move=lidar.T_world, T_crop_move=lidar.T_crop)
        else:
            eng.processFrame(p)


def check_engine_stage(seg, eng, min_voxels):
    segres = seg.results(contours=False)
    pts, coords = eng.downloadPoints(), eng.downloadVoxelCoords()
    want = opr.object_points(segres, pts, coords, min_voxels)
    seg.object_points(eng, min_voxels)
    got = seg.object_points_results()
    opr.assert_equal(got, want)
    assert len(got["ids"]) == len(pts) == eng.point_count()
    return want


def test_engine_stage(seg, gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, ComponentParams
    eng = gpu_engine_factory(0)
    try:
        p = ComponentParams()
        assert 1 <= p.occupancy_lifetime <= 255
        dense_frames(eng, p)
        seg.label_engine_grid(eng, SEG_CONNECTIONS)
        w0 = check_engine_stage(seg, eng, 0)
        n = len(w0["ids"])
        # lifetime in 1..255: every point's cell is marked, so every point is in an object
        assert n > 10000 and not (w0["ids"] == NONE).any() and w0["total"] == n
        sizes = w0["voxels"][w0["voxels"] > 0]
        assert len(sizes) > 2 and sizes.min() < sizes.max()
        opr.assert_equal(check_engine_stage(seg, eng, 1), w0)
        mid = int(sizes.min()) + max((int(sizes.max()) - int(sizes.min())) // 2, 1)
        wm = check_engine_stage(seg, eng, mid)
        assert 0 < wm["total"] < n and np.array_equal(wm["ids"], w0["ids"])
        wb = check_engine_stage(seg, eng, 2**31)
        assert wb["total"] == 0
        # a new labelling on the same segmenter, then the stage again
        seg.label_engine_grid(eng)
        opr.assert_equal(check_engine_stage(seg, eng, mid), wm)
        d = seg.object_points_device()
        assert all(d[k] for k in ("ids", "points", "index", "obj_start", "voxels", "count"))
    finally:
        eng.close()


def test_engine_stage_lifetime_256_marks_nothing(seg, gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, ComponentParams
    eng = gpu_engine_factory(0)
    try:
        p = ComponentParams()
        p.occupancy_lifetime = 256  # the u8 grid stores 0: every cell is background
        dense_frames(eng, p, frames=1)
        assert not eng.downloadVoxelOccupancyGrid().any()
        seg.label_engine_grid(eng, SEG_CONNECTIONS)
        w = check_engine_stage(seg, eng, 0)
        assert len(w["ids"]) > 10000 and (w["ids"] == NONE).all() and w["total"] == 0
        assert not w["voxels"].any()
    finally:
        eng.close()


def test_engine_stage_with_rollbuffer_window(seg, gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, ComponentParams
    eng = gpu_engine_factory(0)
    try:
        p = ComponentParams()
        p.ps_filter_size = 0
        p.ps_timespan = 1000.0
        dense_frames(eng, p, frames=1)
        depth_only = eng.point_count()
        dense_frames(eng, p, frames=1, sequence=True)
        assert eng.point_count() > depth_only > 0           # selected sequence points are in
        seg.label_engine_grid(eng, SEG_CONNECTIONS)
        w = check_engine_stage(seg, eng, 0)
        assert w["total"] == len(w["ids"]) > depth_only
        check_engine_stage(seg, eng, 8)
    finally:
        eng.close()


def test_engine_stage_after_labelling_on_the_segmenters_stream(gpu_engine_factory):
    """label_layers and group_points run on the segmenter's own (non-blocking) stream and return
    without a wait; object_points runs on the engine's.  Each must see the other's finished work."""
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, ComponentParams, Segmenter
    eng, s = gpu_engine_factory(0), Segmenter(0)
    try:
        p = ComponentParams()
        dense_frames(eng, p)
        s.label_engine_grid(eng, SEG_CONNECTIONS)            # the engine's stream, then a wait
        mv = 8
        want = check_engine_stage(s, eng, mv)
        assert 0 < want["total"]
        (W, H, L), _ = eng.grid_size()
        grid = eng.downloadVoxelOccupancyGrid().reshape(L, H, W)
        d_grid = dev(grid)
        other = dev(np.ones((L, H, W), np.uint8))            # one object per grid: other labels
        rng = np.random.default_rng(5)
        n, nobj = 20 * TILE + 7, 300
        gp, gi = odd_points(rng, n), rng.integers(0, nobj, n).astype(np.uint32)
        gwant = opr.group(gp, gi, nobj, None)
        d_gp, d_gi = dev(gp), dev(gi)
        for _ in range(3):
            s.label_layers(other.ptr, W, H, L, SEG_CONNECTIONS)
            s.label_layers(d_grid.ptr, W, H, L, SEG_CONNECTIONS)   # own stream, no final wait
            s.object_points(eng, mv)                               # engine's stream
            opr.assert_equal(s.object_points_results(), want)
            # the workspace is shared: a partition on the own stream, then the stage again
            s.group_points(d_gp.ptr, d_gi.ptr, n, nobj)
            s.object_points(eng, mv)
            opr.assert_equal(s.object_points_results(), want)
            # ... and the other way round
            s.object_points(eng, 0)
            s.group_points(d_gp.ptr, d_gi.ptr, n, nobj)
            opr.assert_equal(s.object_points_results(), gwant)
    finally:
        s.close()
        eng.close()


def test_ids_length_belongs_to_the_call(gpu_engine_factory):
    """The result keeps the n of its own call when the engine goes on to a frame of another size."""
    from ros_gpu_depthmap_fusion_amd import synth
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, ComponentParams, Segmenter
    eng, s = gpu_engine_factory(0), Segmenter(0)
    try:
        p = ComponentParams()
        dense_frames(eng, p, frames=1)
        s.label_engine_grid(eng, SEG_CONNECTIONS)
        want = check_engine_stage(s, eng, 0)
        n = len(want["ids"])
        s.object_points(eng, 0)
        c = synth.make_camera(0, 160, 120)
        eng.clear()
        eng.addDepthmap(synth.dense_frame(c, 0, 0), *c.intrinsics(), c.T_world, c.T_crop)
        eng.processFrame(p)
        assert 0 < eng.point_count() < n
        got = s.object_points_results()
        assert len(got["ids"]) == n
        opr.assert_equal(got, want)
    finally:
        s.close()
        eng.close()


# ---- refusals -----------------------------------------------------------------------------------
def test_refusals(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd import synth
    from ros_gpu_depthmap_fusion_amd.gdf import (SEG_CONNECTIONS, SEG_CONTOURS, ComponentParams,
                                                GDFError, Segmenter)
    eng, s = gpu_engine_factory(0), Segmenter(0)

    def refused(f, *a):
        with pytest.raises(GDFError) as e:
            f(*a)
        assert e.value.status == -2, (a, e.value)

    def cam(W, H, k=0):
        c = synth.make_camera(0, W, H)
        return (synth.dense_frame(c, 0, k), *c.intrinsics(), c.T_world, c.T_crop)

    try:
        p = ComponentParams()
        eng.clear()
        eng.addDepthmap(*cam(160, 120))
        eng.processFrame(p)
        gs, _ = eng.grid_size()
        cells, ids = dev(np.zeros(4, np.uint32)), dev(np.zeros(4, np.uint32))
        refused(s.object_points, eng)                        # no labelling
        refused(s.point_object_ids, cells.ptr, 4, ids.ptr)
        refused(s.object_points_results)                     # no result either
        s.label_engine_grid(eng, SEG_CONTOURS)               # a labelling without connections
        refused(s.object_points, eng)
        refused(s.point_object_ids, cells.ptr, 4, ids.ptr)
        small = np.ones((2, 5, 7), np.uint8)
        g = label_grid(s, small)                             # not the engine's grid size
        refused(s.object_points, eng)
        s.label_engine_grid(eng, SEG_CONNECTIONS)
        s.object_points(eng)
        good = s.object_points_results()
        assert good["total"] == eng.point_count() > 1000
        # the engine's side: what radiusFilter(source="points") refuses
        eng.clear()
        refused(s.object_points, eng)                        # before the frame's compaction
        run_batch(eng, p, [[cam(160, 120, 0)], [cam(160, 120, 1)]])
        refused(s.object_points, eng)                        # a multi-frame batch
        nparts, cap = 3, 160 * 120
        h = hiprt()
        sp, srk, srs = h.DeviceArray(16 * cap), h.DeviceArray(4 * cap), h.DeviceArray(4 * cap)
        cnt = h.DeviceArray(8 * nparts)
        eng.clear()
        eng.addDepthmap(*cam(160, 120))
        eng.set_emit_partition(nparts, sp.ptr, srk.ptr, srs.ptr, cap, cnt.ptr)
        eng.processFrame(p, synchronous=True, defer_occupancy_grid=True, defer_voxelize=True)
        refused(s.object_points, eng)                        # armed with the emit partition
        # a refused call launched nothing and left the last result alone
        opr.assert_equal(s.object_points_results(), good, keys=("points", "index", "obj_start"))
        # ... and the next valid call is correct
        eng.clear()
        eng.addDepthmap(*cam(160, 120))
        eng.processFrame(p)
        s.label_engine_grid(eng, SEG_CONNECTIONS)
        w = check_engine_stage(s, eng, 0)                    # (against the reference on this grid)
        assert w["total"] == good["total"]
        del g
    finally:
        s.close()
        eng.close()


# ---- facade -------------------------------------------------------------------------------------
def test_facade_object_points(tmp_path, seg):
    exe = tmp_path / "facade_object_points"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "facade_object_points.cpp"), "-L", LIB, "-lgdf",
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
        pts, coords = rd("points", "<f4").reshape(-1, 4), rd("coords", "<u4")
        got = {"ids": rd("ids", "<u4"), "points": rd("opoints", "<f4").reshape(-1, 4),
               "index": rd("oindex", "<u4"), "obj_start": rd("ostarts", "<u4"),
               "voxels": rd("ovoxels", "<u4")}
        got["nobj"], got["total"] = len(got["voxels"]), len(got["index"])
        o = oracle_mod.object_segmentation_front(grid)
        want = opr.object_points(o, pts, coords, mv)
        assert len(pts) > 0 and want["total"] > 0, f
        opr.assert_equal(got, want)
        # the Python binding on the same data: ids from the labelled grid, then the partition
        keep_grid = label_grid(seg, grid)
        d_cells, d_ids, d_pts = dev(coords), dev(np.zeros(len(coords), np.uint32)), dev(pts)
        seg.point_object_ids(d_cells.ptr, len(coords), d_ids.ptr)
        nobj = seg.merge_labels()[1]
        d_keep = dev(opr.keep_of(got["voxels"], mv))
        seg.group_points(d_pts.ptr, d_ids.ptr, len(coords), nobj, d_keep.ptr)
        py = seg.object_points_results()
        assert np.array_equal(d_ids.to_numpy(np.uint32, len(coords)), got["ids"]), f
        opr.assert_equal(py, got, keys=("points", "index", "obj_start"))
        del keep_grid
