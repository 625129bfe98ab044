"""The object layer per segment of the rows and per frame of an engine's batch on the GPU
(include/gdf_segment.h, "the object layer per segment") against the CPU restatement
of the rules (tests/object_segments_ref.py) and, GPU against GPU, against the unsegmented calls on
every slice.  All outputs are integers or copies: every comparison is bit for bit, and the outputs
are painted before the calls so that nothing is written outside a result."""
import numpy as np
import pytest

import object_moments_ref as omr
import object_points_ref as opr
import object_segment_scenes as scenes
import object_segments_ref as osr
import voxel_table_ref as vtr
from drive import run_batch
from test_gpu_object_points import d2h, dev, h2d, hiprt, label_grid

pytestmark = pytest.mark.gpu

NONE = osr.NONE
CANARY = 0xC0FFEE11
ARG, STATE, CAPACITY = -1, -2, -5
PARTITION = scenes.partition_scenes()
TABLE = scenes.table_scenes()


@pytest.fixture(scope="module")
def seg(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import Segmenter
    s = Segmenter(0)
    yield s
    s.close()


def grouped(seg) -> dict:
    r = seg.object_points_results()
    r["seg_out_start"] = seg.group_segments()
    d_ptr, nseg = seg.group_segments_device()
    assert nseg == len(r["seg_out_start"]) - 1 and np.array_equal(d2h(d_ptr, np.uint32, nseg + 1), r["seg_out_start"])
    return r


def tabled(seg) -> dict:
    r = seg.voxel_table_results()
    r["vox_seg_start"] = seg.voxel_segments()
    d_ptr, nseg = seg.voxel_segments_device()
    assert nseg == len(r["vox_seg_start"]) - 1 and np.array_equal(d2h(d_ptr, np.uint32, nseg + 1), r["vox_seg_start"])
    return r


def run_group(seg, d_pts, d_ids, n_cap, starts, nobj, d_keep=0):
    """group_points_segments on device arrays, its row outputs painted first: the downloaded result;
    behind the kept total the paint must survive."""
    d_st = dev(starts)
    args = (d_pts, d_ids, n_cap, d_st.ptr, len(starts) - 1, nobj, d_keep)
    seg.group_points_segments(*args)                          # sizes the workspace
    seg.object_points_counts()
    d = seg.object_points_device()
    h2d(d["points"], np.full(4 * max(n_cap, 1), CANARY, np.uint32))
    h2d(d["index"], np.full(max(n_cap, 1), CANARY, np.uint32))
    seg.group_points_segments(*args)
    got = grouped(seg)
    d2 = seg.object_points_device()
    assert d2["points"] == d["points"] and d2["index"] == d["index"] and d2["ids"] == 0 == d2["voxels"]
    total = got["total"]
    assert d2h(d2["count"], np.uint32, 1)[0] == total
    assert (d2h(d2["points"], np.uint32, 4 * max(n_cap, 1))[4 * total:] == CANARY).all()
    assert (d2h(d2["index"], np.uint32, max(n_cap, 1))[total:] == CANARY).all()
    return got


def slices_group(seg, d_pts, d_ids, n_cap, starts, nobj, d_keep=0) -> dict:
    """The defining property on the same device arrays: gdf_seg_group_points on every slice."""
    st = iter(osr.clamp_starts(starts, n_cap).tolist())
    state = {"a": next(st)}

    def rule(pts, ids, nobj_, keep):
        a, b = state["a"], next(st)
        state["a"] = b
        seg.group_points(d_pts + 16 * a, d_ids + 4 * a, b - a, nobj_, d_keep)
        return seg.object_points_results()

    z = np.zeros(n_cap, np.uint32)                            # (the rule reads the device arrays)
    return osr.group_by_slices(np.zeros((n_cap, 4), np.float32), z, starts, nobj, None, slice_rule=rule)


def run_table(seg, d_cells, n_cap, starts, C):
    """voxel_table_segments on a device array, its outputs painted first; behind G and n, and before
    the first segment, the paint must survive."""
    d_st = dev(starts)
    args = (d_cells, n_cap, d_st.ptr, len(starts) - 1, C)
    seg.voxel_table_segments(*args)
    seg.voxel_table_counts()
    d = seg.voxel_table_device()
    # (a voxel has a row and a (segment, cell) pair of its own: the per-voxel arrays hold that many)
    caps = {k: max(n_cap if k == "point_voxel" else min(n_cap, (len(starts) - 1) * C), 1) for k in vtr.KEYS}
    for k in vtr.KEYS:
        h2d(d[k], np.full(caps[k], CANARY, np.uint32))
    seg.voxel_table_segments(*args)
    got = tabled(seg)
    d2 = seg.voxel_table_device()
    assert all(d2[k] == d[k] for k in vtr.KEYS) and d2["weights"] == 0 and "weights" not in got
    G, n = got["num_voxels"], got["n"]
    assert d2h(d2["count"], np.uint32, 1)[0] == G
    for k, m in (("vox_cells", G), ("vox_counts", G), ("point_voxel", n)):
        raw = d2h(d2[k], np.uint32, caps[k])
        assert np.array_equal(raw[:m], got[k]) and (raw[m:] == CANARY).all(), (k, m)
    return got


def slices_table(seg, d_cells, n_cap, starts, C) -> dict:
    st = iter(osr.clamp_starts(starts, n_cap).tolist())
    state = {"a": next(st)}

    def rule(cells, C_):
        a, b = state["a"], next(st)
        state["a"] = b
        seg.voxel_table(d_cells + 4 * a, b - a, C_)
        return seg.voxel_table_results()

    return osr.table_by_slices(np.zeros(n_cap, np.uint32), starts, C, fill=CANARY, slice_rule=rule)


# ---- built scenes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PARTITION))
def test_partition_scene(seg, name):
    s = PARTITION[name]
    n = len(s["ids"])
    pts = scenes.odd_points(np.random.default_rng(len(name)), n)
    d_pts, d_ids = dev(pts), dev(s["ids"])
    d_keep = dev(s["keep"]) if s["keep"] is not None else None
    kp = d_keep.ptr if d_keep else 0
    want = osr.group(pts, s["ids"], s["starts"], s["nobj"], s["keep"])
    got = run_group(seg, d_pts.ptr, d_ids.ptr, n, s["starts"], s["nobj"], kp)
    osr.assert_group_equal(got, want)
    assert got["nobj"] == s["nobj"] and seg.object_points_device()["obj_start"]
    osr.assert_group_equal(slices_group(seg, d_pts.ptr, d_ids.ptr, n, s["starts"], s["nobj"], kp), want)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_scene(seg, name):
    s = TABLE[name]
    n = len(s["cells"])
    d_cells = dev(s["cells"])
    want = osr.table(s["cells"], s["starts"], s["C"], fill=CANARY)
    got = run_table(seg, d_cells.ptr, n, s["starts"], s["C"])
    osr.assert_table_equal(got, want)
    osr.assert_table_equal(slices_table(seg, d_cells.ptr, n, s["starts"], s["C"]), want)


def test_rows_outside_the_segments_are_not_read(seg):
    """A capacity above the last start and rows below the first one: those rows hold ids and cells
    that would be kept (and are nowhere else), and they leave no trace."""
    n_cap, nobj, C = 3000, 9, 4000
    rng = np.random.default_rng(5)
    starts = np.array([130, 700, 700, 2100], np.uint32)
    ids = rng.integers(0, nobj - 1, n_cap).astype(np.uint32)
    cells = rng.integers(0, C - 50, n_cap).astype(np.uint32)
    ids[:130] = ids[2100:] = nobj - 1
    cells[:130] = C - 1 - np.arange(130, dtype=np.uint32) % 50
    cells[2100:] = C - 1 - np.arange(900, dtype=np.uint32) % 50
    pts = scenes.odd_points(rng, n_cap)
    d_pts, d_ids, d_cells = dev(pts), dev(ids), dev(cells)
    got = run_group(seg, d_pts.ptr, d_ids.ptr, n_cap, starts, nobj)
    osr.assert_group_equal(got, osr.group(pts, ids, starts, nobj))
    assert got["total"] == 2100 - 130 and not np.diff(got["obj_start"].astype(np.int64))[nobj - 1::nobj].any()
    t = run_table(seg, d_cells.ptr, n_cap, starts, C)
    osr.assert_table_equal(t, osr.table(cells, starts, C, fill=CANARY))
    assert t["n"] == 2100 and not (t["vox_cells"] >= C - 50).any() and (t["point_voxel"][:130] == CANARY).all()


def test_unaligned_pointers(seg):
    """cells at +4 bytes and points at +16 bytes of their allocations."""
    n, nobj, C = 2500, 11, 900
    rng = np.random.default_rng(6)
    starts = np.array([0, 65, 1000, 2049, n], np.uint32)
    ids, cells = rng.integers(0, nobj + 1, n).astype(np.uint32), rng.integers(0, C + 1, n).astype(np.uint32)
    pts = scenes.odd_points(rng, n)
    d_pts = dev(np.concatenate([np.zeros((1, 4), np.float32), pts]))
    d_ids = dev(np.concatenate([[0], ids]).astype(np.uint32))
    d_cells = dev(np.concatenate([[0], cells]).astype(np.uint32))
    got = run_group(seg, d_pts.ptr + 16, d_ids.ptr + 4, n, starts, nobj)
    osr.assert_group_equal(got, osr.group(pts, ids, starts, nobj))
    t = run_table(seg, d_cells.ptr + 4, n, starts, C)
    osr.assert_table_equal(t, osr.table(cells, starts, C))


def test_a_small_call_after_a_large_one(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import Segmenter
    s = Segmenter(0)
    try:
        rng = np.random.default_rng(7)

        def once(n, nseg, nobj, C):
            starts = np.concatenate([[0], np.sort(rng.integers(0, n + 1, nseg - 1)), [n]]).astype(np.uint32)
            ids, cells = rng.integers(0, nobj + 1, n).astype(np.uint32), rng.integers(0, C + 1, n).astype(np.uint32)
            pts = scenes.odd_points(rng, n)
            d_pts, d_ids, d_cells = dev(pts), dev(ids), dev(cells)
            osr.assert_group_equal(run_group(s, d_pts.ptr, d_ids.ptr, n, starts, nobj), osr.group(pts, ids, starts, nobj))
            osr.assert_table_equal(run_table(s, d_cells.ptr, n, starts, C), osr.table(cells, starts, C))

        once(70000, 16, 5000, 1 << 20)
        for n, nseg, nobj, C in ((63, 2, 3, 33), (5, 64, 1, 1), (257, 3, 300, 513), (1, 1, 1, 1), (4099, 8, 40, 70000)):
            once(n, nseg, nobj, C)
        once(70000, 16, 5000, 1 << 20)
    finally:
        s.close()


def test_moments_of_a_segmented_result(seg):
    """One record per (segment, object), in group order."""
    n, nseg, nobj = 5000, 5, 7
    rng = np.random.default_rng(8)
    grid = dict(lower=np.array([-1, -2, -0.5], np.float32), cell=np.array([0.1, 0.1, 0.12], np.float32),
                gs=np.array([30, 40, 9], np.uint32))
    pts = np.concatenate([rng.uniform(-1.2, 2.2, (n, 1)), rng.uniform(-2.2, 2.2, (n, 1)),
                          rng.uniform(-0.6, 0.7, (n, 1)), np.ones((n, 1))], 1).astype(np.float32)
    ids = rng.integers(0, nobj + 1, n).astype(np.uint32)
    starts = np.array([0, 512, 512, 2049, 4000, n - 3], np.uint32)
    d_pts, d_ids = dev(pts), dev(ids)
    want = osr.group(pts, ids, starts, nobj)
    osr.assert_group_equal(run_group(seg, d_pts.ptr, d_ids.ptr, n, starts, nobj), want)
    got = seg.object_moments(grid["lower"], grid["cell"], grid["gs"])
    assert len(got) == nseg * nobj
    omr.assert_equal(got, omr.moments(want["points"], want["obj_start"], **grid))
    assert int(got["count"].sum() + got["outside"].sum()) == want["total"] and got["outside"].sum() > 0


def test_argument_checks(seg):
    from ros_gpu_depthmap_fusion_amd.gdf import GDFError
    rng = np.random.default_rng(9)
    n, nobj, C = 300, 5, 1000
    ids, cells = rng.integers(0, nobj, n).astype(np.uint32), rng.integers(0, C, n).astype(np.uint32)
    pts = scenes.odd_points(rng, n)
    starts = np.array([0, 100, n], np.uint32)
    d_pts, d_ids, d_cells, d_st = dev(pts), dev(ids), dev(cells), dev(starts)
    big = dev(np.zeros(66, np.uint32))
    good_g = run_group(seg, d_pts.ptr, d_ids.ptr, n, starts, nobj)
    good_t = run_table(seg, d_cells.ptr, n, starts, C)

    def refused(f, *a, status=ARG):
        with pytest.raises(GDFError) as e:
            f(*a)
        assert e.value.status == status, (a, e.value)
        osr.assert_group_equal(grouped(seg), good_g)             # the earlier results are still readable
        osr.assert_table_equal(tabled(seg), good_t)

    for nseg, k in scenes.PARTITION_REFUSALS:
        refused(seg.group_points_segments, d_pts.ptr, d_ids.ptr, n, big.ptr, nseg, k)
    for a in ((0, d_ids.ptr, n, d_st.ptr, 2, nobj), (d_pts.ptr, 0, n, d_st.ptr, 2, nobj), (d_pts.ptr, d_ids.ptr, n, 0, 2, nobj)):
        refused(seg.group_points_segments, *a)
    for nseg, k in scenes.TABLE_REFUSALS:
        refused(seg.voxel_table_segments, d_cells.ptr, n, big.ptr, nseg, k)
    refused(seg.voxel_table_segments, 0, n, d_st.ptr, 2, C)
    refused(seg.voxel_table_segments, d_cells.ptr, n, 0, 2, C)
    buf = np.zeros(8, np.uint32)
    for get in (seg._lib.gdf_seg_get_group_segments, seg._lib.gdf_seg_get_voxel_segments):
        with pytest.raises(GDFError) as e:
            seg._check(get(seg._h, None, buf.ctypes.data, 2))
        assert e.value.status == CAPACITY
    with pytest.raises(GDFError) as e:                         # obj_start holds nseg * nobj + 1 words
        seg._check(seg._lib.gdf_seg_download_object_points(seg._h, None, 0, None, None, 0, buf.ctypes.data, None, nobj + 1))
    assert e.value.status == CAPACITY
    # n_cap == 0: empty results
    seg.group_points_segments(d_pts.ptr, d_ids.ptr, 0, d_st.ptr, 2, nobj)
    r = grouped(seg)
    assert r["total"] == 0 and not r["obj_start"].any() and len(r["obj_start"]) == 2 * nobj + 1
    assert r["seg_out_start"].tolist() == [0, 0, 0]
    seg.voxel_table_segments(d_cells.ptr, 0, d_st.ptr, 2, C)
    t = tabled(seg)
    assert t["num_voxels"] == 0 and t["n"] == 0 and t["vox_seg_start"].tolist() == [0, 0, 0]
    # an unsegmented result has no segment table
    seg.group_points(d_pts.ptr, d_ids.ptr, n, nobj)
    seg.voxel_table(d_cells.ptr, n, C)
    for f in (seg.group_segments, seg.voxel_segments, seg.group_segments_device, seg.voxel_segments_device):
        with pytest.raises(GDFError) as e:
            f()
        assert e.value.status == STATE
    assert len(seg.object_points_results()["obj_start"]) == nobj + 1


# ---- engine batches -----------------------------------------------------------------------------------
def params(lifetime=10, average=True):
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    p = ComponentParams()
    p.occupancy_lifetime = lifetime
    p.voxel_average = average
    return p


def cam(W, H, f=0, k=0):
    from ros_gpu_depthmap_fusion_amd import synth
    c = synth.make_camera(k, W, H)
    return (synth.dense_frame(c, f, k), *c.intrinsics(), c.T_world, c.T_crop)


def batch(eng, p, B, W=160, H=120):
    run_batch(eng, p, [[cam(W, H, f)] for f in range(B)])


def ranges(eng, B):
    if B == 1:
        return np.array([0, eng.point_count()], np.uint32), np.array([0, eng.voxelized_count()], np.uint32)
    ps, vs = eng.batch_ranges()
    return np.asarray(ps, np.uint32), np.asarray(vs, np.uint32)


def check_points_batch(seg, eng, B, min_voxels):
    segres = seg.results(contours=False)
    pts, coords = eng.downloadPoints(), eng.downloadVoxelCoords()
    ps, _ = ranges(eng, B)
    assert len(ps) == B + 1 and ps[-1] == len(pts)
    want = osr.object_points_batch(segres, pts, coords, ps, min_voxels)
    seg.object_points_batch(eng, min_voxels)
    got = grouped(seg)
    osr.assert_group_equal(got, want, keys=osr.GROUP_KEYS + ("ids", "voxels"))
    assert len(got["obj_start"]) == B * got["nobj"] + 1 and got["nobj"] == segres["num_objects"]
    return want, ps


def check_voxels_batch(seg, eng, B, min_voxels):
    segres = seg.results(contours=False)
    coords, vox = eng.downloadVoxelCoords(), eng.downloadVoxelizedPoints()
    ps, vs = ranges(eng, B)
    want = osr.object_voxels_batch(segres, coords, ps, vox, min_voxels)
    seg.object_voxels_batch(eng, min_voxels)
    got = grouped(seg)
    got.update(tabled(seg))
    osr.assert_group_equal(got, want, keys=osr.GROUP_KEYS + ("ids", "voxels"))
    osr.assert_table_equal(got, want)
    assert np.array_equal(got["weights"], want["weights"])
    assert np.array_equal(got["vox_seg_start"], vs)              # the engine's own voxel ranges
    assert got["num_voxels"] == len(vox) == len(got["ids"]) and got["n"] == len(coords)
    return want


@pytest.mark.parametrize("B,W,H,lifetime,average",
                         [(2, 160, 120, 10, True), (3, 160, 120, 10, False), (8, 160, 120, 10, True),
                          (3, 160, 120, 1, True), (8, 160, 120, 1, False), (8, 640, 480, 10, True)])
def test_engine_batch(seg, gpu_engine_factory, B, W, H, lifetime, average):
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, GDFError
    eng = gpu_engine_factory(0)
    try:
        p = params(lifetime, average)
        batch(eng, p, B, W, H)
        seg.label_engine_grid(eng, SEG_CONNECTIONS)              # the grid after the batch's last frame
        w0, ps = check_points_batch(seg, eng, B, 0)
        ncells = eng.grid_size()[1]
        coords = eng.downloadVoxelCoords()
        assert len(coords) > 1000 * B and (np.diff(ps.astype(np.int64)) > 0).all()
        if lifetime >= B:   # every in-grid point of every frame lies in a foreground cell of the grid
            assert not (w0["ids"][coords < ncells] == NONE).any()
            inside = np.concatenate([[0], np.cumsum(coords < ncells)])[ps.astype(np.int64)]
            assert np.array_equal(w0["seg_out_start"], inside) and inside[-1] > 0.99 * len(coords)
        sizes = w0["voxels"][w0["voxels"] > 0]
        mid = int(sizes.min()) + max((int(sizes.max()) - int(sizes.min())) // 2, 1)
        wm, _ = check_points_batch(seg, eng, B, mid)
        assert wm["total"] <= w0["total"] and np.array_equal(wm["ids"], w0["ids"])
        v0 = check_voxels_batch(seg, eng, B, 0)
        assert int(v0["weights"].sum()) == w0["total"]
        # a voxelized row carries the id of the points folded into it
        pv = v0["point_voxel"]
        assert np.array_equal(v0["ids"][pv[pv != NONE]], w0["ids"][pv != NONE])
        vm = check_voxels_batch(seg, eng, B, mid)
        assert vm["total"] <= v0["total"]
        # the moments of the grouped voxelized rows: one record per (frame, object)
        gs, _ = eng.grid_size()
        grid = dict(lower=np.asarray(p.voxel_min, np.float32), cell=np.asarray(p.voxel_size, np.float32),
                    gs=np.array(gs, np.uint32))
        m = seg.object_moments(grid["lower"], grid["cell"], grid["gs"])
        assert len(m) == B * vm["nobj"]
        omr.assert_equal(m, omr.moments(vm["points"], vm["obj_start"], **grid))
        for f in (seg.object_points, seg.object_voxels):         # the single-frame calls still refuse
            with pytest.raises(GDFError) as e:
                f(eng)
            assert e.value.status == STATE and "multi-frame batch" in str(e.value)
    finally:
        eng.close()


@pytest.mark.parametrize("average", [True, False])
def test_a_one_frame_batch_equals_the_single_frame_calls(seg, gpu_engine_factory, average):
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS
    eng = gpu_engine_factory(0)
    try:
        p = params(10, average)
        batch(eng, p, 1)
        seg.label_engine_grid(eng, SEG_CONNECTIONS)
        for mv in (0, 40):
            check_points_batch(seg, eng, 1, mv)
            a = grouped(seg)
            seg.object_points(eng, mv)
            b = seg.object_points_results()
            opr.assert_equal(a, b)
            assert a["seg_out_start"].tolist() == [0, b["total"]] and a["total"] > 0
            check_voxels_batch(seg, eng, 1, mv)
            a = grouped(seg)
            a.update(tabled(seg))
            seg.object_voxels(eng, mv)
            b = seg.object_points_results()
            b.update(seg.voxel_table_results())
            opr.assert_equal(a, b)
            vtr.assert_equal(a, b)
            assert np.array_equal(a["weights"], b["weights"])
            assert a["vox_seg_start"].tolist() == [0, b["num_voxels"]]
    finally:
        eng.close()


def test_refusals_and_invalidation(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, SEG_CONTOURS, GDFError, Segmenter
    eng, s = gpu_engine_factory(0), Segmenter(0)

    def refused(f, *a, status=STATE, text=""):
        with pytest.raises(GDFError) as e:
            f(*a)
        assert e.value.status == status and text in str(e.value), (a, e.value)

    try:
        p = params()
        batch(eng, p, 2)
        for f in (s.object_points_batch, s.object_voxels_batch):
            refused(f, eng)                                      # no labelling
        s.label_engine_grid(eng, SEG_CONTOURS)                   # a labelling without connections
        for f in (s.object_points_batch, s.object_voxels_batch):
            refused(f, eng)
        g = label_grid(s, np.ones((2, 5, 7), np.uint8))          # not the engine's grid size
        for f in (s.object_points_batch, s.object_voxels_batch):
            refused(f, eng, text="not the engine's grid")
        s.label_engine_grid(eng, SEG_CONNECTIONS)
        good = check_voxels_batch(s, eng, 2, 0)
        assert good["total"] == good["num_voxels"] > 100

        def still_good():
            got = grouped(s)
            got.update(tabled(s))
            osr.assert_group_equal(got, good, keys=osr.GROUP_KEYS + ("ids", "voxels"))
            osr.assert_table_equal(got, good)
            assert np.array_equal(got["weights"], good["weights"])

        eng.clear()
        refused(s.object_voxels_batch, eng, text="compaction")   # before the frame's compaction
        refused(s.object_points_batch, eng, text="compaction")
        eng.addDepthmap(*cam(160, 120))
        eng.processFrame(p, synchronous=True, defer_occupancy_grid=True, defer_voxelize=True)
        refused(s.object_voxels_batch, eng, text="before the frame's voxelize")
        still_good()
        nparts, cap = 3, 160 * 120
        h = hiprt()
        sp, srk, srs = h.DeviceArray(16 * cap), h.DeviceArray(4 * cap), h.DeviceArray(4 * cap)
        cnt = h.DeviceArray(8 * nparts)
        eng.clear()
        eng.addDepthmap(*cam(160, 120))
        eng.set_emit_partition(nparts, sp.ptr, srk.ptr, srs.ptr, cap, cnt.ptr)
        eng.processFrame(p, synchronous=True, defer_occupancy_grid=True, defer_voxelize=True)
        refused(s.object_voxels_batch, eng, text="emit partition")
        refused(s.object_points_batch, eng, text="emit partition")
        still_good()                                             # refusals launched nothing
        eng.set_emit_partition(0)
        # the grouped result is the segmenter's: object_points_batch replaces it, the table stays
        batch(eng, p, 3)
        s.label_engine_grid(eng, SEG_CONNECTIONS)
        w = check_voxels_batch(s, eng, 3, 0)
        check_points_batch(s, eng, 3, 0)
        r = tabled(s)
        osr.assert_table_equal(r, w)
        assert "weights" not in r and s.voxel_table_device()["weights"] == 0
        # a labelling after the calls invalidates the table and the grouped result
        s.object_voxels_batch(eng, 0)
        s.label_engine_grid(eng, SEG_CONNECTIONS)
        for f in (s.voxel_table_results, s.object_points_results, s.group_segments, s.voxel_segments):
            refused(f)
        check_voxels_batch(s, eng, 3, 0)                         # ... and the next valid call is correct
        del g
    finally:
        s.close()
        eng.close()


def test_profiled_calls_report_their_passes(seg, gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, GDFError
    eng = gpu_engine_factory(0)
    try:
        p = params()
        batch(eng, p, 3)
        seg.label_engine_grid(eng, SEG_CONNECTIONS)
        seg.set_profiling(True)
        want, _ = check_points_batch(seg, eng, 3, 0)             # profiled: the same result
        groups = 3 * want["nobj"]
        passes = 1 if groups <= 256 else 2 if groups <= 65536 else 3
        ms = seg.object_points_times()
        assert len(ms) == 2 * passes + 3 and (ms >= 0).all() and ms.sum() > 0
        check_voxels_batch(seg, eng, 3, 0)
        ms = seg.voxel_table_times()
        assert len(ms) == 8 and (ms >= 0).all() and ms.sum() > 0
        d_cells, d_st = dev(np.arange(100, dtype=np.uint32)), dev(np.array([0, 50, 100], np.uint32))
        seg.voxel_table_segments(d_cells.ptr, 100, d_st.ptr, 2, 1000)
        assert len(seg.voxel_table_times()) == 5
        seg.set_profiling(False)
        seg.object_voxels_batch(eng, 0)
        with pytest.raises(GDFError):
            seg.voxel_table_times()
    finally:
        seg.set_profiling(False)
        eng.close()
