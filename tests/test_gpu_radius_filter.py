"""The radius outlier filter on the GPU (include/gdf_filter.h) against its CPU restatement
(tests/radius_ref.py): kept points (all four words), count and keep flags bit for bit, through
gdf_radius_filter_points unless a test says otherwise.  Every scene first asserts FROM THE
REFERENCE that it holds what it is there for, so no case can pass empty."""
import functools
import os
import subprocess

import numpy as np
import pytest

import radius_ref as R
import radius_scenes as S
from drive import compare_results, run_batch, stagewise_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ros_gpu_depthmap_fusion_amd", "lib")
FIX = os.path.join(ROOT, "tests", "golden", "facade")
BOX = ((0, -8, -0.5), (10, 8, 2))
BOX_CUT = ((0, -8, -0.5), (5, 8, 2))


@pytest.fixture(scope="module")
def gpu(gpu_engine_factory):
    eng = gpu_engine_factory()
    yield eng
    eng.close()


@functools.lru_cache(maxsize=None)
def ref_of(name, m):
    """The reference of a named scene, computed once and shared (read-only) by the tests."""
    s = S.get(name)
    keep, counts = R.reference(s["pts"], s["lower"], s["upper"], s["radius"], m)
    keep.setflags(write=False)
    counts.setflags(write=False)
    return keep, counts


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_points(gpu, pts, lower, upper, radius, m, with_keep=True):
    """gdf_radius_filter_points over a host array: (out points, count, keep flags)."""
    from ros_gpu_depthmap_fusion_amd import hiprt
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_params
    n = len(pts)
    d_in = hiprt.DeviceArray.from_numpy(pts) if n else hiprt.DeviceArray(16)
    d_out = hiprt.DeviceArray.from_numpy(np.full((max(n, 1), 4), 0xFFFFFFFF, np.uint32))
    d_cnt = hiprt.DeviceArray.from_numpy(np.full(1, 0xFFFFFFFF, np.uint32))
    d_keep = hiprt.DeviceArray.from_numpy(np.full(max(n, 1), 0xFF, np.uint8))
    gpu.radiusFilterPoints(d_in.ptr if n else 0, n, radius_filter_params(lower, upper, radius, m),
                           d_out.ptr if n else 0, d_cnt.ptr, d_keep.ptr if with_keep else 0)
    gpu.synchronize()
    cnt = int(d_cnt.to_numpy(np.uint32, 1)[0])
    assert cnt <= n
    out = d_out.to_numpy(np.float32, 4 * max(n, 1)).reshape(-1, 4)
    keep = d_keep.to_numpy(np.uint8, max(n, 1))[:n]
    return out, cnt, keep


def check(gpu, pts, lower, upper, radius, m, keep_ref, tag):
    out, cnt, keep = run_points(gpu, pts, lower, upper, radius, m)
    want = R.apply(pts, keep_ref)
    assert cnt == len(want), (tag, m, cnt, len(want))
    assert np.array_equal(keep, keep_ref.astype(np.uint8)), (tag, m, "keep flags")
    assert np.array_equal(bits(out[:cnt]), bits(want)), (tag, m, "points")
    # nothing is written behind the count
    assert (bits(out[cnt:]) == 0xFFFFFFFF).all(), (tag, m, "wrote past the count")


def check_scene(gpu, name, mins=None):
    s = S.get(name)
    for m in (mins or s["mins"]):
        check(gpu, s["pts"], s["lower"], s["upper"], s["radius"], m, ref_of(name, m)[0], name)


# ---- micro clouds -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.MICRO_NAMES)
def test_micro_clouds(gpu, name):
    s = S.get(name)
    n = len(s["pts"])
    assert ref_of(name, 0)[0].sum() == n                      # (all inside: min 0 keeps them all)
    assert not ref_of(name, n + 1)[0].any() and not ref_of(name, max(n, 1))[0].any()
    if n >= 2:
        assert ref_of(name, 1)[0].all()
    if name == "micro_n3":
        assert ref_of(name, 2)[0].tolist() == [False, True, False]
    if name == "micro_coincident70":
        assert ref_of(name, 69)[0].all() and ref_of(name, 69)[1].tolist() == [69] * 70
    check_scene(gpu, name)


def test_no_keep_buffer_and_aliasing(gpu):
    from ros_gpu_depthmap_fusion_amd import hiprt
    from ros_gpu_depthmap_fusion_amd.gdf import GDFError, radius_filter_params
    s = S.get("wave_n257_h1")
    out, cnt, _ = run_points(gpu, s["pts"], s["lower"], s["upper"], s["radius"], 1, with_keep=False)
    want = R.apply(s["pts"], ref_of("wave_n257_h1", 1)[0])
    assert 0 < cnt == len(want) and np.array_equal(bits(out[:cnt]), bits(want))
    d = hiprt.DeviceArray.from_numpy(s["pts"])
    o = hiprt.DeviceArray(s["pts"].nbytes)
    c = hiprt.DeviceArray(4)
    p = radius_filter_params(s["lower"], s["upper"], s["radius"], 1)
    with pytest.raises(GDFError) as e:
        gpu.radiusFilterPoints(d.ptr, len(s["pts"]), p, d.ptr, c.ptr)
    assert e.value.status == -1
    with pytest.raises(GDFError) as e:
        gpu.radiusFilterPoints(d.ptr, 4, radius_filter_params((1, 0, 0), (0, 1, 1), 0.1, 1), o.ptr, c.ptr)
    assert e.value.status == -1


# ---- threshold ladder ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.LADDER_NAMES)
def test_threshold_ladder(gpu, name):
    s = S.get(name)
    keep, counts = ref_of(name, 1)
    cls = s["cls"]
    for idx in (s["base_idx"], s["partner_idx"]):             # kept / kept / dropped
        assert keep[idx][cls == 0].all() and keep[idx][cls == 1].all()
        assert not keep[idx][cls == 2].any()
        assert (counts[idx] == (cls < 2)).all()               # (pairs are isolated)
    assert len(s["pts"]) == 8192 and min((cls == c).sum() for c in range(3)) > 1300
    assert set(np.unique(s["base_side"])) == {-2, -1, 0, 1, 2} and set(np.unique(s["kind"])) == {0, 1, 2, 3}
    check_scene(gpu, name)


# ---- wave and tile edges ------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.WAVE_NAMES)
def test_wave_and_tile_edges(gpu, name):
    s = S.get(name)
    n = len(s["pts"])
    inside = R.inside_mask(s["pts"], s["lower"], s["upper"]).sum()
    assert 0.6 * n < inside < 0.9 * n                          # about a quarter outside
    assert 0 < ref_of(name, 4)[0].sum() < inside
    assert ref_of(name, 0)[0].sum() == inside and not ref_of(name, n)[0].any()
    check_scene(gpu, name)


# ---- crowded cell -------------------------------------------------------------------------------
def test_crowded_cell(gpu):
    s = S.get("crowded")
    cl = s["cluster"]
    assert cl.sum() == 3000
    k2999, c = ref_of("crowded", 2999)
    assert k2999[cl].all() and not k2999[~cl].any() and (c[cl] == 2999).all()
    assert not ref_of("crowded", 3000)[0].any()
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_plan
    cells, edge = radius_filter_plan(s["lower"], s["upper"], s["radius"])
    cell_of = np.floor((s["pts"][cl, :3].astype(np.float64) + 1) / edge.astype(np.float64))
    assert (cell_of == cell_of[0]).all()                       # one cell holds the cluster
    check_scene(gpu, "crowded")


# ---- plan extremes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.EXTREME_NAMES)
def test_plan_extremes(gpu, name):
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_plan
    s = S.get(name)
    lo, hi, r, want = S.PLAN_EXTREMES[name[len("extreme_"):]]
    assert radius_filter_plan(lo, hi, r)[0] == want
    inside = R.inside_mask(s["pts"], s["lower"], s["upper"])
    on_upper = inside & (s["pts"][:, :3] == np.asarray(hi, np.float32)).any(axis=1)
    k = ref_of(name, s["mins"][0])[0]
    assert 0 < inside.sum() < len(inside) and on_upper.sum() >= 3    # points on the clamped last cells
    assert k[on_upper].any() and 0 < k.sum()
    assert ref_of(name, s["mins"][-1])[0].sum() < k.sum()
    check_scene(gpu, name)


# ---- both paths of the cell counters' scan -------------------------------------------------------
def test_scenes_sit_on_both_sides_of_the_cell_scan_switch():
    """The scan of the cell counters runs in one block up to 8192 cells and in three launches above.
    Scenes of at most 4097 points already take both paths - wave_n4097_h1 (14^3 cells, run by
    test_wave_and_tile_edges) and extreme_both_caps (2^22 cells, run by test_plan_extremes) - so
    this test only pins their plans."""
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_plan
    assert "wave_n4097_h1" in S.WAVE_NAMES and "extreme_both_caps" in S.EXTREME_NAMES
    ncells = {}
    for name in ("wave_n4097_h1", "extreme_both_caps"):
        s = S.get(name)
        assert len(s["pts"]) <= 4097
        ncells[name] = int(np.prod(np.asarray(radius_filter_plan(s["lower"], s["upper"], s["radius"])[0],
                                              np.uint64)))
    assert ncells == {"wave_n4097_h1": 2744, "extreme_both_caps": 1 << 22}
    assert ncells["wave_n4097_h1"] <= 8192 < ncells["extreme_both_caps"]


# ---- more than one block of every kernel --------------------------------------------------------
def test_multi_block_paths(gpu):
    name = "multiblock_65537"
    s = S.get(name)
    keep, counts = ref_of(name, 4)                             # (the window form: n > 8192)
    assert len(s["pts"]) == 65537 and 4.0 < counts.mean() < 4.6
    assert 0.5 * 65537 < keep.sum() < 0.7 * 65537
    check_scene(gpu, name)


# ---- reuse --------------------------------------------------------------------------------------
def test_one_engine_reused_across_sizes_boxes_and_radii(gpu_engine_factory):
    eng = gpu_engine_factory()
    try:
        assert [len(S.get(n)["pts"]) for n in S.REUSE_NAMES] == [8191, 3, 4097]
        for name in S.REUSE_NAMES:
            m = 2 if name == "micro_n3" else 4
            assert 0 < ref_of(name, m)[0].sum() < len(S.get(name)["pts"])
            check_scene(eng, name, [m])
    finally:
        eng.close()


# ---- engine stage -------------------------------------------------------------------------------
def dense_cam(W, H, frame=0):
    from ros_gpu_depthmap_fusion_amd import synth
    cam = synth.make_camera(0, W, H)
    return (synth.dense_frame(cam, 0, frame), *cam.intrinsics(), cam.T_world, cam.T_crop)


def stage_case(gpu, source, box, radius, m, frac=None):
    src = gpu.downloadPoints() if source == "points" else gpu.downloadVoxelizedPoints()
    keep, _ = R.reference(src, box[0], box[1], radius, m)
    if frac is not None:
        assert abs(keep.mean() - frac[0]) < frac[1], (source, radius, m, keep.mean())
    assert 0 < keep.sum() < len(src)
    gpu.radiusFilter(box[0], box[1], radius, m, source=source)
    got = gpu.downloadFilteredPoints()
    assert gpu.filtered_count() == len(got) == keep.sum()
    assert np.array_equal(bits(got), bits(R.apply(src, keep))), (source, radius, m)
    return keep


@pytest.mark.parametrize("mode", ["stagewise", "processFrame"])
def test_engine_stage(gpu_engine_factory, mode):
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams, GDFError
    gpu = gpu_engine_factory()
    try:
        p = ComponentParams()
        cams = [dense_cam(160, 120)]
        gpu.clear()
        with pytest.raises(GDFError) as e:                     # before the frame's compaction
            gpu.radiusFilter(*BOX, 0.05, 4, source="points")
        assert e.value.status == -2
        if mode == "stagewise":
            stagewise_frame(gpu, cams, p)
        else:
            gpu.addDepthmap(*cams[0])
            gpu.processFrame(p)
        with pytest.raises(GDFError) as e:                     # no filter ran on this frame yet
            gpu.downloadFilteredPoints()
        assert e.value.status == -2
        assert (len(gpu.downloadPoints()), len(gpu.downloadVoxelizedPoints())) == (5091, 1028)
        stage_case(gpu, "points", BOX, 0.05, 4, (0.69, 0.01))
        stage_case(gpu, "points", BOX, 0.05, 16, (0.065, 0.005))
        stage_case(gpu, "voxelized", BOX, 0.15, 6, (0.50, 0.01))
        inside_cut = R.inside_mask(gpu.downloadPoints(), *BOX_CUT).sum()
        assert 0 < inside_cut < 5091
        for args in (("points", BOX_CUT, 0.05, 4), ("points", BOX_CUT, 0.05, 16),
                     ("voxelized", BOX_CUT, 0.15, 6)):
            stage_case(gpu, *args)
        ptr, cnt_ptr = gpu.device_filtered()
        assert ptr and cnt_ptr
        # a frame without voxelize has no voxelized source
        p2 = ComponentParams(enable_voxel_filter=False)
        gpu.clear()
        gpu.addDepthmap(*cams[0])
        gpu.processFrame(p2)
        with pytest.raises(GDFError) as e:
            gpu.radiusFilter(*BOX, 0.15, 6, source="voxelized")
        assert e.value.status == -2
        stage_case(gpu, "points", BOX, 0.05, 4, (0.69, 0.01))
    finally:
        gpu.close()


def test_stage_call_refuses_batches_and_emit_partition_frames(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd import hiprt
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams, GDFError
    gpu = gpu_engine_factory()
    try:
        p = ComponentParams()
        run_batch(gpu, p, [[dense_cam(160, 120, 0)], [dense_cam(160, 120, 1)]])
        for source in ("points", "voxelized"):
            with pytest.raises(GDFError) as e:                 # a multi-frame batch
                gpu.radiusFilter(*BOX, 0.05, 4, source=source)
            assert e.value.status == -2
        # a frame armed with the emit partition: over 1 Mi pixels its compaction writes the send
        # lists only (no compacted points to filter); a small one compacts and then partitions -
        # refused alike
        nparts = 3
        for W, H, by_compaction in ((1280, 960, True), (160, 120, False)):
            cap = W * H
            sp, srk, srs = (hiprt.DeviceArray(16 * cap), hiprt.DeviceArray(4 * cap),
                            hiprt.DeviceArray(4 * cap))
            cnt = hiprt.DeviceArray(8 * nparts)
            gpu.clear()
            gpu.addDepthmap(*dense_cam(W, H))
            gpu.set_emit_partition(nparts, sp.ptr, srk.ptr, srs.ptr, cap, cnt.ptr)
            gpu.processFrame(p, synchronous=True, defer_occupancy_grid=True, defer_voxelize=True)
            assert ("parts" in gpu.frame_kernels()["emit"]) == by_compaction
            with pytest.raises(GDFError) as e:
                gpu.radiusFilter(*BOX, 0.05, 4, source="points")
            assert e.value.status == -2
        # the engine is usable afterwards
        gpu.clear()
        gpu.addDepthmap(*dense_cam(160, 120))
        gpu.processFrame(p)
        stage_case(gpu, "points", BOX, 0.05, 4, (0.69, 0.01))
    finally:
        gpu.close()


# ---- armed --------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 3])
def test_armed_frames(gpu_engine_factory, depth):
    from oracle import OracleFusion
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams, GDFError
    gpu, orc = gpu_engine_factory(), OracleFusion()
    try:
        p = ComponentParams()
        gpu.set_pipeline_depth(depth)
        gpu.set_graphs(True)
        gpu.setRadiusFilter(True, *BOX, radius=0.15, min_neighbors=6)

        def frame(f, armed):
            cams = [dense_cam(160, 120, f)]
            for eng in (gpu, orc):
                eng.clear()
                eng.addDepthmap(*cams[0])
                eng.processFrame(p)
            compare_results(gpu, orc, tag=f"depth {depth} frame {f}")   # unfiltered outputs intact
            if not armed:
                with pytest.raises(GDFError) as e:
                    gpu.downloadFilteredPoints()
                assert e.value.status == -2
                return
            src = gpu.downloadVoxelizedPoints()
            keep, _ = R.reference(src, *BOX, 0.15, 6)
            assert 0 < keep.sum() < len(src)
            got = gpu.downloadFilteredPoints()
            assert np.array_equal(bits(got), bits(R.apply(src, keep))), (depth, f)

        for f in range(3):
            frame(f, True)
        if depth == 1:
            assert gpu.graph_stats()[1] >= 1                   # the later frames replayed
        # armed and a 2-frame batch: refused before anything is launched, engine usable afterwards
        with pytest.raises(GDFError) as e:
            run_batch(gpu, p, [[dense_cam(160, 120, 3)], [dense_cam(160, 120, 4)]])
        assert e.value.status == -2
        frame(3, True)
        # armed without the voxel filter: the points are the source
        gpu.clear()
        gpu.addDepthmap(*dense_cam(160, 120, 0))
        gpu.processFrame(ComponentParams(enable_voxel_filter=False))
        src = gpu.downloadPoints()
        keep, _ = R.reference(src, *BOX, 0.15, 6)
        assert 0 < keep.sum() < len(src)
        assert np.array_equal(bits(gpu.downloadFilteredPoints()), bits(R.apply(src, keep)))
        gpu.setRadiusFilter(False)                             # disabling stops it
        frame(4, False)
    finally:
        gpu.close()


def test_disarmed_engine_runs_no_filter(gpu_engine_factory):
    from oracle import OracleFusion
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams, GDFError
    gpu, orc = gpu_engine_factory(), OracleFusion()
    try:
        p = ComponentParams()
        gpu.setRadiusFilter(True, *BOX, radius=0.15, min_neighbors=6)
        gpu.setRadiusFilter(False)
        for f in range(2):
            for eng in (gpu, orc):
                eng.clear()
                eng.addDepthmap(*dense_cam(160, 120, f))
                eng.processFrame(p)
            compare_results(gpu, orc, tag=f"disarmed frame {f}")
            with pytest.raises(GDFError) as e:
                gpu.downloadFilteredPoints()
            assert e.value.status == -2
        with pytest.raises(GDFError) as e:                     # arming validates its parameters
            gpu.setRadiusFilter(True, *BOX, radius=0.0, min_neighbors=1)
        assert e.value.status == -1
    finally:
        gpu.close()


# ---- a 320 x 240 frame --------------------------------------------------------------------------
def test_qvga_frame(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    gpu = gpu_engine_factory()
    try:
        gpu.clear()
        gpu.addDepthmap(*dense_cam(320, 240))
        gpu.processFrame(ComponentParams())
        src = gpu.downloadPoints()
        assert len(src) == 25631
        keep, _ = R.window(src, *BOX, 0.05, 16)
        assert abs(keep.mean() - 0.78) < 0.01
        gpu.radiusFilter(*BOX, 0.05, 16, source="points")
        assert np.array_equal(bits(gpu.downloadFilteredPoints()), bits(R.apply(src, keep)))
    finally:
        gpu.close()


# ---- facade -------------------------------------------------------------------------------------
def test_facade_radius_filter(tmp_path, gpu_engine_factory):
    gpu_engine_factory  # (builds libgdf.so, checks a GPU is visible)
    exe = tmp_path / "facade_radius"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "facade_radius.cpp"), "-L", LIB, "-lgdf",
           "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    outd = tmp_path / "out"
    outd.mkdir()
    radius, m = 0.2, 6
    args = [str(radius), str(m)] + [str(v) for v in BOX_CUT[0] + BOX_CUT[1]]
    r = subprocess.run([str(exe), FIX, str(outd)] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    frames = int(open(os.path.join(FIX, "manifest.txt")).readline().split()[1])
    for f in range(frames):
        gold = np.fromfile(os.path.join(FIX, f"voxelized{f}.bin"), "<f4").reshape(-1, 3)
        vox4 = np.fromfile(outd / f"voxelized4_{f}.bin", "<f4").reshape(-1, 4)
        assert len(gold) > 0 and np.array_equal(bits(vox4[:, :3]), bits(gold)), f
        keep, _ = R.reference(vox4, *BOX_CUT, radius, m)
        inside = R.inside_mask(vox4, *BOX_CUT).sum()
        assert 0 < keep.sum() < inside < len(vox4), f
        got = np.fromfile(outd / f"filtered{f}.bin", "<f4").reshape(-1, 4)
        assert np.array_equal(bits(got), bits(R.apply(vox4, keep))), f"frame {f} m_points_filtered"
        byp = np.fromfile(outd / f"bypass{f}.bin", "<f4").reshape(-1, 4)
        assert np.array_equal(bits(byp), bits(vox4)), f"frame {f} bypassRadiusFilter"
