"""The segmented radius outlier filter on the GPU (include/gdf_filter.h: one segment per frame of
a batch, over a sparse cell table) against its CPU restatement (tests/radius_segments_ref.py):
kept points (all four words), total, out_start and keep flags bit for bit, nothing written behind
the total or behind start[nseg].  Every composition's own property is asserted from the reference
in test_radius_segments_ref.py; here each case asserts that its answer is mixed."""
import functools

import numpy as np
import pytest

import radius_ref as R
import radius_scenes as S
import radius_segment_scenes as C
from drive import compare_frames, run_batch
from radius_segments_ref import apply_segments, reference_segments

pytestmark = pytest.mark.gpu

BOX = ((0, -8, -0.5), (10, 8, 2))
POISON = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gpu(gpu_engine_factory):
    eng = gpu_engine_factory()
    yield eng
    eng.close()


@functools.lru_cache(maxsize=None)
def ref_of(name, m):
    """The reference of a named composition, computed once and shared (read-only)."""
    c = C.get(name)
    keep, out_start = reference_segments(c["pts"], c["starts"], c["lower"], c["upper"], c["radius"], m)
    keep.setflags(write=False)
    out_start.setflags(write=False)
    return keep, out_start


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_segments(gpu, pts, starts, lower, upper, radius, m, with_keep=True):
    """gdf_radius_filter_segments over host arrays: (out points, total, out_start, keep flags)."""
    from ros_gpu_depthmap_fusion_amd import hiprt
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_params
    n, nseg = len(pts), len(starts) - 1
    d_in = hiprt.DeviceArray.from_numpy(pts) if n else hiprt.DeviceArray(16)
    d_st = hiprt.DeviceArray.from_numpy(np.asarray(starts, np.uint32))
    d_out = hiprt.DeviceArray.from_numpy(np.full((max(n, 1), 4), POISON, np.uint32))
    d_os = hiprt.DeviceArray.from_numpy(np.full(nseg + 2, POISON, np.uint32))
    d_cnt = hiprt.DeviceArray.from_numpy(np.full(1, POISON, np.uint32))
    d_keep = hiprt.DeviceArray.from_numpy(np.full(max(n, 1), 0xFF, np.uint8))
    gpu.radiusFilterSegments(d_in.ptr if n else 0, n, d_st.ptr, nseg,
                             radius_filter_params(lower, upper, radius, m), d_out.ptr if n else 0,
                             d_os.ptr, d_cnt.ptr, d_keep.ptr if with_keep else 0)
    gpu.synchronize()
    cnt = int(d_cnt.to_numpy(np.uint32, 1)[0])
    assert cnt <= n
    out = d_out.to_numpy(np.float32, 4 * max(n, 1)).reshape(-1, 4)
    os_ = d_os.to_numpy(np.uint32, nseg + 2)
    assert os_[nseg + 1] == POISON, "wrote past out_start[nseg]"
    keep = d_keep.to_numpy(np.uint8, max(n, 1))[:n]
    return out, cnt, os_[:nseg + 1], keep


def check(gpu, pts, starts, lower, upper, radius, m, keep_ref, out_start_ref, tag, with_keep=True):
    out, cnt, out_start, keep = run_segments(gpu, pts, starts, lower, upper, radius, m, with_keep)
    want = apply_segments(pts, keep_ref)
    end = int(starts[-1])
    assert cnt == len(want), (tag, m, cnt, len(want))
    assert np.array_equal(out_start, out_start_ref), (tag, m, out_start, out_start_ref)
    assert np.array_equal(bits(out[:cnt]), bits(want)), (tag, m, "points")
    assert (bits(out[cnt:]) == POISON).all(), (tag, m, "wrote past the total")
    if with_keep:
        assert np.array_equal(keep[:end], keep_ref.astype(np.uint8)), (tag, m, "keep flags")
    assert (keep[end:] == 0xFF).all(), (tag, m, "keep flags behind start[nseg]")


def check_comp(gpu, name, mins=None):
    c = C.get(name)
    for m in (mins or c["mins"]):
        keep, out_start = ref_of(name, m)
        check(gpu, c["pts"], c["starts"], c["lower"], c["upper"], c["radius"], m, keep, out_start, name)


def assert_mixed(name):
    c = C.get(name)
    keep = ref_of(name, c["mins"][0])[0]
    assert 0 < keep.sum() < len(keep), name


# ---- through gdf_radius_filter_segments ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_ref(name, m):
    s = S.get(name)
    keep, _ = R.reference(s["pts"], s["lower"], s["upper"], s["radius"], m)
    keep.setflags(write=False)
    return keep


@pytest.mark.parametrize("name", S.SMALL_NAMES)
def test_one_segment(gpu, name):
    s = S.get(name)
    n = len(s["pts"])
    for m in s["mins"]:
        keep = one_ref(name, m)
        check(gpu, s["pts"], [0, n], s["lower"], s["upper"], s["radius"], m, keep,
              np.array([0, keep.sum()], np.uint32), name)


def test_twin(gpu):
    assert_mixed("twin")
    check_comp(gpu, "twin")


def test_edges(gpu):
    c = C.get("edges")
    assert_mixed("edges")
    assert c["starts"][-1] < len(c["pts"])
    check_comp(gpu, "edges")


@pytest.mark.parametrize("nseg", [16, 64])
def test_many_segments(gpu, nseg):
    assert_mixed(f"many_{nseg}")
    check_comp(gpu, f"many_{nseg}")


def test_bad_nseg_and_aliasing(gpu):
    from ros_gpu_depthmap_fusion_amd import hiprt
    from ros_gpu_depthmap_fusion_amd.gdf import GDFError, radius_filter_params
    c = C.get("many_64")
    n = len(c["pts"])
    d = hiprt.DeviceArray.from_numpy(c["pts"])
    o = hiprt.DeviceArray(c["pts"].nbytes)
    st = hiprt.DeviceArray.from_numpy(np.concatenate([c["starts"], [n, n]]).astype(np.uint32))
    os_ = hiprt.DeviceArray(4 * 67)
    cnt = hiprt.DeviceArray(4)
    p = radius_filter_params(c["lower"], c["upper"], c["radius"], 1)
    for nseg in (65, 0):
        with pytest.raises(GDFError) as e:
            gpu.radiusFilterSegments(d.ptr, n, st.ptr, nseg, p, o.ptr, os_.ptr, cnt.ptr)
        assert e.value.status == -1
    with pytest.raises(GDFError) as e:                         # in == out
        gpu.radiusFilterSegments(d.ptr, n, st.ptr, 64, p, d.ptr, os_.ptr, cnt.ptr)
    assert e.value.status == -1
    with pytest.raises(GDFError) as e:                         # bad params
        gpu.radiusFilterSegments(d.ptr, n, st.ptr, 64, radius_filter_params((1, 0, 0), (0, 1, 1), 0.1, 1),
                                 o.ptr, os_.ptr, cnt.ptr)
    assert e.value.status == -1
    check_comp(gpu, "many_64", [1])                            # the engine is usable afterwards


def test_ladder_against_the_sparse_plans_faces(gpu):
    assert_mixed("ladder")
    check_comp(gpu, "ladder")


def test_many_distinct_cells(gpu):
    assert_mixed("lattice")
    check_comp(gpu, "lattice")


def test_crowded_cell(gpu):
    assert_mixed("crowded2")
    check_comp(gpu, "crowded2")


def test_one_engine_reused_across_sizes_boxes_and_radii(gpu_engine_factory):
    eng = gpu_engine_factory()
    try:
        assert [len(C.get(n)["pts"]) for n in C.REUSE_NAMES] == [8191, 31, 4097, 514]
        # the table's slots on both sides of the scan's switch from one block (<= 8192 words) to three
        # launches.  The expression mirrors rf_table_slots of csrc/gdf_filter.hpp (the library does not
        # export it): it pins the scenes' sizes, it would not notice a change of that function.
        slots = [max(1024, 1 << (2 * max(len(C.get(n)["pts"]), 512) - 1).bit_length()) for n in C.REUSE_NAMES]
        assert slots[3] == 2048 and slots[0] == 16384          # twin, lattice
        for rounds in range(2):                                # (a table left from a larger call)
            for name in C.REUSE_NAMES:
                assert_mixed(name)
                check_comp(eng, name, C.get(name)["mins"][:1])
    finally:
        eng.close()


def test_no_keep_buffer_and_empty_input(gpu):
    c = C.get("edges")
    keep, out_start = ref_of("edges", 1)
    check(gpu, c["pts"], c["starts"], c["lower"], c["upper"], c["radius"], 1, keep, out_start,
          "edges without flags", with_keep=False)
    none = np.zeros((0, 4), np.float32)                        # n_cap = 0 is valid
    out, cnt, os_, _ = run_segments(gpu, none, [0, 0, 0], c["lower"], c["upper"], c["radius"], 1)
    assert cnt == 0 and os_.tolist() == [0, 0, 0]


def test_start_table_is_clamped_and_made_monotone(gpu):
    """Starts above n_cap and decreasing starts: read as clamped to n_cap and non-decreasing."""
    c = C.get("twin")
    n = len(c["pts"])
    raw = np.array([0, 300, 257, 0xFFFFFFF0], np.uint32)
    seen = [0, 300, 300, n]
    keep, out_start = reference_segments(c["pts"], seen, c["lower"], c["upper"], c["radius"], 1)
    assert 0 < keep.sum() < n
    out, cnt, os_, flags = run_segments(gpu, c["pts"], raw, c["lower"], c["upper"], c["radius"], 1)
    assert cnt == keep.sum() and np.array_equal(os_, out_start)
    assert np.array_equal(flags, keep.astype(np.uint8))
    assert np.array_equal(bits(out[:cnt]), bits(apply_segments(c["pts"], keep)))


# ---- through the engine -------------------------------------------------------------------------
def dense_cam(W, H, frame=0):
    from ros_gpu_depthmap_fusion_amd import synth
    cam = synth.make_camera(0, W, H)
    return (synth.dense_frame(cam, 0, frame), *cam.intrinsics(), cam.T_world, cam.T_crop)


def batch_case(gpu, source, radius, m):
    """radiusFilterBatch on the batch the engine just ran against the reference over its own
    downloads and ranges."""
    ps, vs = gpu.batch_ranges()
    src, starts = ((gpu.downloadPoints(), ps) if source == "points" else
                   (gpu.downloadVoxelizedPoints(), vs))
    assert starts[0] == 0 and starts[-1] == len(src) and (np.diff(starts.astype(np.int64)) > 0).all()
    keep, out_start = reference_segments(src, starts, *BOX, radius, m)
    assert 0 < keep.sum() < len(src)
    gpu.radiusFilterBatch(*BOX, radius, m, source=source)
    got = gpu.downloadFilteredPoints()
    assert gpu.filtered_count() == len(got) == keep.sum()
    assert np.array_equal(bits(got), bits(apply_segments(src, keep))), (source, radius, m)
    assert np.array_equal(gpu.filtered_ranges(), out_start), (source, gpu.filtered_ranges(), out_start)
    ptr, nseg = gpu.device_filtered_ranges()
    assert ptr and nseg == len(starts) - 1
    return keep, src, starts


@pytest.mark.parametrize("frames", [(0, 1), (0, 1, 2), (0, 0)])
def test_engine_batches(gpu_engine_factory, frames):
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    gpu = gpu_engine_factory()
    try:
        run_batch(gpu, ComponentParams(), [[dense_cam(160, 120, f)] for f in frames])
        for source, radius, m in (("points", 0.05, 4), ("points", 0.05, 16), ("voxelized", 0.15, 6)):
            keep, src, starts = batch_case(gpu, source, radius, m)
            if frames == (0, 0) and source == "points":        # per frame, not merged
                merged, _ = R.reference(src, *BOX, radius, m)
                assert (merged & ~keep).any()
    finally:
        gpu.close()


def test_one_frame_batch_equals_the_single_frame_filter(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    gpu = gpu_engine_factory()
    try:
        gpu.clear()
        gpu.addDepthmap(*dense_cam(160, 120))
        gpu.processFrame(ComponentParams())
        for source, radius, m in (("points", 0.05, 4), ("voxelized", 0.15, 6)):
            gpu.radiusFilter(*BOX, radius, m, source=source)
            want = gpu.downloadFilteredPoints()
            assert gpu.filtered_ranges().tolist() == [0, len(want)]
            gpu.radiusFilterBatch(*BOX, radius, m, source=source)
            got = gpu.downloadFilteredPoints()
            assert 0 < len(want) and np.array_equal(bits(got), bits(want)), source
            assert gpu.filtered_ranges().tolist() == [0, len(want)]
    finally:
        gpu.close()


def test_batch_stage_refusals(gpu_engine_factory):
    from ros_gpu_depthmap_fusion_amd import hiprt
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams, GDFError
    gpu = gpu_engine_factory()
    try:
        p = ComponentParams()
        gpu.clear()
        for source in ("points", "voxelized"):                 # before the frame
            with pytest.raises(GDFError) as e:
                gpu.radiusFilterBatch(*BOX, 0.05, 4, source=source)
            assert e.value.status == -2
        with pytest.raises(GDFError) as e:                     # no filter ran: no ranges
            gpu.filtered_ranges()
        assert e.value.status == -2
        frames = [[dense_cam(160, 120, 0)], [dense_cam(160, 120, 1)]]
        run_batch(gpu, ComponentParams(enable_voxel_filter=False), frames)
        with pytest.raises(GDFError) as e:                     # a batch without voxelize
            gpu.radiusFilterBatch(*BOX, 0.15, 6, source="voxelized")
        assert e.value.status == -2
        batch_case(gpu, "points", 0.05, 4)
        nparts, cap = 3, 160 * 120                             # an emit-partition frame
        sp, srk, srs = hiprt.DeviceArray(16 * cap), hiprt.DeviceArray(4 * cap), hiprt.DeviceArray(4 * cap)
        cnt = hiprt.DeviceArray(8 * nparts)
        gpu.clear()
        gpu.addDepthmap(*dense_cam(160, 120))
        gpu.set_emit_partition(nparts, sp.ptr, srk.ptr, srs.ptr, cap, cnt.ptr)
        gpu.processFrame(p, synchronous=True, defer_occupancy_grid=True, defer_voxelize=True)
        with pytest.raises(GDFError) as e:
            gpu.radiusFilterBatch(*BOX, 0.05, 4, source="points")
        assert e.value.status == -2
        run_batch(gpu, p, frames)                              # the engine is usable afterwards
        batch_case(gpu, "voxelized", 0.15, 6)
    finally:
        gpu.close()


@functools.lru_cache(maxsize=None)
def oracle_frames(frames):
    """The oracle's per-frame results of consecutive batches (the grid's history carried on)."""
    import px_scenes
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    ref = px_scenes.run_oracle([[dense_cam(160, 120, f)] for f in frames], ComponentParams())
    return ref


@pytest.mark.parametrize("depth", [1, 3])
def test_armed_batches(gpu_engine_factory, depth):
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams, GDFError
    gpu = gpu_engine_factory()
    try:
        p = ComponentParams()
        gpu.set_pipeline_depth(depth)
        gpu.set_graphs(True)
        gpu.setRadiusFilterBatch(True, *BOX, radius=0.15, min_neighbors=6)
        ref = oracle_frames((0, 1, 0, 1, 0, 1, 2, 3, 4, 0, 1, 0, 1))

        def batch(k, armed):
            run_batch(gpu, p, [[dense_cam(160, 120, 0)], [dense_cam(160, 120, 1)]])
            first = 2 * k if k < 3 else 2 * k + 3              # (three single frames after batch 2)
            compare_frames(gpu, ref[first:first + 2], f"depth {depth} batch {k}")   # unfiltered outputs intact
            if not armed:
                with pytest.raises(GDFError) as e:
                    gpu.downloadFilteredPoints()
                assert e.value.status == -2
                return
            src, (_, vs) = gpu.downloadVoxelizedPoints(), gpu.batch_ranges()
            keep, out_start = reference_segments(src, vs, *BOX, 0.15, 6)
            assert 0 < keep.sum() < len(src)
            assert np.array_equal(bits(gpu.downloadFilteredPoints()), bits(apply_segments(src, keep))), k
            assert np.array_equal(gpu.filtered_ranges(), out_start)

        for k in range(3):
            batch(k, True)
        # single frames stay with the single-frame arm (unset: no filter); their graphs (a batch
        # launches directly) are captured and replayed as ever
        for f in (2, 3, 4):
            run_batch(gpu, p, [[dense_cam(160, 120, f)]])
            compare_frames(gpu, [ref[4 + f]], f"depth {depth} single {f}")
            with pytest.raises(GDFError) as e:
                gpu.downloadFilteredPoints()
            assert e.value.status == -2
        if depth == 1:
            assert gpu.graph_stats()[1] >= 1                   # replays still counted
        # a deferred-voxelize batch while armed: refused before any launch
        with pytest.raises(GDFError) as e:
            gpu.clear()
            gpu.addDepthmap(*dense_cam(160, 120, 0))
            gpu.nextFrameInBatch()
            gpu.addDepthmap(*dense_cam(160, 120, 1))
            gpu.processFrame(p, defer_occupancy_grid=True, defer_voxelize=True)
        assert e.value.status == -2
        # the batch arm leaves single frames alone
        gpu.clear()
        gpu.addDepthmap(*dense_cam(160, 120, 0))
        gpu.processFrame(ComponentParams(enable_voxel_filter=False))
        with pytest.raises(GDFError) as e:
            gpu.downloadFilteredPoints()
        assert e.value.status == -2
        # armed without the voxel filter: the points are the source
        run_batch(gpu, ComponentParams(enable_voxel_filter=False),
                  [[dense_cam(160, 120, 0)], [dense_cam(160, 120, 1)]])
        src, (ps, _) = gpu.downloadPoints(), gpu.batch_ranges()
        keep, out_start = reference_segments(src, ps, *BOX, 0.15, 6)
        assert 0 < keep.sum() < len(src)
        assert np.array_equal(bits(gpu.downloadFilteredPoints()), bits(apply_segments(src, keep)))
        gpu.setRadiusFilterBatch(False)                        # disarming stops it
        batch(3, False)
        # the single-frame arm alone still refuses a batch
        gpu.setRadiusFilter(True, *BOX, radius=0.15, min_neighbors=6)
        with pytest.raises(GDFError) as e:
            run_batch(gpu, p, [[dense_cam(160, 120, 0)], [dense_cam(160, 120, 1)]])
        assert e.value.status == -2
        gpu.setRadiusFilter(False)
        batch(4, False)
        with pytest.raises(GDFError) as e:                     # arming validates its parameters
            gpu.setRadiusFilterBatch(True, *BOX, radius=0.0, min_neighbors=1)
        assert e.value.status == -1
    finally:
        gpu.close()
