"""The two-pixel compaction kernels (k_mask_px_o8<2,256> / k_mask_px<2,256> + k_emit_px2<256>, and
k_mask_px<2,640> + k_emit_px2<640>) against the oracle at small shapes (bar: bit-exact, as
test_gpu_round4.py).  The scenes and what each must contain are tests/px_scenes.py's (checked
without a GPU by test_px_scenes.py):

  widths   a dense synthetic W x 24 frame at W = 193 (one segment, second pixels in lanes 0..64
           only), 199 (odd), 256, 385 (tail 129), 391 (odd: row starts step by 14 bytes modulo
           16), 448 (tail 192), 449 (tail 193), 512, 577 (three segments, tail 65) - at the
           launch defaults, and with a flying-pixel threshold under which the row-start columns
           0..3 (kRowStart: left neighbours at the previous row's end) keep points;
  heights  391 x H, H = 1, 4, 5, 8, 9, 12: a single camera (nothing kept up to H = 8), and the
           second of two equal cameras, whose rows 0..3 (the kGeneral rows) keep points with
           neighbours in the first camera;
  mixed    199 x 7 (and x 9), 448 x 12, 96 x 10 in one frame: an odd pixel count before the next
           staged map, 128-pixel segments in the 256-thread launch, the camera lookup by ballot;
  device   the 391 x 12 map at byte offsets 2, 6, 14 modulo 16 inside an allocation whose other
           pixels are a valid depth;
  empty    448 x 16 batches with empty frames (1 and 3, or all four);
  replay   one frame four times: direct launch, graph capture, replays;
  640      1211 x 720 and two cameras 1211 x 400 with whole row ranges cropped, no knob.

Every case asserts the kernels the engine ran (frame_kernels) FIRST: the small scenes reach the px
kernels only under GDF_SEG_ITEMS=256, and a width outside 193..256 / 385..512 / 577..768 would run
k_mask + k_emit and pass for the wrong reason.  Then points (order included), voxel keys, voxel
means, grid and history bit for bit, in points mode and under GDF_FORCE_RUNS=1.
"""
import numpy as np
import pytest

import px_scenes as S
from drive import compare_frames, engine_with, run_batch

pytestmark = pytest.mark.gpu

RUNS, POINTS = {"GDF_FORCE_RUNS": "1"}, {}
MODES = [POINTS, RUNS]
PX_O8 = {"mask": S.K_MASK_O8, "emit": S.K_EMIT_PX}
PX = {"mask": S.K_MASK_PX, "emit": S.K_EMIT_PX}
P640 = {"mask": S.K_MASK_640, "emit": S.K_EMIT_640}


@pytest.fixture(scope="module")
def Engine(gpu_engine_factory):
    return gpu_engine_factory


def px_engine(Engine, knobs):
    return engine_with(Engine, **S.PX_ENV, **knobs)


def check(gpu, sc, want, tag):
    """One processFrame over the scene's frames: the kernels first, then every output."""
    run_batch(gpu, sc.params, sc.frames)
    assert gpu.frame_kernels() == want, (tag, gpu.frame_kernels(), gpu.tuning())
    compare_frames(gpu, sc.ref, tag)


def test_frame_kernels_reports_the_path(Engine):
    """frame_kernels(): empty before any frame; the px pair under the knob at 448 and - the same
    engine, the next frame - the fallback pair at 257 and 320 (segments of 192), which is what a
    px test at a wrong width would silently run; k_mask_px<2,256> under GDF_MASK_OCC8=0; k_mask
    for 448 without the knob; empty again after a frame without depth maps."""
    from ros_gpu_depthmap_fusion_amd import synth
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    p = ComponentParams()

    def frame(gpu, W):
        cam = synth.make_camera(0, W, 24)
        run_batch(gpu, p, [[S.cam_args(cam, synth.dense_frame(cam, 0, 0))]])
        return gpu.frame_kernels()

    gpu = px_engine(Engine, {})
    assert gpu.frame_kernels() == {}
    assert frame(gpu, 448) == PX_O8
    assert frame(gpu, 257) == {"mask": S.K_MASK, "emit": S.K_EMIT}
    assert frame(gpu, 320) == {"mask": S.K_MASK, "emit": S.K_EMIT}
    assert frame(gpu, 512) == PX_O8
    assert frame(px_engine(Engine, {"GDF_MASK_OCC8": "0"}), 448) == PX
    plain = Engine()
    assert frame(plain, 448) == {"mask": S.K_MASK, "emit": S.K_EMIT}
    # a frame of rollbuffer points only: no depth compaction
    lidar = synth.make_camera(1, 64, 48)
    pts = synth.back_project(lidar, synth.dense_frame(lidar, 1, 0))
    eye = np.eye(4, dtype=np.float32)
    plain.addPointSequence(pts, *synth.sequence_time(0), synth.move_transform(0))
    plain.clear()
    plain.processFrame(p, T_world_move=eye, T_crop_move=eye)
    assert plain.frame_kernels() == {}


@pytest.mark.parametrize("knobs", MODES + [{"GDF_MASK_OCC8": "0"}, {"GDF_NO_MASK_PACKED": "1"}])
@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("W", S.WIDTHS)
def test_widths_match_oracle(Engine, W, wrap, knobs):
    """Row tails of every kind, odd widths and every 16-byte alignment of a row start (the band's
    chunk loads), and the kRowStart wrap columns; the 8-wave and the plain kernel, the packed
    and the scalar form."""
    want = PX if knobs.get("GDF_MASK_OCC8") == "0" else PX_O8
    check(px_engine(Engine, knobs), S.width_scene(W, wrap), want, f"W={W} wrap={wrap} {knobs}")


@pytest.mark.parametrize("knobs", MODES)
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("H", S.HEIGHTS)
def test_heights_match_oracle(Engine, H, two, knobs):
    """Fewer rows than the band (H < 9), and the rows 0..3 of a second camera, which read the
    first camera's last rows by linear index."""
    sc = S.height_scene(H, two)
    gpu = px_engine(Engine, knobs)
    check(gpu, sc, PX_O8, f"H={H} two={two} {knobs}")
    if not two and H <= 8:  # nothing kept: no points, the grid as it was created
        assert len(gpu.downloadPoints()) == 0 and len(gpu.downloadVoxelizedPoints()) == 0
        assert not gpu.downloadVoxelOccupancyGrid().any() and not gpu.historic_grid().any()


@pytest.mark.parametrize("knobs", MODES + [{"GDF_NO_SEG_UNIFORM": "1"},
                                           {"GDF_NO_SEG_UNIFORM": "1", **RUNS}])
@pytest.mark.parametrize("h0", [7, 9])
def test_mixed_cameras_match_oracle(Engine, h0, knobs):
    """Cameras of three widths in one frame: the second staged map starts at a 2-byte-odd
    offset, the third runs 128-pixel segments in the 256-thread launch."""
    check(px_engine(Engine, knobs), S.mixed_scene(h0), PX_O8, f"mixed h0={h0} {knobs}")


@pytest.mark.parametrize("knobs", MODES)
@pytest.mark.parametrize("off", S.DEVICE_OFFSETS)
def test_device_maps_at_unaligned_addresses(Engine, off, knobs):
    """The 391 x 12 map through a device pointer `off` bytes past a 16-byte boundary, 256 bytes
    and more inside an allocation filled with 3000 mm - a valid depth inside the box: a band load
    that took a pixel from outside the map would change the result, and none leaves the
    allocation."""
    from ros_gpu_depthmap_fusion_amd import hiprt
    sc = S.device_scene()
    (depth, scale, fx, fy, cx, cy, Tw, Tc), = sc.frames[0]
    H, W = depth.shape
    lead = 128 + off // 2  # pixels before the map
    buf = np.full(lead + H * W + 128, 3000, np.uint16)
    buf[lead:lead + H * W] = depth.reshape(-1)
    dev = hiprt.DeviceArray.from_numpy(buf)
    ptr = dev.ptr + 2 * lead
    assert ptr % 16 == off and 2 * lead >= 64 and buf.nbytes - 2 * (lead + H * W) >= 64
    gpu = px_engine(Engine, knobs)
    gpu.clear()
    gpu.addDepthmapDevice(ptr, W, H, scale, fx, fy, cx, cy, Tw, Tc)
    gpu.processFrame(sc.params)
    assert gpu.frame_kernels() == PX_O8, (off, gpu.frame_kernels())
    compare_frames(gpu, sc.ref, f"device +{off} {knobs}")
    gpu.synchronize()
    dev.close()


@pytest.mark.parametrize("knobs", MODES)
@pytest.mark.parametrize("all_empty", [False, True])
def test_empty_frames_in_a_batch_match_oracle(Engine, all_empty, knobs):
    """Frames of zero depth in a 4-frame batch (frames 1 and 3, or all): their first segments'
    blocks store frame_pt_start and the last block the count, though they hold no point."""
    sc = S.empty_batch_scene(all_empty)
    gpu = px_engine(Engine, knobs)
    check(gpu, sc, PX_O8, f"empty all={all_empty} {knobs}")
    ps, vs = gpu.batch_ranges()
    n = [len(r["points"]) for r in sc.ref]
    assert list(np.diff(ps)) == n and [len(r["vox"]) for r in sc.ref] == list(np.diff(vs))
    assert len(gpu.downloadPoints()) == sum(n)
    for j, r in enumerate(sc.ref):
        assert np.array_equal(gpu.downloadBatchVoxelOccupancyGrid(j), r["grid"]), j


@pytest.mark.parametrize("knobs", MODES)
def test_replayed_frames_match_oracle(Engine, knobs):
    """The same 449 x 24 frame four times on one engine: launched directly, captured, replayed -
    the kernels reported and every output of each frame."""
    sc = S.replay_scene()
    gpu = px_engine(Engine, knobs)
    for j, args in enumerate(sc.frames):
        run_batch(gpu, sc.params, [args])
        assert gpu.frame_kernels() == PX_O8, (j, gpu.frame_kernels())
        compare_frames(gpu, [sc.ref[j]], f"replay {j} {knobs}")
    captures, replays = gpu.graph_stats()
    assert captures >= 1 and replays >= 1, (captures, replays)


@pytest.mark.parametrize("knobs", MODES)
@pytest.mark.parametrize("ncams", [1, 2])
def test_640_forms_match_oracle(Engine, ncams, knobs):
    """The 640-pixel forms at their product shape (no segment knob): 1211-pixel rows in segments
    of 640 + 571, at least 1024 segments, more than 30 % of them emptied by the crop alone, the
    frame's last among them."""
    check(engine_with(Engine, **knobs), S.p640_scene(ncams), P640, f"640 x{ncams} {knobs}")
