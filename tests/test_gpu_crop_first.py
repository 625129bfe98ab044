"""The px mask kernels evaluate the crop before the flying-pixel rings, and k_emit_px2 leaves an
empty segment after its first load round (bar: bit-exact against the oracle, as
test_gpu_round4.py).

The scenes are 448 pixels wide and run under GDF_SEG_ITEMS=256: rows in segments of 256 + 192,
the launch the px kernels take (k_mask_px_o8<2,256> / k_mask_px<2,256> + k_emit_px2<256>, thread
t of a segment at x0 owning the pixels x0 + t and x0 + t + 128).  Every case asserts FIRST, from
the engine's frame_kernels(), that those kernels ran: at their first width, 320 without the knob,
these scenes were one 320-pixel segment per row and ran k_mask<false,4> + k_emit - neither kernel
the file was written for.  That run is kept: every case runs its scene at 448 and then, without
the knob, at 320 x 32 (valid coverage of k_mask), with those kernels asserted too.

Hand-built depth maps (tests/px_scenes.py) put every shape of "nothing kept" where the two changes
act, and each scene ASSERTS FROM THE ORACLE'S STAGE ARRAYS, on the CPU, that it holds what it is
meant to hold (px_scenes.crop_scene_contents; without a GPU: test_px_scenes.py):

  1  a segment in the middle of a frame with every pixel valid and flying-clean but outside the
     crop (emit's early exit, mask's ring skip), as a row's first and as its last segment;
  2  the same for the first segment of a frame other than frame 0 of a batch and for the last
     segment of the batch's last frame - the two blocks with a duty that must not exit;
  3  a segment where wave 0's 128 pixels (columns 0..63, 128..191) are cropped and wave 1 keeps
     pixels - and the same in the row's 192-pixel segment (wave 0: 256..319, 384..447; wave 1:
     320..383, its second pixels past the row's end);
  4  kept pixels with depth-valid neighbours outside the crop within 4 pixels (>= 50): a cropped
     pixel still serves as a ring neighbour;
  5  a segment empty because its depth is zero, and one empty by the flying filter alone;
  6  a frame with the crop off (box +-1e9);
  7  a frame of two 448 x 16 cameras (the empty-segment exit behind the lane-ballot camera lookup,
     with and without the lookup by division);
  8  every scene in run mode (GDF_FORCE_RUNS=1) and in points mode;
  9  scene 3 also with GDF_NO_MASK_PACKED=1 (the scalar px form) and GDF_MASK_OCC8=0;
  10 the batch through gdf_set_emit_partition (k_emit_px2_parts<256>: empty segments under the
     partition's bookkeeping), 1 and 3 parts.

"Flying-clean" is asserted where the image allows it: columns 0..3 read their left neighbours
from the previous row's end, columns W-4..W-1 fail the filter's bounds test, and so do a frame's
first and last rows; the segments of 1 are clean in every column 4..W-5, those of 2 (row 0, row
H-1) are valid and outside the crop.

The last test pins k_mask's debug stage masks (bits 0, 1, 2) at the launch defaults.
"""
import numpy as np
import pytest

import px_scenes as S
from drive import (compare_frames, compare_results, engine_with, run_batch, stagewise_frame,
                   voxelize_parts_and_compare)
from oracle import OracleFusion
from px_scenes import cam_args
from ros_gpu_depthmap_fusion_amd import synth
from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams

pytestmark = pytest.mark.gpu

RUNS, POINTS = {"GDF_FORCE_RUNS": "1"}, {}
PACKED_OFF, OCC8_OFF = {"GDF_NO_MASK_PACKED": "1"}, {"GDF_MASK_OCC8": "0"}


@pytest.fixture(scope="module")
def Engine(gpu_engine_factory):
    return gpu_engine_factory


def layout(W):
    """(the segment knob, the kernels it must select) of the scenes at width W."""
    if W == 448:
        return S.PX_ENV, {"mask": S.K_MASK_O8, "emit": S.K_EMIT_PX}
    assert W == 320  # one 320-pixel segment per row: not the px kernels
    return {}, {"mask": S.K_MASK, "emit": S.K_EMIT}


def run_and_compare(Engine, sc, W, knobs, tag, frames=None, ref=None):
    env, want = layout(W)
    if W == 448 and knobs.get("GDF_MASK_OCC8") == "0":
        want = {"mask": S.K_MASK_PX, "emit": S.K_EMIT_PX}
    gpu = engine_with(Engine, **env, **knobs)
    for fr, rf in ([(sc.frames, sc.ref)] if frames is None else zip(frames, ref)):
        run_batch(gpu, sc.params, fr)
        assert gpu.frame_kernels() == want, (tag, gpu.frame_kernels(), gpu.tuning())
        compare_frames(gpu, rf, tag)


WIDTHS = (448, 320)  # the px layout, then the file's first width: k_mask + k_emit


@pytest.mark.parametrize("knobs", [POINTS, RUNS, PACKED_OFF, {**PACKED_OFF, **RUNS}, OCC8_OFF,
                                   {**OCC8_OFF, **RUNS}])
def test_batch_of_cropped_segments_matches_oracle(Engine, knobs):
    """Scenes 1-5 in one 3-frame batch of W x 32 frames (8, 9: run and points mode, the packed
    and the scalar px form, the 8-wave and the plain kernel)."""
    for W in WIDTHS:
        run_and_compare(Engine, S.crop_scene("batch", W), W, knobs, f"batch {W} {knobs}")


@pytest.mark.parametrize("knobs", [POINTS, RUNS])
def test_single_frames_of_the_batch_match_oracle(Engine, knobs):
    """The batch's frames one at a time (no frame_pt_start: an empty first segment may leave)."""
    for W in WIDTHS:
        sc = S.crop_scene("batch", W)
        run_and_compare(Engine, sc, W, knobs, f"frames {W} {knobs}",
                        frames=[[f] for f in sc.frames], ref=[[r] for r in sc.ref])


@pytest.mark.parametrize("knobs", [POINTS, RUNS])
def test_crop_off_matches_oracle(Engine, knobs):
    """Scene 6: a dense frame with the box at +-1e9 (everything the filter passes is kept)."""
    for W in WIDTHS:
        run_and_compare(Engine, S.crop_scene("nocrop", W), W, knobs, f"nocrop {W} {knobs}")


@pytest.mark.parametrize("knobs", [POINTS, RUNS, {"GDF_NO_SEG_UNIFORM": "1"},
                                   {"GDF_NO_SEG_UNIFORM": "1", **RUNS}])
def test_two_cameras_match_oracle(Engine, knobs):
    """Scene 7: two W x 16 cameras in one frame, the rows above and below the box empty; the
    segment's camera by division (equal cameras) and by the lane ballot."""
    for W in WIDTHS:
        run_and_compare(Engine, S.crop_scene("twocam", W), W, knobs, f"twocam {W} {knobs}")


@pytest.mark.parametrize("nparts", [1, 3])
def test_batch_through_the_emit_partition_matches_oracle(Engine, nparts):
    """10: the 3-frame batch with the send lists of a key-range partition written by the
    compaction itself (gdf_set_emit_partition: k_mask_px + k_emit_px2_parts<256>); every part
    voxelized on its own equals the oracle's voxel means and marks of each frame
    (test_gpu_round4.py::test_partition_runs_voxelize_runs_match_oracle's method)."""
    from ros_gpu_depthmap_fusion_amd import hiprt
    p, frames, ref = S.crop_scene("batch", 448)
    B = len(frames)
    gpu = engine_with(Engine, **S.PX_ENV)
    gpu.clear()
    for j, args in enumerate(frames):
        if j:
            gpu.nextFrameInBatch()
        for a in args:
            gpu.addDepthmap(*a)
    cap = 448 * S.CROP_H * B  # (the send buffers hold the frames' pixels before compaction)
    sp, srk, srs = hiprt.DeviceArray(16 * cap), hiprt.DeviceArray(4 * cap), hiprt.DeviceArray(4 * cap)
    cnt = hiprt.DeviceArray(8 * nparts)
    gpu.set_emit_partition(nparts, sp.ptr, srk.ptr, srs.ptr, cap, cnt.ptr)
    gpu.processFrame(p, synchronous=True, defer_occupancy_grid=True, defer_voxelize=True)
    assert gpu.frame_kernels() == {"mask": S.K_MASK_O8, "emit": S.K_EMIT_PARTS}, gpu.frame_kernels()
    gpu.synchronize()
    voxelize_parts_and_compare(gpu, nparts, B, sp, srk, srs, cnt, [r["vox"] for r in ref],
                               [r["keys"] for r in ref], ("crop-first batch", nparts))


def test_debug_stage_masks_at_launch_defaults(Engine):
    """set_debug: k_mask's per-pixel stage masks (bit 0 depth, bit 1 flying filter, bit 2 crop)
    of a 200 x 150 two-camera frame at the launch defaults (F = 4, no rot45) equal the oracle's -
    the crop-first order of the px kernels did not reach the kernel that writes them."""
    p = ComponentParams()
    gpu, orc = Engine(), OracleFusion(threads=4)
    gpu.set_debug(True)
    cams = synth.cameras(2, 200, 150)
    args = [cam_args(c, synth.dense_frame(c, k, 1)) for k, c in enumerate(cams)]
    stagewise_frame(gpu, args, p)
    stagewise_frame(orc, args, p)
    sm, st = gpu.stage_masks(), orc.stage_arrays()
    assert len(sm) == orc.num_points_total()
    depth_valid = np.concatenate([a[0].reshape(-1) != 0 for a in args])
    np.testing.assert_array_equal((sm & 1) != 0, depth_valid)
    np.testing.assert_array_equal((sm & 2) != 0, st["maskB"] != 0)
    np.testing.assert_array_equal((sm & 4) != 0, st["maskA"] != 0)
    assert (st["maskB"] != 0).any() and ((st["maskB"] != 0) & (st["maskA"] == 0)).any()
    compare_results(gpu, orc, tag="debug")
