"""The compaction above kFusedPrefixSegs = 4096 segments against the oracle (bar: bit-exact, as
test_gpu_round4.py): k_mask stores raw segment counts and adds them to the totals of its group of
64 segments, k_emit sums the totals of the groups before its own and the raw counts before its own
inside its group (gdf_kernels.hip store_seg_counts / group_partials).  The totals are
accumulators that the first sort pass of the frame's voxelize clears - or the engine, where no
voxelize followed a compaction.

The path needs more than 4096 segments, so the shapes are narrow and tall:

  px        8 frames of 256 x 521 under GDF_SEG_ITEMS=256: 4168 one-row segments, 65 full groups
            and a last group of 8; 521 is no multiple of 64, so frames 1.. start mid-group;
  general   8 frames of 64 x 521 under GDF_SEG_ITEMS=64: the same segment count through
            k_mask + k_emit;
  empty     both shapes with rows 300..449 of frame 2 at depth 0 (whole groups without a kept
            pixel and without an add, inside the rows the other frames keep) and the last frame
            entirely empty (the last block still writes the counts);
  replay    one 256 x 4200 frame four times on one engine (direct launch, capture, replays): what
            totals that are not zero again at the next launch would break;
  stages    applyPointMask twice on one engine without a voxelize in between (the engine clears
            the totals itself), then a processFrame;
  scans     GDF_NO_GROUP_SCAN=1 on the px shape (the scan launches and seg_offsets);
  groups    GDF_GROUP_BLOCKS=1024 on the px shape: the group phase's blocks walk several tiles.

Every case asserts the kernels the engine ran (frame_kernels) FIRST, then points (order
included), voxel keys, voxel means, grid and history bit for bit, with nothing set, under
GDF_FORCE_RUNS=1 and - these shapes hold more than 1 Mi pixels, where the engine sorts runs by
itself - under GDF_NO_RUNS=1 for the points path.
"""
import functools

import numpy as np
import pytest

import px_scenes as S
from drive import compare_frames, engine_with, run_batch
from ros_gpu_depthmap_fusion_amd import synth
from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams

pytestmark = pytest.mark.gpu

MODES = [{}, {"GDF_FORCE_RUNS": "1"}, {"GDF_NO_RUNS": "1"}]
PX_O8 = {"mask": S.K_MASK_O8, "emit": S.K_EMIT_PX}
PLAIN = {"mask": S.K_MASK, "emit": S.K_EMIT}
SEGS, GROUP = 4096, 64  # kFusedPrefixSegs, kScanGroup (gdf_device.hpp)
H, B = 521, 8
ZERO_ROWS = (300, 450)


@pytest.fixture(scope="module")
def Engine(gpu_engine_factory):
    return gpu_engine_factory


def kept_per_segment(sc):
    """Kept pixels of every segment of the batch, in segment order (one-segment rows)."""
    return np.concatenate([A.sum(axis=1) for f in range(len(sc.frames)) for A, _ in sc.masks(f)])


@functools.lru_cache(maxsize=None)
def batch_scene(W, empty=False):
    """B dense W x 521 frames (W = one segment); empty: frame 2 with rows 300..450 at depth 0,
    and the last frame all zero."""
    cam = synth.make_camera(0, W, H)
    maps = [synth.dense_frame(cam, 0, j) for j in range(B)]
    if empty:
        maps[2] = maps[2].copy()
        maps[2][ZERO_ROWS[0]:ZERO_ROWS[1]] = 0
        maps[B - 1] = np.zeros((H, W), np.uint16)
    frames = [[S.cam_args(cam, d)] for d in maps]
    p = ComponentParams()
    sc = S.Scene(p, frames, S.run_oracle(frames, p))
    n = kept_per_segment(sc)
    ngroups = (len(n) + GROUP - 1) // GROUP
    assert len(n) == B * H > SEGS and len(n) % GROUP and H % GROUP
    per_group = np.add.reduceat(n, np.arange(0, len(n), GROUP))
    assert len(per_group) == ngroups
    # segments with and without points inside one group, and groups that hold points after
    # groups that hold points (a sum over more than one total)
    mixed = [g for g in range(ngroups) if 0 < np.count_nonzero(n[g * GROUP:(g + 1) * GROUP]) < GROUP]
    assert mixed and np.count_nonzero(per_group) >= 8
    if empty:
        g0, g1 = (2 * H + ZERO_ROWS[0] + GROUP - 1) // GROUP, (2 * H + ZERO_ROWS[1]) // GROUP
        assert g1 > g0 and not per_group[g0:g1].any()  # a whole group inside the zeroed rows
        # ... behind kept rows of its own frame (W = 256: and before some) and before later frames'
        assert n[2 * H:2 * H + ZERO_ROWS[0]].any() and n[3 * H:].any()
        assert W != 256 or n[2 * H + ZERO_ROWS[1]:3 * H].any()
        assert not n[(B - 1) * H:].any() and len(sc.ref[B - 1]["points"]) == 0
    else:
        assert all(len(r["points"]) > 1000 for r in sc.ref)
    return sc


@functools.lru_cache(maxsize=None)
def tall_scene(n=4):
    """One dense 256 x 4200 frame n times, as single frames (the oracle carries the history)."""
    cam = synth.make_camera(0, 256, 4200)
    frames = [[S.cam_args(cam, synth.dense_frame(cam, 0, 0))]] * n
    p = ComponentParams()
    sc = S.Scene(p, frames, S.run_oracle(frames, p))
    assert 4200 > SEGS and len(sc.ref[0]["points"]) > 10000
    return sc


def check(gpu, sc, want, tag):
    run_batch(gpu, sc.params, sc.frames)
    assert gpu.frame_kernels() == want, (tag, gpu.frame_kernels(), gpu.tuning())
    compare_frames(gpu, sc.ref, tag)


@pytest.mark.parametrize("knobs", MODES)
def test_px_kernels_match_oracle(Engine, knobs):
    check(engine_with(Engine, **S.PX_ENV, **knobs), batch_scene(256), PX_O8, f"px {knobs}")


@pytest.mark.parametrize("knobs", MODES)
def test_general_kernels_match_oracle(Engine, knobs):
    check(engine_with(Engine, GDF_SEG_ITEMS="64", **knobs), batch_scene(64), PLAIN, f"general {knobs}")


@pytest.mark.parametrize("knobs", MODES)
@pytest.mark.parametrize("W", [256, 64])
def test_empty_groups_and_empty_last_frame(Engine, W, knobs):
    """Groups that receive no add keep the zero they started from; the last frame's blocks hold
    nothing, and its last block still writes the counts and the frame ranges."""
    want = PX_O8 if W == 256 else PLAIN
    gpu = engine_with(Engine, GDF_SEG_ITEMS=str(W), **knobs)
    sc = batch_scene(W, True)
    check(gpu, sc, want, f"empty W={W} {knobs}")
    ps, _ = gpu.batch_ranges()
    assert list(np.diff(ps)) == [len(r["points"]) for r in sc.ref]
    # ... and the same engine's next batch starts from zero totals again (its grid carries the
    # first batch's history, which the scene's oracle run does not: the compaction's outputs)
    full = batch_scene(W)
    run_batch(gpu, full.params, full.frames)
    assert gpu.frame_kernels() == want
    pts, keys = gpu.downloadPoints(), gpu.downloadVoxelCoords()
    assert list(np.diff(gpu.batch_ranges()[0])) == [len(r["points"]) for r in full.ref]
    assert np.array_equal(pts.view(np.uint32), np.concatenate([r["points"] for r in full.ref]).view(np.uint32))
    assert np.array_equal(keys, np.concatenate([r["keys"] for r in full.ref]))


@pytest.mark.parametrize("knobs", MODES)
def test_replayed_frames_match_oracle(Engine, knobs):
    """Direct launch, capture, two replays of one 4200-segment frame: every repetition equals the
    oracle (totals left over from the launch before would shift every point behind group 0)."""
    sc = tall_scene()
    gpu = engine_with(Engine, **S.PX_ENV, **knobs)
    for j, args in enumerate(sc.frames):
        run_batch(gpu, sc.params, [args])
        assert gpu.frame_kernels() == PX_O8, (j, gpu.frame_kernels())
        compare_frames(gpu, [sc.ref[j]], f"replay {j} {knobs}")
    captures, replays = gpu.graph_stats()
    assert captures >= 1 and replays >= 1, (captures, replays)


def stages_to_mask(gpu, cams, p):
    """The component's stage calls of a depth-only frame up to applyPointMask (drive.py)."""
    gpu.clear()
    for c in cams:
        gpu.addDepthmap(*c)
    gpu.preparePointAndMaskBuffers()
    gpu.uploadDepthmaps()
    gpu.convertDepthmaps()
    gpu.filterFlyingPixels(p.flying_filter_size, p.flying_threshold, p.flying_rot45)
    gpu.cropPoints(p.crop_min, p.crop_max)
    gpu.applyPointMask()


@pytest.mark.parametrize("knobs", MODES)
def test_compactions_without_a_voxelize_between(Engine, knobs):
    """applyPointMask twice in a row: no sort pass ran in between, the engine clears the totals
    before the second compaction; then a fused frame on the same engine."""
    sc = tall_scene()
    gpu = engine_with(Engine, **S.PX_ENV, **knobs)
    want = sc.ref[0]["points"].view(np.uint32)
    for j in range(2):
        stages_to_mask(gpu, sc.frames[0], sc.params)
        assert gpu.frame_kernels() == PX_O8, (j, gpu.frame_kernels())
        got = gpu.downloadPoints()
        assert len(got) == len(want) and np.array_equal(got.view(np.uint32), want), (j, knobs)
    check(gpu, S.Scene(sc.params, sc.frames[:1], sc.ref[:1]), PX_O8, f"stages {knobs}")


@pytest.mark.parametrize("knobs", MODES)
def test_scan_launches_still_agree(Engine, knobs):
    check(engine_with(Engine, **S.PX_ENV, GDF_NO_GROUP_SCAN="1", **knobs), batch_scene(256), PX_O8,
          f"scan launches {knobs}")


@pytest.mark.parametrize("knobs", MODES)
def test_group_phase_blocks_walk_several_tiles(Engine, knobs):
    """More than 262144 pixels of capacity: the group phase counts group starts per tile
    (k_group_count); 1024 blocks walk the capacity's tiles."""
    check(engine_with(Engine, **S.PX_ENV, GDF_GROUP_BLOCKS="1024", **knobs), batch_scene(256), PX_O8,
          f"group blocks {knobs}")
