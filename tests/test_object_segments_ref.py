"""The segmented partition and the segmented voxel table restated on the CPU
(tests/object_segments_ref.py): the two forms of each rule agree, each equals the unsegmented rule
applied to every slice (the defining properties of DESIGN.md §15), every built scene
(tests/object_segment_scenes.py) holds the case it was built for, and the three frames of the facade
fixture as one 3-segment input give the fixture's voxel ranges and key lists.  No GPU."""
import os

import numpy as np
import pytest

import object_points_ref as opr
import object_segment_scenes as scenes
import object_segments_ref as osr
import voxel_ref
import voxel_table_ref as vtr
from test_voxel_table_ref import fixture_frame, fixture_grid, manifest

NONE = osr.NONE
PARTITION = scenes.partition_scenes()
TABLE = scenes.table_scenes()
BIG = 1 << 20     # groups above which the plain loops are skipped (a list per group)


def test_the_binding_declares_the_segmented_calls():
    from ros_gpu_depthmap_fusion_amd.gdf import EXPORTED, Segmenter
    for name in ("group_points_segments", "voxel_table_segments", "object_points_batch",
                 "object_voxels_batch", "group_segments", "voxel_segments", "group_segments_device",
                 "voxel_segments_device"):
        assert callable(getattr(Segmenter, name)), name
    for sym in ("gdf_seg_group_points_segments", "gdf_seg_voxel_table_segments",
                "gdf_seg_object_points_batch", "gdf_seg_object_voxels_batch",
                "gdf_seg_get_group_segments", "gdf_seg_get_device_group_segments",
                "gdf_seg_get_voxel_segments", "gdf_seg_get_device_voxel_segments"):
        assert sym in EXPORTED, sym


def test_clamped_starts_in_both_forms():
    for starts, n, want in (([0, 5, 9], 9, [0, 5, 9]), ([0, 200, 100, 300, 250, 500], 500, [0, 200, 200, 300, 300, 500]),
                            ([0, 200, 501, 1 << 31, NONE], 500, [0, 200, 500, 500, 500]),
                            ([70, 200, 333, 480], 500, [70, 200, 333, 480]), ([3, 1], 2, [2, 2])):
        assert osr.clamp_starts(np.array(starts, np.uint32), n).tolist() == want
        assert osr.clamp_starts_loop(np.array(starts, np.uint32), n) == want
    assert osr.row_segments([2, 4, 4, 7], 9).tolist() == [-1, -1, 0, 0, 2, 2, 2, -1, -1]


@pytest.mark.parametrize("name", sorted(PARTITION))
def test_partition_scene(name):
    s = PARTITION[name]
    assert s["holds"](s), name
    rng = np.random.default_rng(len(name))
    pts = scenes.odd_points(rng, len(s["ids"]))
    nseg = len(s["starts"]) - 1
    a = osr.group(pts, s["ids"], s["starts"], s["nobj"], s["keep"])
    b = osr.group_by_slices(pts, s["ids"], s["starts"], s["nobj"], s["keep"])
    osr.assert_group_equal(a, b)
    if nseg * s["nobj"] <= BIG:
        osr.assert_group_equal(a, osr.group_loop(pts, s["ids"], s["starts"], s["nobj"], s["keep"]))
        osr.assert_group_equal(a, osr.group_by_slices(pts, s["ids"], s["starts"], s["nobj"], s["keep"],
                                                      slice_rule=opr.group_loop))
    assert len(a["obj_start"]) == nseg * s["nobj"] + 1 and a["obj_start"][0] == 0
    assert a["obj_start"][-1] == a["total"] == a["seg_out_start"][-1] and len(a["seg_out_start"]) == nseg + 1
    st = osr.clamp_starts(s["starts"], len(s["ids"]))
    assert ((a["index"] >= st[0]) & (a["index"] < st[-1])).all()
    # stable: inside a group the input rows ascend
    grp = np.repeat(np.arange(nseg * s["nobj"]), np.diff(a["obj_start"].astype(np.int64)))
    same = grp[1:] == grp[:-1]
    assert (np.diff(a["index"].astype(np.int64))[same] > 0).all()
    if name in ("every row dropped", "all empty"):
        assert a["total"] == 0
    if name == "keep drops a segment":
        assert a["seg_out_start"][1] == a["seg_out_start"][2] and a["total"] > 0


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_scene(name):
    s = TABLE[name]
    assert s["holds"](s), name
    a = osr.table(s["cells"], s["starts"], s["C"])
    osr.assert_table_equal(a, osr.table_loop(s["cells"], s["starts"], s["C"]))
    osr.assert_table_equal(a, osr.table_by_slices(s["cells"], s["starts"], s["C"]))
    osr.assert_table_equal(a, osr.table_by_slices(s["cells"], s["starts"], s["C"], slice_rule=vtr.table_loop))
    nseg = len(s["starts"]) - 1
    assert a["vox_seg_start"][0] == 0 and a["vox_seg_start"][-1] == a["num_voxels"]
    assert len(a["vox_seg_start"]) == nseg + 1 and (a["vox_cells"] < s["C"]).all()
    st = osr.clamp_starts(s["starts"], len(s["cells"]))
    rows = st[-1] - st[0] - int((s["cells"][st[0]:st[-1]] >= s["C"]).sum())
    assert int(a["vox_counts"].sum()) == rows and (a["vox_counts"] > 0).all()
    if name.startswith("same cell across border"):
        b = int(s["starts"][1])       # the two rows at the border are two voxels of one cell
        pv = a["point_voxel"]
        assert pv[b - 1] != pv[b] and a["vox_cells"][pv[b - 1]] == a["vox_cells"][pv[b]] == 1234
        assert pv[b - 1] < a["vox_seg_start"][1] <= pv[b]
    if name == "a run over three segments":
        assert len({int(a["point_voxel"][i]) for i in (100, 175, 250)}) == 3
    if name.startswith("every cell"):
        assert a["num_voxels"] == 3 * s["C"]


def test_refusal_lists_are_beyond_the_bounds():
    for nseg, nobj in scenes.PARTITION_REFUSALS:
        assert not (1 <= nseg <= 64) or nobj == 0 or nseg * nobj > scenes.MAX_GROUPS
    for nseg, C in scenes.TABLE_REFUSALS:
        assert not (1 <= nseg <= 64) or C == 0 or nseg * C > scenes.MAX_CELLS


def test_fixture_frames_as_one_three_segment_batch():
    grid = fixture_grid()
    frames = [fixture_frame(f) for f in range(3)]
    coords = np.concatenate([fr["coords"] for fr in frames])
    pts = np.concatenate([fr["points"] for fr in frames])
    point_start = np.concatenate([[0], np.cumsum([len(fr["coords"]) for fr in frames])]).astype(np.uint32)
    t = osr.table(coords, point_start, grid.ncells)
    osr.assert_table_equal(t, osr.table_loop(coords, point_start, grid.ncells))
    assert t["vox_seg_start"].tolist() == [0, 560, 560 + 563, 560 + 563 + 593]
    average = manifest()["voxel_average"][0] != 0
    for f, fr in enumerate(frames):
        a, b = int(t["vox_seg_start"][f]), int(t["vox_seg_start"][f + 1])
        distinct, rows = voxel_ref.voxelize_ref(fr["coords"], fr["points"], average=average, grid=grid)
        assert np.array_equal(t["vox_cells"][a:b], distinct), f
        assert b - a == len(fr["voxelized"])
        pv = t["point_voxel"][point_start[f]:point_start[f + 1]]
        chain = vtr.chain_means(fr["points"], pv - np.uint32(a), b - a)
        assert np.array_equal(np.ascontiguousarray(chain[:, :3]).view(np.uint32), fr["voxelized"].view(np.uint32)), f
    assert len(pts) == t["n"]
