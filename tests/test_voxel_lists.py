"""CPU checks of the voxelize scenes (tests/voxel_lists.py) and their reference
(tests/voxel_ref.py): the two reference forms agree bit for bit and with the C oracle, the
restated kernel constants match the source, every scene holds the case it is named for, the
scenes together reach every route of k_group and k_group_runs on both sides of every threshold,
and the point values make every group's sum depend on the order of its points."""
import os
import re

import numpy as np
import pytest

import voxel_lists as vl
from voxel_ref import Grid, cut_runs, expand_runs, marks_ref, runs_of, voxelize_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ros_gpu_depthmap_fusion_amd", "csrc")
GRID22 = Grid(*vl.GRIDS[22])
SCENES = vl.scenes()
_built = {}


def built(scene, ncells=GRID22.ncells):
    k = (scene.name, ncells)
    if k not in _built:
        _built[k] = scene.build(ncells)
    return _built[k]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_grids_have_their_key_width():
    for b, g in vl.GRIDS.items():
        assert Grid(*g).key_bits == b
    assert Grid(*vl.GRIDS[26]).ncells <= 64 << 20


def test_scene_names_are_unique():
    names = [s.name for s in SCENES]
    assert len(set(names)) == len(names)


def test_reference_forms_agree():
    """The plain loop over sequential_sum and the cumsum form give the same rows, bit for bit,
    on every scene (22-bit grid) and on the digit and length scenes of the narrowest grid."""
    small = Grid(*vl.GRIDS[8]).ncells
    for sc in SCENES:
        for nc in (GRID22.ncells, small) if sc.keyfn is not None else (GRID22.ncells,):
            b = built(sc, nc)
            ka, ra = voxelize_ref(b["keys"], b["pts"], form="loop")
            kb, rb = voxelize_ref(b["keys"], b["pts"], form="vector")
            assert np.array_equal(ka, kb), sc.name
            assert np.array_equal(bits(ra), bits(rb)), sc.name
            assert np.array_equal(ka, [k for k, _ in b["groups"]]), sc.name


@pytest.mark.parametrize("average", [True, False])
def test_reference_equals_oracle(average):
    """One small synthetic frame through the C oracle: voxelize_ref over its compacted points and
    voxel coordinates equals its voxelized cloud bit for bit (means and corners)."""
    from oracle import OracleFusion
    from ros_gpu_depthmap_fusion_amd import synth
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    p = ComponentParams()
    p.voxel_average = average
    cam = synth.make_camera(0, 192, 144)
    orc = OracleFusion(threads=1)
    orc.clear()
    orc.addDepthmap(synth.dense_frame(cam, 0, 0), *cam.intrinsics(), cam.T_world, cam.T_crop)
    orc.processFrame(p)
    grid = Grid(p.voxel_min, p.voxel_max, p.voxel_size)
    assert grid.gs == orc.grid_size()
    pts, keys = orc.downloadPoints(), orc.downloadVoxelCoords()
    want = orc.downloadVoxelizedPoints()
    assert len(pts) > 2000 and int(np.bincount(keys).max()) > 8
    for form in ("vector", "loop"):
        _, rows = voxelize_ref(keys, pts, average=average, grid=grid, form=form)
        assert rows.shape == want.shape
        assert np.array_equal(bits(rows), bits(want)), form


def test_constants_match_source():
    """The constants restated in voxel_lists.py, read out of the kernels' source text."""
    src = ""
    for f in ("gdf_kernels.hip", "gdf_device.hpp"):
        with open(os.path.join(CSRC, f)) as fh:
            src += fh.read()

    def const(name):
        m = re.findall(r"constexpr\s+(?:int|uint32_t)\s+" + name + r"\s*=\s*(\d+)\s*;", src)
        assert len(m) == 1, name
        return int(m[0])

    def tuning(name):
        m = re.findall(r"^\s*uint32_t\s+" + name + r"\s*=\s*(\d+)\s*;", src, re.M)
        assert len(m) == 1, name
        return int(m[0])

    for name in ("kGroupThreads", "kStagePts", "kGatherChunk", "kExtraRuns", "kHugeGroup",
                 "kHugeRuns", "kRunPasses", "kXRunTile", "kSortThreads", "kSortGroup"):
        assert const(name) == getattr(vl, name), name
    for name in ("small_group", "run_stage", "run_inblock", "group_scan_tiles", "run_wave"):
        assert tuning(name) == getattr(vl.DEFAULT, name), name
    # the group look-back's granule: lookback2_wave groups tiles by tile >> 6, the in-kernel
    # group scan by kScanGroup
    assert const("kScanGroup") == vl.kLookGranule
    assert re.search(r"const uint32_t G = tile >> 6, first = G << 6", src)
    assert 1 << 6 == vl.kLookGranule


def test_run_helpers():
    keys = np.array([5, 5, 5, 2, 2, 9, 5, 5], np.uint32)
    rk, rs = runs_of(keys)
    assert rk.tolist() == [5, 2, 9, 5] and rs.tolist() == [0, 3, 5, 6, 8]
    ck, cs = cut_runs(rk, rs, [0, 1, 3, 7, 8, 99])
    assert ck.tolist() == [5, 5, 2, 9, 5, 5] and cs.tolist() == [0, 1, 3, 5, 6, 7, 8]
    assert np.array_equal(expand_runs(ck, cs), keys)
    assert runs_of(np.zeros(0, np.uint32))[1].tolist() == [0]
    assert marks_ref([0, 31, 32, 95], 4).tolist() == [0x80000001, 1, 0x80000000, 0]


@pytest.mark.parametrize("scene", SCENES, ids=lambda s: s.name)
def test_scene_holds_its_case(scene):
    """The scene's description, list and run decomposition are consistent, and the census (default
    knobs) shows the events the scene is named for."""
    b = built(scene)
    rk, rs = runs_of(b["keys"])
    assert np.array_equal(rk, b["run_keys"]) and np.array_equal(rs, b["run_starts"])
    assert sum(sum(r) for _, r in b["groups"]) == len(b["keys"])
    if scene.lens is not None:  # the description survives the arrangement, run for run
        assert [r for _, r in b["groups"]] == [list(r) for r in scene.lens]
    c = vl.census(b)
    assert scene.needs <= c["events"], sorted(scene.needs - c["events"])
    for m in ("points", "runs"):
        assert c[m]["tile_starts"].sum() == len(b["groups"])
        assert c[m]["points"].sum() == len(b["keys"])
    assert np.array_equal(c["points"]["items"], [sum(r) for _, r in b["groups"]])
    assert np.array_equal(c["runs"]["items"], [len(r) for _, r in b["groups"]])
    # k_group: a tile's 256 items end within kStagePts positions of its first group start, so a
    # group of <= small_group points never lies past the staged positions
    assert "kg.short_past_stage" not in c["events"]
    if scene.single_runs:  # item = point = run: one tile geometry for both kernels
        assert np.array_equal(c["points"]["start"], c["runs"]["start"])


# every route and both sides of every threshold, per kernel variant
_KG = {"kg.route.thread", "kg.route.stretch", "kg.route.gather", "kg.route.queue", "kg.lookback",
       "kg.scan", "kg.len=small", "kg.len=small+1", "kg.end=staged", "kg.end=staged+1",
       "kg.gather.len%chunk=0", "kg.gather.len%chunk=1", "tile.nostart", "tile.nostart>=3",
       "tile.end=tile", "tile.end=tile-1", "tile.end=tile+1", "last.end=tile", "last.end=tile+1",
       "tile.first_at=200"}
_KGR_ALL = {"kgr.route.thread", "kgr.route.queue.long", "kgr.route.queue.cross", "kgr.lookback",
            "kgr.scan", "kgr.pts=small", "kgr.pts=small+1", "kgr.pts=inblock", "kgr.pts=inblock+1",
            "kgr.pts=stage", "kgr.pts=stage+1", "kgr.extra=64", "kgr.extra=65", "tile.nostart"}
_KGR_WAVE = {
    0: {"kgr.route.queue.stage", "kgr.queue.short"},
    1: {"kgr.route.wave", "kgr.route.queue.stage", "kgr.queue.short"},
    2: {"kgr.route.lanes", "kgr.route.queue.windows", "kgr.queue.short", "kgr.short_next_window",
        "kgr.windows=1", "kgr.windows=4", "kgr.route.queue.long.huge",
        "kgr.route.queue.cross.huge", "kgr.pts=huge-1", "kgr.pts=huge", "kgr.runs=huge-1",
        "kgr.runs=huge", "kgr.huge.est_low", "kgr.huge.est_only"},
}


def test_scenes_reach_every_route_and_threshold():
    """Over all scenes: every route of k_group, and of k_group_runs<2048 | 512, 0 | 1 | 2>, on
    both sides of each threshold."""
    ev = set()
    for sc in SCENES:
        ev |= vl.census_points(np.sort(built(sc)["keys"], kind="stable"))["events"]
    assert _KG <= ev, sorted(_KG - ev)
    for stage in (2048, 512):
        for wave in (0, 1, 2):
            kn = vl.Knobs(run_stage=stage, run_wave=wave)
            ev = set()
            for sc in SCENES:
                ev |= vl.census(built(sc), kn)["runs"]["events"]
            want = _KGR_ALL | _KGR_WAVE[wave]
            assert want <= ev, (stage, wave, sorted(want - ev))


def test_off_edge_list_is_exact():
    """Under every knob set of the GPU test, each scene of the knob families still shows the
    events it is named for, but for the events OFF_EDGE lists for that knob set; and each listed
    event is lost by a scene that needs it."""
    fam = [s for s in SCENES if s.family in vl.KNOB_FAMILIES]
    done = {}
    for name, (_, kn) in vl.KNOB_SETS.items():
        if kn not in done:
            done[kn] = {s.name: vl.census(built(s), kn)["events"] for s in fam}
        lost = set()
        for s in fam:
            assert vl.on_edge_needs(s, name) <= done[kn][s.name], (name, s.name)
            lost |= s.needs - done[kn][s.name]
        assert lost == set(vl.OFF_EDGE.get(name, ())), (name, sorted(lost))


def test_point_values_are_order_sensitive():
    """In every scene with groups of >= 8 points, reversing the points inside each group changes
    the reference's bits in at least 90 % of those groups."""
    seen = 0
    for sc in SCENES:
        b = built(sc)
        ch, of = vl.reversal_changes(b["keys"], b["pts"])
        assert ch >= 0.9 * of, (sc.name, ch, of)
        seen += of > 0
    assert seen >= 90
