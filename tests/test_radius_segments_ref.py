"""CPU checks of the segmented radius filter: the library's sparse cell plan against its Python
restatement and against the dense plan, and - from the CPU reference - that every composition of
the GPU tests (tests/radius_segment_scenes.py) holds what it is there for."""
import numpy as np
import pytest

import radius_ref as R
import radius_scenes as S
import radius_segment_scenes as C
from radius_segments_ref import apply_segments, plan_sparse_py, reference_segments

VOXEL_BOX = ((-10, -20, -1), (30, 20, 1.5))
PLAN_CASES = [
    ((-2, -2, -2), (2, 2, 2), 0.05), ((-1, -1, -1), (1, 1, 1), 0.1), ((0, -8, -0.5), (10, 8, 2), 0.05),
    ((0, 0, 0), (8, 8, 1), 0.1), (*VOXEL_BOX, 0.05), (*C.LADDER_BOX, 0.05),
    ((-1, -1, -1), (1, 1, 1), 1e-16),          # r2 below 2^-100: one cell in all
    ((-1e31, -1, -1), (1e31, 1, 1), 0.1),      # an axis longer than 2^100: one cell on it
] + [v[:3] for v in S.PLAN_EXTREMES.values()]


def ref(c, m):
    return reference_segments(c["pts"], c["starts"], c["lower"], c["upper"], c["radius"], m)


# ---- the plan -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lower,upper,radius", PLAN_CASES)
def test_sparse_plan_equals_its_restatement_and_the_dense_plan_where_uncapped(lower, upper, radius):
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_plan, radius_filter_plan_sparse
    cells, edge = radius_filter_plan_sparse(lower, upper, radius)
    pc, pe = plan_sparse_py(lower, upper, radius)
    assert cells == pc and all(1 <= c <= 1024 for c in cells)
    assert [float(e) for e in edge] == [float(np.float32(e)) for e in pe]
    dcells, dedge = radius_filter_plan(lower, upper, radius)
    if cells[0] * cells[1] * cells[2] <= 2 ** 22:
        assert cells == dcells and np.array_equal(edge, dedge)
    else:
        assert dcells != cells and all(d <= c for d, c in zip(dcells, cells))
    r = float(np.float32(radius))
    for a in range(3):                          # the margin the 3x3x3 proof needs
        if cells[a] > 1:
            assert float(edge[a]) >= r * (1 + 2.0 ** -10) * (1 - 2.0 ** -24)


def test_sparse_plan_of_the_voxel_box_and_the_extremes():
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_plan_sparse
    assert radius_filter_plan_sparse(*VOXEL_BOX, 0.05)[0] == (799, 799, 49)
    assert radius_filter_plan_sparse(*S.PLAN_EXTREMES["both_caps"][:3])[0] == (1024, 1024, 1024)
    assert radius_filter_plan_sparse(*S.PLAN_EXTREMES["flat_axis"][:3])[0] == (19, 19, 1)
    assert radius_filter_plan_sparse(*S.PLAN_EXTREMES["radius_over_box"][:3])[0] == (1, 1, 1)
    assert radius_filter_plan_sparse((-1, -1, -1), (1, 1, 1), 1e-16)[0] == (1, 1, 1)
    assert radius_filter_plan_sparse((-1e31, -1, -1), (1e31, 1, 1), 0.1)[0] == (1, 19, 19)
    assert radius_filter_plan_sparse(*C.LADDER_BOX, 0.05)[0] == (303, 303, 59)


@pytest.mark.parametrize("lower,upper,radius", [
    ((-1, -1, -1), (1, 1, 1), 0.0), ((-1, -1, -1), (1, 1, 1), -0.1),
    ((-1, -1, -1), (1, 1, 1), np.nan), ((-1, -1, -1), (1, 1, 1), np.inf),
    ((-1, -1, -1), (1, 1, 1), 1e-30), ((-1, -1, -1), (1, 1, 1), 1e30),
    ((1, -1, -1), (-1, 1, 1), 0.1),
    ((np.nan, -1, -1), (1, 1, 1), 0.1), ((-1, -1, -1), (1, np.inf, 1), 0.1),
])
def test_sparse_plan_refuses_what_the_dense_plan_refuses(lower, upper, radius):
    from ros_gpu_depthmap_fusion_amd.gdf import GDFError, radius_filter_plan, radius_filter_plan_sparse
    for plan in (radius_filter_plan, radius_filter_plan_sparse):
        with pytest.raises(GDFError) as e:
            plan(lower, upper, radius)
        assert e.value.status == -1


def test_null_calls_fail_cleanly():
    import ctypes as Ct
    from ros_gpu_depthmap_fusion_amd.gdf import load_library, radius_filter_params
    lib = load_library()
    p = radius_filter_params((-1, -1, -1), (1, 1, 1), 0.1, 1)
    n = Ct.c_uint32()
    assert lib.gdf_radius_filter_plan_sparse(None, None, None) == -1
    assert lib.gdf_radius_filter_segments(None, None, 0, None, 1, Ct.byref(p), None, None, None, None) == -1
    assert b"null engine" in lib.gdf_last_error()
    assert lib.gdf_radius_filter_batch(None, 0, Ct.byref(p)) == -1
    assert lib.gdf_set_radius_filter_batch(None, 1, Ct.byref(p)) == -1
    assert lib.gdf_get_filtered_ranges(None, None, 0, Ct.byref(n)) == -1
    assert lib.gdf_get_device_filtered_ranges(None, None, Ct.byref(n)) == -1


# ---- the restatement ----------------------------------------------------------------------------
def test_reference_segments_by_hand():
    pts = np.zeros((6, 4), np.float32)
    pts[:, 0] = [0, 0.05, 0.05, 0.1, 5, 0.05]              # r 0.1; the last row is behind start[nseg]
    keep, out_start = reference_segments(pts, [0, 2, 2, 3, 5], (-1, -1, -1), (1, 1, 1), 0.1, 1)
    assert keep.tolist() == [True, True, False, False, False]   # a pair, a lone point, one + an outside one
    assert out_start.tolist() == [0, 2, 2, 2, 2]
    assert np.array_equal(apply_segments(pts, keep), pts[:2])


# ---- the compositions ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_no_composition_has_an_all_kept_or_none_kept_answer(name):
    c = C.get(name)
    keep, out_start = ref(c, c["mins"][0])
    assert c["starts"][0] == 0 and c["starts"][-1] <= len(c["pts"])
    assert 0 < keep.sum() < len(keep), (name, keep.sum(), len(keep))
    assert out_start[0] == 0 and out_start[-1] == keep.sum()


def test_twin_differs_from_the_flattened_array():
    c = C.get("twin")
    keep, _ = ref(c, 1)
    flat, _ = R.reference(c["pts"], c["lower"], c["upper"], c["radius"], 1)
    inside = R.inside_mask(c["pts"], c["lower"], c["upper"])
    assert np.array_equal(flat, inside)                    # (every inside point has its twin)
    assert not np.array_equal(keep, flat) and 0 < keep.sum() < inside.sum()
    assert np.array_equal(keep[:257], keep[257:])


def test_edges_composition():
    c = C.get("edges")
    assert np.diff(c["starts"].astype(np.int64)).tolist() == C.EDGE_LENGTHS
    n = int(c["starts"][-1])
    assert n < len(c["pts"]) and np.isnan(c["pts"][n:n + 24]).all()
    keep, out_start = ref(c, 1)
    # cut, the cloud keeps fewer than whole; the copies behind the end would add neighbours
    whole, _ = R.reference(c["pts"][:n], c["lower"], c["upper"], c["radius"], 1)
    assert 0 < keep.sum() < whole.sum()
    longer = np.concatenate([c["starts"][:-2], [len(c["pts"])] * 2])   # (the 1025 rows read too far)
    read_behind, _ = reference_segments(c["pts"], longer, c["lower"], c["upper"], c["radius"], 1)
    assert read_behind[:n].sum() > keep.sum()
    assert len(set(out_start.tolist())) >= 4


@pytest.mark.parametrize("nseg", [16, 64])
def test_many_segments_composition(nseg):
    c = C.get(f"many_{nseg}")
    L = c["lengths"]
    assert len(c["starts"]) == nseg + 1 and set(L) == {1, 2, 3}
    k1, _ = ref(c, 1)
    k2, _ = ref(c, 2)
    want1 = np.concatenate([[k > 1] * k for k in L])
    want2 = np.concatenate([[k == 3 and j == 1 for j in range(k)] for k in L])
    assert np.array_equal(k1, want1) and np.array_equal(k2, want2)
    assert R.reference(c["pts"], c["lower"], c["upper"], c["radius"], 2)[0].all()   # flattened: all


def test_ladder_composition():
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_plan, radius_filter_plan_sparse
    c = C.get("ladder")
    L = c["ladder"]
    assert radius_filter_plan_sparse(c["lower"], c["upper"], c["radius"])[0] == L["cells"] == (303, 303, 59)
    assert radius_filter_plan(c["lower"], c["upper"], c["radius"])[0] != L["cells"]   # (halved)
    keep, out_start = ref(c, 1)
    a, b = c["middle"]
    assert len(c["starts"]) == 4 and not keep[:a].any() and not keep[b:].any()   # alone: isolated
    mid, cls = keep[a:b], L["cls"]
    for idx in (L["base_idx"], L["partner_idx"]):             # kept / kept / dropped
        assert mid[idx][cls == 0].all() and mid[idx][cls == 1].all() and not mid[idx][cls == 2].any()
    assert min((cls == k).sum() for k in range(3)) > 300
    assert set(np.unique(L["base_side"])) == {-2, -1, 0, 1, 2} and set(np.unique(L["kind"])) == {0, 1, 2, 3}
    assert out_start.tolist() == [0, 0, mid.sum(), mid.sum()]


def test_lattice_composition():
    c = C.get("lattice")
    cells, edge = plan_sparse_py(c["lower"], c["upper"], c["radius"])
    assert cells == (48, 24, 24)
    assert R.inside_mask(c["pts"], c["lower"], c["upper"]).all()
    cell = np.floor(c["pts"][:, :3].astype(np.float64) / np.asarray(edge)).astype(np.int64)
    ids = cell[:, 0] + 48 * (cell[:, 1] + 24 * cell[:, 2])
    assert len(np.unique(ids)) == len(c["pts"]) == 8191        # one point per cell
    keep, _ = ref(c, 1)
    assert abs(keep.mean() - 0.5) < 0.01                       # the rows of even j


def test_crowded_composition():
    c = C.get("crowded2")
    k, _ = ref(c, 2999)
    assert k[3:][c["cluster"]].all() and k.sum() == 3000 and not k[:3].any()
    assert ref(c, 2)[0][:3].tolist() == [False, True, False]
    assert not ref(c, 3000)[0].any()


def test_engine_batch_sources_from_the_oracle():
    """The engine tests' scene: the same 160x120 dense frame twice.  Filtered per frame and as one
    merged cloud the fates differ, at the parameters the GPU test uses."""
    from oracle import OracleFusion
    from ros_gpu_depthmap_fusion_amd import synth
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    cam = synth.make_camera(0, 160, 120)
    o = OracleFusion()
    o.clear()
    o.addDepthmap(synth.dense_frame(cam, 0, 0), *cam.intrinsics(), cam.T_world, cam.T_crop)
    o.processFrame(ComponentParams())
    lo, hi = (0, -8, -0.5), (10, 8, 2)
    for src, radius, m in ((o.downloadPoints(), 0.05, 4), (o.downloadVoxelizedPoints(), 0.15, 6)):
        n = len(src)
        two = np.concatenate([src, src])
        keep, out_start = reference_segments(two, [0, n, 2 * n], lo, hi, radius, m)
        merged, _ = R.reference(two, lo, hi, radius, m)
        assert np.array_equal(keep[:n], keep[n:]) and 0 < keep.sum() < 2 * n
        assert out_start.tolist() == [0, keep[:n].sum(), keep.sum()]
        assert (merged & ~keep).sum() > 0.05 * n               # kept only with the other frame's help
