"""CPU checks of the radius outlier filter: hand-computed answers of the restatement
(tests/radius_ref.py), its two forms against each other on every scene the GPU tests use, and the
cell plan / argument checks of the library (gdf_radius_filter_plan, no GPU)."""
import ctypes as C

import numpy as np
import pytest

import radius_ref as R
import radius_scenes as S

BOX = ((-1, -1, -1), (1, 1, 1))


def P(rows):
    a = np.zeros((len(rows), 4), np.float32)
    a[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    a[:, 3] = np.arange(len(rows))
    return a


def both(pts, lower, upper, radius, m):
    kb, cb = R.brute(pts, lower, upper, radius, m)
    kw, cw = R.window(pts, lower, upper, radius, m)
    assert np.array_equal(kb, kw) and np.array_equal(cb, cw)
    return kb, cb


# ---- hand-computed answers ----------------------------------------------------------------------
def test_pair_at_the_threshold_and_one_step_above():
    r = np.float32(0.25)                       # r2 = 0.0625 exactly; dx = 0.25 exactly: d2 == r2
    k, c = both(P([[0, 0, 0], [0.25, 0, 0]]), *BOX, r, 1)
    assert k.tolist() == [True, True] and c.tolist() == [1, 1]
    x = np.nextafter(np.float32(0.25), np.float32(1))   # dx * dx rounds above 0.0625
    assert np.float32(x * x) > np.float32(0.0625)
    k, c = both(P([[0, 0, 0], [x, 0, 0]]), *BOX, r, 1)
    assert k.tolist() == [False, False] and c.tolist() == [0, 0]


def test_three_collinear_points():
    pts = P([[0, 0, 0], [0.08, 0, 0], [0.16, 0, 0]])    # r 0.1: only the middle one sees two
    k, c = both(pts, *BOX, 0.1, 2)
    assert c.tolist() == [1, 2, 1] and k.tolist() == [False, True, False]


def test_coincident_pair_and_no_self_neighbour():
    k, c = both(P([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]), *BOX, 0.01, 1)
    assert c.tolist() == [1, 1] and k.all()
    k, c = both(P([[0.5, 0.5, 0.5]]), *BOX, 0.01, 1)
    assert c.tolist() == [0] and not k.any()


def test_min_neighbors_0_1_n():
    pts = P([[0, 0, 0], [0.05, 0, 0], [0.9, 0.9, 0.9], [5, 0, 0]])
    assert both(pts, *BOX, 0.1, 0)[0].tolist() == [True, True, True, False]   # every inside point
    assert both(pts, *BOX, 0.1, 1)[0].tolist() == [True, True, False, False]
    assert not both(pts, *BOX, 0.1, len(pts))[0].any()


def test_nan_inf_rows_and_box_faces():
    rows = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf],
            [-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1], [1, 1, 1],
            [np.nextafter(np.float32(1), np.float32(2)), 0, 0]]
    k, c = both(P(rows), *BOX, 0.1, 0)
    assert k.tolist() == [False] * 3 + [True] * 7 + [False]
    assert R.inside_mask(P(rows), *BOX).tolist() == k.tolist()


def test_an_outside_point_is_nobodys_neighbour():
    pts = P([[0.98, 0, 0], [1.02, 0, 0]])               # 0.04 apart, the second outside the box
    k, c = both(pts, *BOX, 0.1, 1)
    assert c.tolist() == [0, 0] and k.tolist() == [False, False]
    k, c = both(pts, (-2, -2, -2), (2, 2, 2), 0.1, 1)   # (both inside: neighbours)
    assert c.tolist() == [1, 1]


def test_w_is_carried_not_read():
    pts = P([[0, 0, 0], [0.05, 0, 0], [0.5, 0, 0]])
    pts[:, 3] = [np.nan, 7.5, -1]
    out = R.apply(pts, R.brute(pts, *BOX, 0.1, 1)[0])
    assert np.array_equal(out.view(np.uint32), pts[:2].view(np.uint32))


# ---- the two forms on the GPU tests' scenes -----------------------------------------------------
@pytest.mark.parametrize("name", S.SMALL_NAMES)
def test_forms_agree_on_gpu_scene(name):
    scene = S.get(name)
    for m in scene["mins"]:
        both(scene["pts"], scene["lower"], scene["upper"], scene["radius"], m)


def test_window_form_on_the_multi_block_scene():
    """Above 8192 points there is no brute force: the window over x against the window over y
    (x and y swapped in points and box; dx*dx + dy*dy is commutative in binary32)."""
    s = S.get("multiblock_65537")
    kx, cx = R.window(s["pts"], s["lower"], s["upper"], s["radius"], 4)
    sw = [1, 0, 2]
    ky, cy = R.window(s["pts"][:, sw + [3]], np.take(s["lower"], sw), np.take(s["upper"], sw),
                      s["radius"], 4)
    assert np.array_equal(kx, ky) and np.array_equal(cx, cy)
    assert 0 < kx.sum() < len(kx) and 3.5 < cx.mean() < 5


def test_engine_frame_sources_from_the_oracle():
    """The engine-stage scenes: the oracle's 160x120 dense frame holds 5091 points and 1028 voxels,
    and both forms agree on them (the GPU tests filter the engine's own, bit-identical, copies)."""
    from oracle import OracleFusion
    from ros_gpu_depthmap_fusion_amd import synth
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    cam = synth.make_camera(0, 160, 120)
    o = OracleFusion()
    o.clear()
    o.addDepthmap(synth.dense_frame(cam, 0, 0), *cam.intrinsics(), cam.T_world, cam.T_crop)
    o.processFrame(ComponentParams())
    pts, vox = o.downloadPoints(), o.downloadVoxelizedPoints()
    assert (len(pts), len(vox)) == (5091, 1028)
    lo, hi = (0, -8, -0.5), (10, 8, 2)
    assert abs(both(pts, lo, hi, 0.05, 4)[0].mean() - 0.69) < 0.01
    assert abs(both(pts, lo, hi, 0.05, 16)[0].mean() - 0.065) < 0.005
    assert abs(both(vox, lo, hi, 0.15, 6)[0].mean() - 0.50) < 0.01
    k = both(pts, lo, (5, 8, 2), 0.05, 4)[0]
    assert 0 < k.sum() < R.inside_mask(pts, lo, (5, 8, 2)).sum() < len(pts)


# ---- the library's plan and argument checks (no GPU) ---------------------------------------------
PLAN_TABLE = [
    ((-2, -2, -2), (2, 2, 2), 0.05, (79, 79, 79)),          # the launch defaults
    ((-1, -1, -1), (1, 1, 1), 0.1, (19, 19, 19)),
    ((0, -8, -0.5), (10, 8, 2), 0.05, None),
    ((0, 0, 0), (8, 8, 1), 0.1, None),
    ((-10, -20, -1), (30, 20, 1.5), 0.05, None),            # the voxel box: 799 x 799 x 49 > 2^22
] + [v for v in S.PLAN_EXTREMES.values()]


@pytest.mark.parametrize("lower,upper,radius,want", PLAN_TABLE)
def test_plan_invariants(lower, upper, radius, want):
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_plan
    cells, edge = radius_filter_plan(lower, upper, radius)
    if want is not None:
        assert cells == tuple(want)
    pc, pe = S.plan_py(lower, upper, radius)
    assert cells == pc
    assert all(1 <= c <= 1024 for c in cells) and cells[0] * cells[1] * cells[2] <= 2 ** 22
    r = float(np.float32(radius))
    for a in range(3):
        ext = float(np.float32(upper[a])) - float(np.float32(lower[a]))
        assert edge[a] == np.float32(ext / cells[a])
        if cells[a] > 1:   # (edge is reported in float32: half an ulp below the double is allowed)
            assert float(edge[a]) >= r * (1 + 2.0 ** -10) * (1 - 2.0 ** -24)


def test_plan_caps_bind_for_the_2km_box():
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_plan
    lo, hi, r, want = S.PLAN_EXTREMES["both_caps"]
    cells, edge = radius_filter_plan(lo, hi, r)
    assert cells == want and cells[0] * cells[1] * cells[2] == 2 ** 22
    assert 2000 / (r * (1 + 2.0 ** -10)) > 1024             # (the per-axis cap bound first)


@pytest.mark.parametrize("lower,upper,radius", [
    ((-1, -1, -1), (1, 1, 1), 0.0), ((-1, -1, -1), (1, 1, 1), -0.1),
    ((-1, -1, -1), (1, 1, 1), np.nan), ((-1, -1, -1), (1, 1, 1), np.inf),
    ((-1, -1, -1), (1, 1, 1), 1e-30),       # r2 underflows to 0
    ((-1, -1, -1), (1, 1, 1), 1e30),        # r2 overflows
    ((1, -1, -1), (-1, 1, 1), 0.1),         # lower > upper
    ((np.nan, -1, -1), (1, 1, 1), 0.1), ((-1, -1, -1), (1, np.inf, 1), 0.1),
])
def test_plan_refuses_bad_arguments(lower, upper, radius):
    from ros_gpu_depthmap_fusion_amd.gdf import GDFError, radius_filter_plan
    with pytest.raises(GDFError) as e:
        radius_filter_plan(lower, upper, radius)
    assert e.value.status == -1


def test_null_engine_calls_fail_cleanly():
    from ros_gpu_depthmap_fusion_amd.gdf import load_library, radius_filter_params
    lib = load_library()
    p = radius_filter_params((-1, -1, -1), (1, 1, 1), 0.1, 1)
    n = C.c_uint32()
    assert lib.gdf_radius_filter_points(None, None, 0, C.byref(p), None, None, None) == -1
    assert b"null engine" in lib.gdf_last_error()
    assert lib.gdf_radius_filter(None, 0, C.byref(p)) == -1
    assert lib.gdf_set_radius_filter(None, 1, C.byref(p)) == -1
    assert lib.gdf_get_filtered_count(None, C.byref(n)) == -1
    assert lib.gdf_download_filtered_points(None, None, 0, C.byref(n)) == -1
    assert lib.gdf_get_device_filtered(None, None, None) == -1
    assert lib.gdf_radius_filter_plan(None, None, None) == -1
