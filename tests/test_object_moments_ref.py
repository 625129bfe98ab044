"""The per-object moments rule on the CPU: the two restatements agree, a hand-computed
cloud, the voxel coordinate inside q on the facade fixture, the overflow bound, and the library's
host helper gdf_obj_shapes_from_moments against the Python restatement, bit for bit."""
import os

import numpy as np
import pytest

import object_moments_ref as omr
from conftest import ROOT

FIX = os.path.join(ROOT, "tests", "golden", "facade")


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def random_starts(rng, total, nobj):
    cuts = np.sort(rng.integers(0, total + 1, nobj - 1))
    return np.concatenate([[0], cuts, [total]]).astype(np.uint32)


@pytest.mark.parametrize("n,nobj", [(0, 1), (1, 1), (97, 1), (300, 7), (300, 400)])
def test_the_two_forms_agree(n, nobj):
    rng = np.random.default_rng(n + nobj)
    p, rows = omr.special_cloud(rng, n)
    if n >= 97 * 3:
        omr.check_special_classes(p, rows)
    start = random_starts(rng, n, nobj)
    a = omr.moments(p, start, **omr.GRID)
    b = omr.moments_loop(p, start, **omr.GRID)
    omr.assert_equal(a, b)
    assert np.array_equal(a["count"].astype(np.int64) + a["outside"], np.diff(start.astype(np.int64)))
    none = a["count"] == 0
    assert (a["qmin"][none] == 0xFFFFFFFF).all() and not a["qmax"][none].any()
    assert not a["sum"][none].any() and not a["sum2"][none].any()
    if nobj == 400:
        assert none.any() and (~none).any()


def test_hand_computed_cloud():
    """Five rows on grid (4, 2, 2), lower 0, cell 1: q = 256 p, the upper face clamps to 256 gs - 1,
    one row below the grid.  A second object holds a single NaN row."""
    p = np.array([[0, 0, 0, 9], [1.5, 0.25, 1, 9], [4, 2, 2, 9], [-0.5, 0, 0, 9],
                  [1023 / 256, 1.0, 0.5, 9], [np.nan, 0, 0, 9]], np.float32)
    start = [0, 5, 6]
    want = omr.empty(2)
    # q: (0, 0, 0), (384, 64, 256), (1023, 511, 511), -, (1023, 256, 128)
    want[0] = (4, 1, [0, 0, 0], [1023, 511, 511], [2430, 831, 895],
               [2240514, 809217, 752001, 330753, 310273, 343041])
    want[1] = (0, 1, [0xFFFFFFFF] * 3, [0] * 3, [0] * 3, [0] * 6)
    grid = dict(lower=[0, 0, 0], cell=[1, 1, 1], gs=[4, 2, 2])
    omr.assert_equal(omr.moments(p, start, **grid), want)
    omr.assert_equal(omr.moments_loop(p, start, **grid), want)


def fixture_grid():
    man = {}
    for line in open(os.path.join(FIX, "manifest.txt")):
        key, *vals = line.split()
        man[key] = [float(v) for v in vals]
    v = np.array(man["voxel"], np.float32)
    lo, hi, cs = v[0:3], v[3:6], v[6:9]
    gs = np.ceil((hi - lo) / cs).astype(np.uint32)  # computeVoxelCoords, in f32
    return int(man["frames"][0]), lo, cs, gs


def test_q_holds_the_voxel_coordinate_on_the_facade_fixture():
    frames, lo, cs, gs = fixture_grid()
    assert gs.tolist() == [60, 40, 24]
    rows = 0
    for f in range(frames):
        p = np.fromfile(os.path.join(FIX, f"points{f}.bin"), "<f4").reshape(-1, 4)
        coords = np.fromfile(os.path.join(FIX, f"coords{f}.bin"), "<u4")
        assert len(p) == len(coords) > 1000
        measured, q = omr.measure(p, lo, cs, gs)
        v = (q >> 8).astype(np.uint64)
        lin = v[:, 0] + v[:, 1] * gs[0] + v[:, 2] * (int(gs[0]) * int(gs[1]))
        assert measured.mean() > 0.9
        assert np.array_equal(lin[measured], coords[measured].astype(np.uint64))
        rows += len(p)
    assert rows == 19496


def test_overflow_bound():
    """(256 max gs - 1)^2 n_cap < 2^64: the largest admissible pairs and the first inadmissible."""
    m = 256 * 65536 - 1
    assert omr.sums_fit((65536, 1, 1), 65536) and m * m * 65536 < 2**64
    assert not omr.sums_fit((1, 65536, 1), 65537) and m * m * 65537 >= 2**64
    # every row count of a u32 at gs 256; none of the largest at 257
    assert omr.sums_fit((256, 256, 256), 2**32 - 1) and not omr.sums_fit((2, 257, 1), 2**32 - 1)
    # the launch-default grid (60 x 40 x 24 cells) allows 2^30 rows
    assert omr.sums_fit((60, 40, 24), 2**30)
    # at the bound the largest possible sum fits, one row more of the largest q^2 does not
    assert m * m * 65536 + m * m >= 2**64


# ---- gdf_obj_shapes_from_moments -------------------------------------------------------------------
def c_shapes(m, lower, cell):
    from ros_gpu_depthmap_fusion_amd import build_library
    from ros_gpu_depthmap_fusion_amd.gdf import obj_shapes_from_moments
    build_library()
    return obj_shapes_from_moments(m, lower, cell)


def numerator(r, k):
    a, b = omr.PAIRS[k]
    return int(r["count"]) * int(r["sum2"][k]) - int(r["sum"][a]) * int(r["sum"][b])


def shape_cases():
    rng = np.random.default_rng(11)
    m = omr.empty(6)
    top = 2**24 - 1
    # 0: 60 000 rows, half at q = 0 and half at the top of a 65536-cell axis: numerators near 2^78
    h = 30_000
    assert omr.sums_fit((65536,) * 3, 2 * h)
    m[0] = (2 * h, 5, [0] * 3, [top] * 3, [h * top] * 3, np.array([h * top * top] * 6, np.uint64))
    # 1: x ascending while y descends: a negative xy numerator
    q = np.stack([np.arange(50) * 100, 9000 - np.arange(50) * 37, rng.integers(0, 500, 50)], 1)
    m[1] = (50, 0, q.min(0), q.max(0), q.sum(0), [(q[:, a] * q[:, b]).sum() for a, b in omr.PAIRS])
    # 2: no measured row; 3: one row
    m[2]["outside"] = 4
    m[3] = (1, 0, [7, 8, 9], [7, 8, 9], [7, 8, 9], [49, 56, 63, 64, 72, 81])
    # 4, 5: random clouds through the rule
    p, _ = omr.special_cloud(rng, 600)
    m[4:6] = omr.moments(p, [0, 250, 600], **omr.GRID)
    return m


def test_shapes_from_moments_equal_the_restatement_bit_for_bit():
    m = shape_cases()
    assert numerator(m[0], 0) > 2**64 and numerator(m[1], 1) < 0
    assert m[2]["count"] == 0 and m[3]["count"] == 1
    for lower, cell in ((omr.GRID["lower"], omr.GRID["cell"]), ([-3.0, -3.0, -1.0], [0.15, 0.15, 0.15]),
                        ([1e-3, 7.7, -123.456], [0.1, 3.3, 1e-2])):
        got, want = c_shapes(m, lower, cell), omr.shapes(m, lower, cell)
        for k in omr.SHAPE_DTYPE.names:
            assert np.array_equal(u64(got[k]), u64(want[k])), (k, got[k], want[k])
        for k in omr.SHAPE_DTYPE.names:
            assert np.isnan(got[k][2]).all() and np.isfinite(got[k][[0, 1, 3, 4, 5]]).all()
        assert not got["cov"][3].any() and not np.signbit(got["cov"][3]).any()  # one row: +0.0
        assert got["cov"][1][1] < 0 < got["cov"][1][0]
        # the centroid lies inside the bounds
        ok = [0, 1, 3, 4, 5]
        assert (got["min_world"][ok] <= got["centroid"][ok]).all()
        assert (got["centroid"][ok] <= got["max_world"][ok]).all()
    # zero records: nothing is read or written
    assert len(c_shapes(omr.empty(0), [0, 0, 0], [1, 1, 1])) == 0


def test_a_line_along_x_has_no_spread_in_y_and_z():
    n = 200
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = np.linspace(0.01, 1.7, n)
    p[:, 1], p[:, 2] = 0.3, 2.4
    m = omr.moments(p, [0, n], **omr.GRID)
    assert m["count"][0] == n
    for s in (c_shapes(m, omr.GRID["lower"], omr.GRID["cell"]),
              omr.shapes(m, omr.GRID["lower"], omr.GRID["cell"])):
        xx, xy, xz, yy, yz, zz = s["cov"][0]
        assert yy == 0.0 and zz == 0.0 and yz == 0.0 and xy == 0.0 and xz == 0.0 and xx > 0.1
