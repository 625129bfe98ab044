"""The voxel-table rule restated on the CPU (tests/voxel_table_ref.py): its two forms agree with each
other and with np.unique, and on the facade fixture (tests/golden/facade) the table of a frame's
voxel coords is the key list of the frame's voxelized rows.  No GPU."""
import os

import numpy as np
import pytest

import voxel_ref
import voxel_table_ref as vtr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "facade")
NONE = vtr.NONE


def manifest():
    m = {}
    for line in open(os.path.join(FIX, "manifest.txt")):
        k, *v = line.split()
        m[k] = [float(x) for x in v]
    return m


def fixture_frame(f):
    rd = lambda name, dt: np.fromfile(os.path.join(FIX, f"{name}{f}.bin"), dt)
    return {"points": rd("points", "<f4").reshape(-1, 4), "coords": rd("coords", "<u4"),
            "voxelized": rd("voxelized", "<f4").reshape(-1, 3), "grid": rd("grid", "u1")}


def fixture_grid():
    v = manifest()["voxel"]
    return voxel_ref.Grid(v[0:3], v[3:6], v[6:9])


def cell_lists():
    """name -> (cells, C): the patterns of the GPU test at small sizes."""
    rng = np.random.default_rng(14)
    out = {}
    for n in (0, 1, 63, 64, 65, 257, 1025):
        for C in (1, 31, 32, 33, 513, 70000):
            rnd = rng.integers(0, C, n).astype(np.uint32)
            asc = (np.arange(n, dtype=np.uint64) % C).astype(np.uint32)
            runs = np.repeat(rng.integers(0, C, n // 3 + 1), rng.integers(1, 9, n // 3 + 1))[:n]
            third = rnd.copy()
            third[::3] = rng.choice(np.array([C, C + 1, 1 << 31, NONE], np.uint64), len(third[::3]))
            out[f"random n{n} C{C}"] = (rnd, C)
            out[f"ascending n{n} C{C}"] = (asc, C)
            out[f"descending n{n} C{C}"] = (asc[::-1].copy(), C)
            out[f"one cell n{n} C{C}"] = (np.full(n, C - 1, np.uint32), C)
            out[f"runs n{n} C{C}"] = (runs.astype(np.uint32), C)
            out[f"third outside n{n} C{C}"] = (third.astype(np.uint32), C)
            out[f"all outside n{n} C{C}"] = (np.full(n, C, np.uint32), C)
    return out


def test_loop_and_vector_forms_agree_with_each_other_and_with_unique():
    seen_outside = seen_voxels = False
    for name, (cells, C) in cell_lists().items():
        a, b = vtr.table(cells, C), vtr.table_loop(cells, C)
        try:
            vtr.assert_equal(a, b)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None
        inside = cells < C
        u, inv, cnt = np.unique(cells[inside], return_inverse=True, return_counts=True)
        assert np.array_equal(a["vox_cells"], u) and np.array_equal(a["vox_counts"], cnt), name
        assert np.array_equal(a["point_voxel"][inside], inv.reshape(-1)), name
        assert (a["point_voxel"][~inside] == NONE).all(), name
        assert a["vox_counts"].sum() == len(cells) - (~inside).sum(), name
        assert (a["vox_counts"] > 0).all() and (np.diff(a["vox_cells"].astype(np.int64)) > 0).all()
        assert np.array_equal(a["vox_cells"][a["point_voxel"][inside]], cells[inside]), name
        seen_outside |= bool((~inside).any())
        seen_voxels |= a["num_voxels"] > 1
    assert seen_outside and seen_voxels


@pytest.mark.parametrize("f", range(3))
def test_table_of_the_fixture_coords_is_the_voxelized_key_list(f):
    fr, grid = fixture_frame(f), fixture_grid()
    coords, pts = fr["coords"], fr["points"]
    assert len(coords) == len(pts) > 0
    t = vtr.table(coords, grid.ncells)
    vtr.assert_equal(t, vtr.table_loop(coords, grid.ncells))
    distinct, rows = voxel_ref.voxelize_ref(coords, pts, average=manifest()["voxel_average"][0] != 0,
                                            grid=grid)
    assert np.array_equal(t["vox_cells"], distinct)
    assert t["num_voxels"] == len(fr["voxelized"]) == (560, 563, 593)[f]
    xyz = lambda r: np.ascontiguousarray(r[:, :3]).view(np.uint32)  # (the fixture keeps x, y, z)
    assert np.array_equal(xyz(rows), fr["voxelized"].view(np.uint32))
    # the sequential chain over the rows with point_voxel == g, in input order, is voxelized row g
    chain = vtr.chain_means(pts, t["point_voxel"], t["num_voxels"], form="loop")
    assert np.array_equal(chain.view(np.uint32),
                          vtr.chain_means(pts, t["point_voxel"], t["num_voxels"]).view(np.uint32))
    assert np.array_equal(xyz(chain), fr["voxelized"].view(np.uint32))
    assert np.array_equal(chain.view(np.uint32), rows.view(np.uint32))
    outside = int((coords >= grid.ncells).sum())
    assert int(t["vox_counts"].sum()) == len(coords) - outside
    # every voxel's cell is occupied in the frame's grid
    assert fr["grid"].size == grid.ncells and (fr["grid"][t["vox_cells"]] != 0).all()


def test_frame_0_grid_cells_are_exactly_the_table():
    fr, grid = fixture_frame(0), fixture_grid()
    t = vtr.table(fr["coords"], grid.ncells)
    assert np.array_equal(np.flatnonzero(fr["grid"]).astype(np.uint32), t["vox_cells"])
