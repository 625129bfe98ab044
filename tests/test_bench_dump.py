"""bench.py --dump-outputs: the writer's budget, formats and sampling (host logic, a stand-in
engine; the GPU run of the option is the benchmark itself)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


class StandInEngine:
    """The download calls dump_outputs makes, over arrays that depend on the sizes only."""

    def __init__(self, points, cells, frames):
        self.n, self.nc, self.B = points, cells, frames

    def grid_size(self):
        return (self.nc, 1, 1), self.nc

    def downloadPoints(self):
        return (np.arange(4 * self.n, dtype=np.float32) * 0.5).reshape(self.n, 4)

    def downloadVoxelCoords(self):
        return np.arange(self.n, dtype=np.uint32) % max(self.nc, 1)

    def downloadVoxelizedPoints(self):
        return np.arange(4 * (self.n // 8), dtype=np.float32).reshape(self.n // 8, 4)

    def downloadVoxelOccupancyGrid(self):
        return (np.arange(self.nc) % 11).astype(np.uint8)

    def downloadBatchVoxelOccupancyGrid(self, j):
        return ((np.arange(self.nc) + j) % 11).astype(np.uint8)

    def batch_ranges(self):
        ps = np.linspace(0, self.n, self.B + 1).astype(np.uint32)
        return ps, ps // 8


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_when_it_fits(tmp_path):
    eng = StandInEngine(1000, 300, 4)
    info = bench.dump_outputs(eng, 4, str(tmp_path))
    got = load(tmp_path)
    assert set(got) == {"points", "voxel_coords", "voxelized_points", "occupancy_grid",
                        "occupancy_grid_batch", "point_ranges", "voxel_ranges"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["points"], eng.downloadPoints())
    assert np.array_equal(got["voxel_coords"], eng.downloadVoxelCoords())
    assert np.array_equal(got["occupancy_grid"], eng.downloadVoxelOccupancyGrid())
    assert got["occupancy_grid_batch"].shape == (300, 3)
    assert np.array_equal(got["occupancy_grid_batch"][:, 2], eng.downloadBatchVoxelOccupancyGrid(2))
    assert np.array_equal(got["point_ranges"], eng.batch_ranges()[0])
    assert all(v["rows_saved"] == v["shape"][0] for v in info.values())


def test_dump_single_frame_has_no_batch_arrays(tmp_path):
    bench.dump_outputs(StandInEngine(64, 32, 1), 1, str(tmp_path))
    assert set(load(tmp_path)) == {"points", "voxel_coords", "voxelized_points", "occupancy_grid"}


def test_dump_budget_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 600 * 1000)
    eng = StandInEngine(100000, 5000, 4)  # 1.6 MB of points alone
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(eng, 4, str(a))
    bench.dump_outputs(eng, 4, str(b))
    files = [os.path.join(a, f) for f in os.listdir(a)]
    assert sum(os.path.getsize(f) for f in files) <= 600 * 1000 * 64 // 60
    ga, gb = load(a), load(b)
    for k in ga:  # the same rows both times
        assert np.array_equal(ga[k], gb[k]), k
    # arrays under their share stay whole, the points are a sample of whole rows in order
    assert info["occupancy_grid"]["rows_saved"] == 5000  # 20 kB as float32
    assert info["point_ranges"]["rows_saved"] == 5
    # the earlier frames' grids: 12 B a row, a fifteenth of the budget
    assert info["occupancy_grid_batch"]["rows_saved"] == 40000 // 12
    n = info["points"]["rows_saved"]
    assert 0 < n < 100000 and ga["points"].shape == (n, 4)
    rows = (ga["points"][:, 0] / 2).astype(np.int64)  # row r holds 2r, 2r + .5, 2r + 1, 2r + 1.5
    assert np.all(np.diff(rows) > 0)
    assert np.array_equal(ga["points"], eng.downloadPoints()[rows])


def test_dump_wide_coords_keep_their_bits(tmp_path):
    eng = StandInEngine(16, (1 << 24) + 9, 1)
    eng.downloadVoxelCoords = lambda: np.full(16, (1 << 24) + 7, np.uint32)
    eng.downloadVoxelOccupancyGrid = lambda: np.zeros(8, np.uint8)
    bench.dump_outputs(eng, 1, str(tmp_path))
    got = load(tmp_path)["voxel_coords"]
    assert got.dtype == np.float64 and np.all(got == (1 << 24) + 7)
