"""Event-timed cost of the radius outlier filter (include/gdf_filter.h) next to the frame's own
chain, one JSON line per configuration:

    python tools/radius_bench.py [--calls 200] [--warmup 20] [--sizes vga,4k] [--out FILE]

Clouds: the compacted points of one dense VGA frame (~115 K points) and one dense 4K frame
(~3.05 M), and the VGA frame's voxelized cloud; r 0.05, box = the voxel box, min_neighbors 0 / 4 /
16, plus one run whose min_neighbors no point reaches ("noexit": every candidate is evaluated, so
its count kernel's pair evaluations are exactly the candidate pairs the grid offers).

Per line: us per filter call (median of the event-timed calls after warm-up: all its launches),
frame_us (the median of the same frame's gdf_process_frame chain, timed the same way in this
process), the candidate pairs the cell grid offers (host count from the plan), the count kernel's
time taken as the call's time minus the min_neighbors = 0 call's (which skips the candidate loops
and is otherwise the same passes), pairs per second where that is exact (noexit), and the bytes the
other passes move (model of DESIGN.md §11)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ros_gpu_depthmap_fusion_amd import build_library, hiprt, synth  # noqa: E402
from ros_gpu_depthmap_fusion_amd.gdf import (ComponentParams, GPUDepthmapFusion,  # noqa: E402
                                             radius_filter_plan)

SIZES = {"vga": (640, 480), "4k": (3840, 2160)}
NOEXIT = 2 ** 31 - 1


class Timer:
    def __init__(self, stream):
        self.h, self.s = hiprt.hip(), C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        hiprt.check(self.h.hipEventCreate(C.byref(self.a)))
        hiprt.check(self.h.hipEventCreate(C.byref(self.b)))

    def us(self, fn):
        hiprt.check(self.h.hipEventRecord(self.a, self.s))
        fn()
        hiprt.check(self.h.hipEventRecord(self.b, self.s))
        hiprt.check(self.h.hipEventSynchronize(self.b))
        ms = C.c_float()
        hiprt.check(self.h.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return ms.value * 1e3


def median_us(timer, fn, calls, warmup):
    first = timer.us(fn)
    if first > 50e3:          # a call over 50 ms: no further warm-up, fewer calls (reported)
        warmup, calls = 0, max(5, int(5e6 / first))
    for _ in range(warmup):
        timer.us(fn)
    return float(np.median([timer.us(fn) for _ in range(calls)])), calls


def offered_pairs(pts, lower, upper, radius):
    """(inside points, candidate pairs the 3x3x3 cells offer them, cells) from the plan."""
    cells, edge = radius_filter_plan(lower, upper, radius)
    lo, hi = np.asarray(lower, np.float32), np.asarray(upper, np.float32)
    p = pts[:, :3]
    p = p[((p >= lo) & (p <= hi)).all(axis=1)]
    idx = []
    for a in range(3):
        ext = float(hi[a]) - float(lo[a])
        inv = np.float32(cells[a] / ext) if cells[a] > 1 else np.float32(0)
        idx.append(np.minimum(np.floor((p[:, a] - lo[a]) * inv), cells[a] - 1).astype(np.int64))
    occ = np.zeros((cells[2] + 2, cells[1] + 2, cells[0] + 2), np.int64)
    np.add.at(occ, (idx[2] + 1, idx[1] + 1, idx[0] + 1), 1)
    near = np.zeros_like(occ)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near += np.roll(occ, (dz, dy, dx), (0, 1, 2))
    return len(p), int((occ * near).sum() - len(p)), cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="vga,4k")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    build_library()
    p = ComponentParams()
    lower, upper, radius = tuple(p.voxel_min), tuple(p.voxel_max), 0.05
    lines = []
    for size in a.sizes.split(","):
        W, H = SIZES[size]
        gpu = GPUDepthmapFusion(0)
        cam = synth.make_camera(0, W, H)
        depth = hiprt.DeviceArray.from_numpy(synth.dense_frame(cam, 0, 0))
        pc = p.to_c(synchronous=False)

        def frame():
            gpu.clear()
            gpu.addDepthmapDevice(depth.ptr, W, H, *cam.intrinsics(), cam.T_world, cam.T_crop)
            gpu.processFramePrepared(pc)

        timer = Timer(gpu.stream())
        frame_us, _ = median_us(timer, frame, a.calls, a.warmup)
        gpu.synchronize()
        sources = [("points", gpu.downloadPoints())]
        if size == "vga":
            sources.append(("voxelized", gpu.downloadVoxelizedPoints()))
        for source, pts in sources:
            inside, pairs, cells = offered_pairs(pts, lower, upper, radius)
            ncells = cells[0] * cells[1] * cells[2]
            base_us = None
            for m in (0, 4, 16, NOEXIT):
                us, calls = median_us(
                    timer, lambda: gpu.radiusFilter(lower, upper, radius, m, source=source),
                    a.calls, a.warmup)
                kept = gpu.filtered_count()
                if m == 0:
                    base_us = us
                n = len(pts)
                # cell pass 24 n; scan 16 / cell; scatter 8 n + 36 / inside point; the count
                # kernel's own point, cell and flag 21 / inside point; flags twice 2 n; output
                other = n * 34 + ncells * 16 + inside * 57 + kept * 32
                line = dict(cloud=f"{size}_{source}", n=n, inside=inside, kept=kept,
                            min_neighbors="noexit" if m == NOEXIT else m, cells=list(cells),
                            us=round(us, 2), calls=calls, frame_us=round(frame_us, 2),
                            count_us=round(us - base_us, 2), candidate_pairs=pairs,
                            other_bytes=other)
                if m == NOEXIT and us > base_us:
                    line["pairs_per_s"] = float(f"{pairs / ((us - base_us) * 1e-6):.4g}")
                print(json.dumps(line), flush=True)
                lines.append(line)
        gpu.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
