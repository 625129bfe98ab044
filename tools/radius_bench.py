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
other passes move (model of DESIGN.md §11).

    python tools/radius_bench.py --batch 8 [--tables a,b] [--sources points,voxelized] [--mins 0,4,16]

measures the filter per frame of a batch instead (profiles/radius_filter_batch/):
table a, a batch of 8 dense VGA frames - one gdf_radius_filter_batch call against eight
gdf_radius_filter_points calls on the same segments, next to the batch's own chain; table b, the
clouds above as one segment over the sparse cell table against the dense grid's call."""
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


def emit(lines, line):
    print(json.dumps(line), flush=True)
    lines.append(line)


def batch_lines(a, p, lower, upper, radius, lines):
    """(a) A batch of `--batch` dense VGA frames (one camera, as bench.py's step): the segmented
    call (gdf_radius_filter_batch) against one gdf_radius_filter_points call per frame on the same
    segments, next to the batch's own chain.  us: all launches of the call(s), median."""
    from ros_gpu_depthmap_fusion_amd.gdf import radius_filter_params
    W, H = SIZES["vga"]
    B = a.batch
    gpu = GPUDepthmapFusion(0)
    cam = synth.make_camera(0, W, H)
    depths = [hiprt.DeviceArray.from_numpy(synth.dense_frame(cam, 0, f)) for f in range(B)]
    pc = p.to_c(synchronous=False)

    def chain():
        gpu.clear()
        for j, d in enumerate(depths):
            if j:
                gpu.nextFrameInBatch()
            gpu.addDepthmapDevice(d.ptr, W, H, *cam.intrinsics(), cam.T_world, cam.T_crop)
        gpu.processFramePrepared(pc)

    timer = Timer(gpu.stream())
    chain_us, _ = median_us(timer, chain, a.calls, a.warmup)
    gpu.synchronize()
    ps, vs = gpu.batch_ranges()
    for source, pts, starts in (("voxelized", gpu.downloadVoxelizedPoints(), vs),
                                ("points", gpu.downloadPoints(), ps)):
        if source not in a.sources.split(","):
            continue
        n = len(pts)
        d_in = hiprt.DeviceArray.from_numpy(np.ascontiguousarray(pts, np.float32))
        d_out, d_cnt = hiprt.DeviceArray(16 * max(n, 1)), hiprt.DeviceArray(4 * B)
        for m in a.min_list:
            prm = radius_filter_params(lower, upper, radius, m)

            def per_frame():
                for s in range(B):
                    b, e = int(starts[s]), int(starts[s + 1])
                    gpu.radiusFilterPoints(d_in.ptr + 16 * b, e - b, prm, d_out.ptr + 16 * b,
                                           d_cnt.ptr + 4 * s)

            seg_us, calls = median_us(
                timer, lambda: gpu.radiusFilterBatch(lower, upper, radius, m, source=source),
                a.calls, a.warmup)
            kept = gpu.filtered_count()
            pf_us, _ = median_us(timer, per_frame, a.calls, a.warmup)
            gpu.synchronize()
            kept_pf = int(d_cnt.to_numpy(np.uint32, B).sum())
            emit(lines, dict(table="a", cloud=f"vga_b{B}_{source}", frames=B, n=n, kept=kept,
                             kept_per_frame_calls=kept_pf, min_neighbors=m,
                             segments_us=round(seg_us, 2), per_frame_calls_us=round(pf_us, 2),
                             chain_us=round(chain_us, 2), calls=calls,
                             ratio=round(pf_us / seg_us, 3)))
    gpu.close()


def single_lines(a, p, lower, upper, radius, lines):
    """(b) The rows of the single-cloud table: nseg = 1 over the sparse table (gdf_radius_filter_batch
    on a single frame) against the dense grid's call (gdf_radius_filter) on the same input."""
    for size in a.sizes.split(","):
        W, H = SIZES[size]
        gpu = GPUDepthmapFusion(0)
        cam = synth.make_camera(0, W, H)
        depth = hiprt.DeviceArray.from_numpy(synth.dense_frame(cam, 0, 0))
        gpu.clear()
        gpu.addDepthmapDevice(depth.ptr, W, H, *cam.intrinsics(), cam.T_world, cam.T_crop)
        gpu.processFramePrepared(p.to_c(synchronous=False))
        gpu.synchronize()
        timer = Timer(gpu.stream())
        counts = {"points": len(gpu.downloadPoints()), "voxelized": len(gpu.downloadVoxelizedPoints())}
        for source in (("points", "voxelized") if size == "vga" else ("points",)):
            if source not in a.sources.split(","):
                continue
            for m in a.min_list:
                dense_us, calls = median_us(
                    timer, lambda: gpu.radiusFilter(lower, upper, radius, m, source=source),
                    a.calls, a.warmup)
                kept_dense = gpu.filtered_count()
                sparse_us, _ = median_us(
                    timer, lambda: gpu.radiusFilterBatch(lower, upper, radius, m, source=source),
                    a.calls, a.warmup)
                kept = gpu.filtered_count()
                emit(lines, dict(table="b", cloud=f"{size}_{source}", n=counts[source], kept=kept,
                                 kept_dense=kept_dense, min_neighbors=m, sparse_us=round(sparse_us, 2),
                                 dense_us=round(dense_us, 2), calls=calls,
                                 ratio=round(dense_us / sparse_us, 3)))
        gpu.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="vga,4k")
    ap.add_argument("--batch", type=int, default=0,
                    help="N > 0: the segmented filter's tables instead (a batch of N VGA frames "
                         "against per-frame calls; one segment against the dense call)")
    ap.add_argument("--tables", default="a,b", help="with --batch: which of its two tables")
    ap.add_argument("--sources", default="points,voxelized", help="with --batch: which clouds")
    ap.add_argument("--mins", default="0,4,16", help="with --batch: min_neighbors values")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.min_list = [int(m) for m in a.mins.split(",")]
    build_library()
    p = ComponentParams()
    lower, upper, radius = tuple(p.voxel_min), tuple(p.voxel_max), 0.05
    lines = []
    if a.batch > 0 and "a" in a.tables.split(","):
        batch_lines(a, p, lower, upper, radius, lines)
    if a.batch > 0 and "b" in a.tables.split(","):
        single_lines(a, p, lower, upper, radius, lines)
    for size in ([] if a.batch > 0 else a.sizes.split(",")):
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
