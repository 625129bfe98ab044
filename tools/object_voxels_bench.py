"""Event-timed cost of the voxel table and of the object-voxels stage (include/gdf_segment.h,
DESIGN.md §14) next to the frame's own chain and to the same frame's object-points call, one JSON
line per configuration:

    python tools/object_voxels_bench.py [--calls 200] [--warmup 20] [--sizes vga,4k] [--out FILE]

Per shape one dense frame (one camera, the launch-default grid) is processed, its grid labelled
(gdf_seg_label_engine_grid with GDF_SEG_CONNECTIONS), and per min_voxels value gdf_seg_object_voxels
is timed.  Per line: n, G, nobj, total; us per call (median of the event-timed calls after warm-up:
all its launches); frame_us and object_points_us (the same frame's gdf_process_frame chain and its
gdf_seg_object_points call, timed the same way in this process); and per pass the median of the
call's own events (gdf_seg_set_profiling) with the bytes of the model of DESIGN.md §14.
Two more lines per shape time gdf_seg_voxel_table alone on the frame's coords as they are (runs of
equal cells) and on a shuffled copy (no runs: every lane marks and adds for itself), which is what
the lane dedup of k_vt_mark and the per-run adds of k_vt_rank are worth on this data.
The raw lines go to profiles/object_voxels/ by default."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ros_gpu_depthmap_fusion_amd import build_library, hiprt, synth  # noqa: E402
from ros_gpu_depthmap_fusion_amd.gdf import (SEG_CONNECTIONS, ComponentParams,  # noqa: E402
                                             GPUDepthmapFusion, Segmenter)

SIZES = {"vga": (640, 480), "4k": (3840, 2160)}
TILE = 2048       # kOpTile
ROW_WORDS = 64    # kVtRowWords
TABLE = ("clear", "mark", "rows_scan", "expand", "rank")
STAGE = TABLE + ("ids_sizes", "group", "weights")


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
    for _ in range(warmup):
        timer.us(fn)
    return float(np.median([timer.us(fn) for _ in range(calls)]))


def byte_model(n, G, cells, total, nobj):
    """Bytes per pass: every array counted once per kernel that streams it; the
    gathers of k_vt_rank (word_rank and the bitmap word of a row's cell) counted per row."""
    words = (cells + 31) // 32
    rows = (words + ROW_WORDS - 1) // ROW_WORDS
    nt = max((G + TILE - 1) // TILE, 1)
    hist = 1024 * nt
    return {"clear": words * 4,
            "mark": n * 4 + G * 4,                       # cells; about one OR per voxel and wave
            "rows_scan": words * 4 + rows * 4 + rows * 8,
            "expand": words * 4 + rows * 4 + words * 4 + G * 8,
            "rank": n * (4 + 4 + 4 + 4) + G * 4,         # cell, word_rank, bitmap word, point_voxel; adds
            "ids_sizes": G * (4 + 2 + 4 + 4) + nobj * 5,
            "group": G * 5 + 3 * hist + G * 5 + hist + total * 8 + total * (8 + 16 + 16 + 4) + (nobj + 1) * 4,
            "weights": total * 12}


def per_pass(names, ms, model):
    return {k: dict(us=round(float(t) * 1e3, 2), bytes=model[k],
                    gbps=round(model[k] / (float(t) * 1e-3) / 1e9, 1) if t > 0 else None)
            for k, t in zip(names, ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="vga,4k")
    ap.add_argument("--mins", default="0,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_voxels", "lines.txt"))
    a = ap.parse_args()
    build_library()
    p = ComponentParams()
    lines = []
    for size in a.sizes.split(","):
        W, H = SIZES[size]
        gpu, seg = GPUDepthmapFusion(0), Segmenter(0)
        cam = synth.make_camera(0, W, H)
        depth = hiprt.DeviceArray.from_numpy(synth.dense_frame(cam, 0, 0))
        pc = p.to_c(synchronous=False)

        def frame():
            gpu.clear()
            gpu.addDepthmapDevice(depth.ptr, W, H, *cam.intrinsics(), cam.T_world, cam.T_crop)
            gpu.processFramePrepared(pc)

        timer = Timer(gpu.stream())
        frame_us = median_us(timer, frame, a.calls, a.warmup)
        gpu.synchronize()
        n = gpu.point_count()
        _, cells = gpu.grid_size()
        seg.label_engine_grid(gpu, SEG_CONNECTIONS)
        for mv in (int(m) for m in a.mins.split(",")):
            seg.set_profiling(False)
            op_us = median_us(timer, lambda: seg.object_points(gpu, mv), a.calls, a.warmup)
            us = median_us(timer, lambda: seg.object_voxels(gpu, mv), a.calls, a.warmup)
            nobj, total = seg.object_points_counts()
            G, _ = seg.voxel_table_counts()
            seg.set_profiling(True)
            rows = []
            for _ in range(a.calls):
                seg.object_voxels(gpu, mv)
                rows.append(seg.voxel_table_times())
            ms = np.median(np.array(rows), axis=0)
            model = byte_model(n, G, cells, total, nobj)
            line = dict(cloud=f"{size}_voxels", n=n, G=G, cells=cells, nobj=nobj, total=total,
                        min_voxels=mv, us=round(us, 2), frame_us=round(frame_us, 2),
                        object_points_us=round(op_us, 2), calls=a.calls, bytes=sum(model.values()),
                        gbps=round(sum(model.values()) / (us * 1e-6) / 1e9, 1),
                        per_pass=per_pass(STAGE, ms, model))
            print(json.dumps(line), flush=True)
            lines.append(line)
        # the table alone: the frame's coords as they are, and shuffled (no runs of equal cells)
        seg.set_stream(gpu.stream())
        coords = gpu.downloadVoxelCoords()
        rng = np.random.default_rng(n)
        for name, arr in (("runs", coords), ("shuffled", rng.permutation(coords))):
            d_cells = hiprt.DeviceArray.from_numpy(arr)
            heads = int((arr[1:] != arr[:-1]).sum()) + 1 if len(arr) else 0
            seg.set_profiling(False)
            us = median_us(timer, lambda: seg.voxel_table(d_cells.ptr, n, cells), a.calls, a.warmup)
            G, _ = seg.voxel_table_counts()
            seg.set_profiling(True)
            rows = []
            for _ in range(a.calls):
                seg.voxel_table(d_cells.ptr, n, cells)
                rows.append(seg.voxel_table_times())
            ms = np.median(np.array(rows), axis=0)
            model = {k: v for k, v in byte_model(n, G, cells, 0, 0).items() if k in TABLE}
            line = dict(cloud=f"{size}_table_{name}", n=n, G=G, cells=cells, runs=heads,
                        us=round(us, 2), frame_us=round(frame_us, 2), calls=a.calls,
                        bytes=sum(model.values()),
                        gbps=round(sum(model.values()) / (us * 1e-6) / 1e9, 1),
                        per_pass=per_pass(TABLE, ms, model))
            print(json.dumps(line), flush=True)
            lines.append(line)
        seg.close()
        gpu.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
