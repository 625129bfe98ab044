"""Event-timed cost of the per-object moments (include/gdf_segment.h) next to the
calls it follows, one JSON line per configuration:

    python tools/object_moments_bench.py [--calls 200] [--warmup 20] [--sizes vga,4k] [--out FILE]

Per shape one dense frame (one camera, the launch-default grid) is processed, its grid labelled and
gdf_seg_object_points run (min_voxels 0); then gdf_seg_object_moments is timed on that grouped
result: us (median of the event-timed calls after warm-up: both launches), next to object_points_us
and frame_us (that frame's gdf_seg_object_points call and its gdf_process_frame chain, timed the
same way in this process).  Those frames hold a handful of objects, so per shape two more lines
time the moments after gdf_seg_group_points on the same points with uniformly random ids below 256
and 65 536, where many segments fall in every tile.  bytes is the model of DESIGN.md §13: 16 B per
kept row, 104 B per record, and 104 B per partial slot written and read again."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ros_gpu_depthmap_fusion_amd import build_library, hiprt, synth  # noqa: E402
from ros_gpu_depthmap_fusion_amd.gdf import (SEG_CONNECTIONS, ComponentParams,  # noqa: E402
                                             GPUDepthmapFusion, Segmenter)

SIZES = {"vga": (640, 480), "4k": (3840, 2160)}
CHUNK = 512   # kOmChunk
RECORD = 104  # sizeof(gdf_obj_moments)


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


def partial_slots(obj_start):
    """Slots k_om_tiles writes and k_om_finish reads: one per chunk of every object that crosses
    a chunk edge."""
    s, e = obj_start[:-1].astype(np.int64), obj_start[1:].astype(np.int64)
    some = e > s
    c0, c1 = s[some] // CHUNK, (e[some] - 1) // CHUNK
    return int((c1 - c0 + 1)[c1 > c0].sum())


def line_of(cloud, seg, timer, grid, a, **more):
    us = median_us(timer, lambda: seg.object_moments(*grid, download=False), a.calls, a.warmup)
    r = seg.object_points_results()
    m = seg.object_moments_results()
    slots = partial_slots(r["obj_start"])
    nbytes = 16 * r["total"] + RECORD * r["nobj"] + 2 * RECORD * slots
    return dict(cloud=cloud, total=r["total"], nobj=r["nobj"], occupied=int((m["count"] > 0).sum()),
                measured=int(m["count"].sum()), outside=int(m["outside"].sum()),
                partial_slots=slots, us=round(us, 2), calls=a.calls, bytes=nbytes,
                gbps=round(nbytes / (us * 1e-6) / 1e9, 1), **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="vga,4k")
    ap.add_argument("--out", default="")
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
        (gx, gy, gz), _ = gpu.grid_size()
        grid = (np.array(p.voxel_min, np.float32), np.array(p.voxel_size, np.float32),
                np.array([gx, gy, gz], np.uint32))
        seg.label_engine_grid(gpu, SEG_CONNECTIONS)
        op_us = median_us(timer, lambda: seg.object_points(gpu, 0), a.calls, a.warmup)
        line = line_of(f"{size}_points", seg, timer, grid, a, n=n, frame_us=round(frame_us, 2),
                       object_points_us=round(op_us, 2))
        print(json.dumps(line), flush=True)
        lines.append(line)
        # many segments in every tile: the same points under uniformly random ids
        seg.set_stream(gpu.stream())
        d_pts = hiprt.DeviceArray.from_numpy(gpu.downloadPoints())
        rng = np.random.default_rng(n)
        for nobj in (256, 65536):
            d_ids = hiprt.DeviceArray.from_numpy(rng.integers(0, nobj, n).astype(np.uint32))
            gp_us = median_us(timer, lambda: seg.group_points(d_pts.ptr, d_ids.ptr, n, nobj),
                              a.calls, a.warmup)
            line = line_of(f"{size}_points_random_ids", seg, timer, grid, a, n=n,
                           frame_us=round(frame_us, 2), group_points_us=round(gp_us, 2))
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
