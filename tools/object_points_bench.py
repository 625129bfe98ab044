"""Event-timed cost of the object-points stage (include/gdf_segment.h) next to the
frame's own chain, one JSON line per configuration:

    python tools/object_points_bench.py [--calls 200] [--warmup 20] [--sizes vga,4k] [--out FILE]

Per shape one dense frame (one camera, the launch-default grid) is processed, its grid labelled
(gdf_seg_label_engine_grid with GDF_SEG_CONNECTIONS), and gdf_seg_object_points timed for
min_voxels 0 and 8.  Per line: n, nobj, passes, total; us per call (median of the event-timed calls
after warm-up: all its launches); frame_us (the same frame's gdf_process_frame chain timed the same
way in this process); and per pass the median of the call's own events (gdf_seg_set_profiling) with
the GB/s its bytes of the model of DESIGN.md §12 make of it.  Those frames hold a handful of
objects (one 8-bit pass), so per shape three more lines time gdf_seg_group_points alone on the same
points with uniformly random ids below 256, 65 536 and 2^20: one, two and three passes."""
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
TILE = 2048  # kOpTile


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


def byte_model(n, total, nobj, passes):
    """Bytes per pass: every array counted once per kernel that streams it."""
    nt = max((n + TILE - 1) // TILE, 1)
    hist = 1024 * nt                               # 256 digits x 4 B per tile
    b = {"ids": n * (4 + 2 + 4 + 4)}               # cell, label, merged id, id out
    for p in range(passes):
        src = n * 5 if p == 0 else total * 8       # ids + keep flag / pairs
        b[f"count{p}"] = src + hist + 2 * hist     # the tile counts, then their scan in place
        b[f"scatter{p}"] = src + hist + total * 8
    b["gather"] = total * (8 + 16 + 16 + 4)        # pair, point in, point out, index
    b["starts"] = (nobj + 1) * 4
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="vga,4k")
    ap.add_argument("--mins", default="0,8",
                    help="min_voxels values; 'mid' is halfway between the smallest and the largest "
                         "object's voxel count of the frame, so some objects' points are dropped")
    ap.add_argument("--no-synthetic", action="store_true",
                    help="skip the random-id lines (the partition alone at 1 / 2 / 3 passes)")
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
        seg.label_engine_grid(gpu, SEG_CONNECTIONS)
        mins = a.mins.split(",")
        if "mid" in mins:
            seg.object_points(gpu, 0)
            vox = seg.object_points_results()["voxels"]
            vox = vox[vox > 0]
            mid = int(vox.min()) + max((int(vox.max()) - int(vox.min())) // 2, 1)
        for mv in (mid if m == "mid" else int(m) for m in mins):
            seg.set_profiling(False)
            us = median_us(timer, lambda: seg.object_points(gpu, mv), a.calls, a.warmup)
            nobj, total = seg.object_points_counts()
            seg.set_profiling(True)
            rows = []
            for _ in range(a.calls):
                seg.object_points(gpu, mv)
                rows.append(seg.object_points_times())
            ms = np.median(np.array(rows), axis=0)
            passes = (len(ms) - 3) // 2
            names = ["ids"] + [f"{k}{q}" for q in range(passes) for k in ("count", "scatter")] + \
                ["gather", "starts"]
            model = byte_model(n, total, nobj, passes)
            per_pass = {k: dict(us=round(float(t) * 1e3, 2), bytes=model[k],
                                gbps=round(model[k] / (float(t) * 1e-3) / 1e9, 1) if t > 0 else None)
                        for k, t in zip(names, ms)}
            line = dict(cloud=f"{size}_points", n=n, nobj=nobj, passes=passes, total=total,
                        min_voxels=mv, us=round(us, 2), frame_us=round(frame_us, 2), calls=a.calls,
                        bytes=sum(model.values()),
                        gbps=round(sum(model.values()) / (us * 1e-6) / 1e9, 1), per_pass=per_pass)
            print(json.dumps(line), flush=True)
            lines.append(line)
        # the partition alone on the same points with uniformly random ids: what 2 and 3 passes cost
        # (the frames above have a handful of objects: one pass)
        seg.set_stream(gpu.stream())
        d_pts = hiprt.DeviceArray.from_numpy(gpu.downloadPoints())
        rng = np.random.default_rng(n)
        for nobj in (() if a.no_synthetic else (256, 65536, 1 << 20)):
            d_ids = hiprt.DeviceArray.from_numpy(rng.integers(0, nobj, n).astype(np.uint32))
            seg.set_profiling(False)
            us = median_us(timer, lambda: seg.group_points(d_pts.ptr, d_ids.ptr, n, nobj),
                           a.calls, a.warmup)
            _, total = seg.object_points_counts()
            seg.set_profiling(True)
            rows = []
            for _ in range(a.calls):
                seg.group_points(d_pts.ptr, d_ids.ptr, n, nobj)
                rows.append(seg.object_points_times())
            ms = np.median(np.array(rows), axis=0)
            passes = (len(ms) - 3) // 2
            names = ["ids"] + [f"{k}{q}" for q in range(passes) for k in ("count", "scatter")] + \
                ["gather", "starts"]
            model = byte_model(n, total, nobj, passes)
            model["ids"] = 0
            model["count0"] -= n                       # no keep flags
            model["scatter0"] -= n
            per_pass = {k: dict(us=round(float(t) * 1e3, 2), bytes=model[k],
                                gbps=round(model[k] / (float(t) * 1e-3) / 1e9, 1) if t > 0 else None)
                        for k, t in zip(names, ms) if k != "ids"}
            line = dict(cloud=f"{size}_points_random_ids", n=n, nobj=nobj, passes=passes,
                        total=total, us=round(us, 2), frame_us=round(frame_us, 2), calls=a.calls,
                        bytes=sum(model.values()),
                        gbps=round(sum(model.values()) / (us * 1e-6) / 1e9, 1), per_pass=per_pass)
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
