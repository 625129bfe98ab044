"""Event-timed cost of the object layer on a batch (include/gdf_segment.h): one call
per batch against one call per frame, one JSON line per configuration:

    python tools/object_batch_bench.py [--batch 8] [--calls 200] [--warmup 20] [--size vga] [--out FILE]

A batch of N dense frames of one camera on the launch-default grid is processed as one
gdf_process_frame chain and its grid labelled (gdf_seg_label_engine_grid with GDF_SEG_CONNECTIONS).
Timed in this one process, medians of event-timed calls after warm-up:
  frame_us             the batch's gdf_process_frame chain
  object_points_us     gdf_seg_object_points_batch, with its passes (gdf_seg_set_profiling)
  object_voxels_us     gdf_seg_object_voxels_batch, with its passes
  single_*_us          the sum over the same N frames, each processed alone and labelled, of
                       gdf_seg_object_points / gdf_seg_object_voxels: what a caller without the batch
                       calls has to run, one frame after the other
A last line times gdf_seg_voxel_table_segments alone on the batch's coords and gdf_seg_voxel_table on
the same rows' composite cells built ahead of time (what a form that makes the composite inside the
mark and rank passes could save at most).
The raw lines go to profiles/object_batch/ by default."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from object_voxels_bench import SIZES, STAGE, Timer, median_us  # noqa: E402
from ros_gpu_depthmap_fusion_amd import build_library, hiprt, synth  # noqa: E402
from ros_gpu_depthmap_fusion_amd.gdf import (SEG_CONNECTIONS, ComponentParams,  # noqa: E402
                                             GPUDepthmapFusion, Segmenter)


def passes_us(seg, call, times, calls):
    seg.set_profiling(True)
    rows = []
    for _ in range(calls):
        call()
        rows.append(times())
    seg.set_profiling(False)
    return [round(float(t) * 1e3, 2) for t in np.median(np.array(rows), axis=0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--size", default="vga")
    ap.add_argument("--mins", default="0,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_batch", "lines.txt"))
    a = ap.parse_args()
    build_library()
    W, H = SIZES[a.size]
    N = a.batch
    p = ComponentParams()
    gpu, seg = GPUDepthmapFusion(0), Segmenter(0)
    cam = synth.make_camera(0, W, H)
    depth = [hiprt.DeviceArray.from_numpy(synth.dense_frame(cam, f, 0)) for f in range(N)]
    pc = p.to_c(synchronous=False)

    def chain(frames):
        gpu.clear()
        for j, f in enumerate(frames):
            if j:
                gpu.nextFrameInBatch()
            gpu.addDepthmapDevice(depth[f].ptr, W, H, *cam.intrinsics(), cam.T_world, cam.T_crop)
        gpu.processFramePrepared(pc)

    timer = Timer(gpu.stream())
    lines = []
    for mv in (int(m) for m in a.mins.split(",")):
        # one frame after the other: each frame alone, labelled, then the two single-frame calls
        single = {"frame": [], "points": [], "voxels": []}
        for f in range(N):
            single["frame"].append(median_us(timer, lambda: chain([f]), a.calls, a.warmup))
            gpu.synchronize()
            seg.label_engine_grid(gpu, SEG_CONNECTIONS)
            single["points"].append(median_us(timer, lambda: seg.object_points(gpu, mv), a.calls, a.warmup))
            single["voxels"].append(median_us(timer, lambda: seg.object_voxels(gpu, mv), a.calls, a.warmup))
        # the batch
        frame_us = median_us(timer, lambda: chain(range(N)), a.calls, a.warmup)
        gpu.synchronize()
        n = gpu.point_count()
        _, cells = gpu.grid_size()
        seg.label_engine_grid(gpu, SEG_CONNECTIONS)
        op_us = median_us(timer, lambda: seg.object_points_batch(gpu, mv), a.calls, a.warmup)
        nobj, op_total = seg.object_points_counts()
        op_pass = passes_us(seg, lambda: seg.object_points_batch(gpu, mv), seg.object_points_times, a.calls)
        ov_us = median_us(timer, lambda: seg.object_voxels_batch(gpu, mv), a.calls, a.warmup)
        _, ov_total = seg.object_points_counts()
        G, _ = seg.voxel_table_counts()
        ov_pass = passes_us(seg, lambda: seg.object_voxels_batch(gpu, mv), seg.voxel_table_times, a.calls)
        line = dict(cloud=f"{a.size}_batch{N}", frames=N, n=n, G=G, cells=cells, nobj=nobj, groups=N * nobj,
                    min_voxels=mv, calls=a.calls, frame_us=round(frame_us, 2),
                    object_points_us=round(op_us, 2), object_points_total=op_total,
                    object_points_passes=op_pass,
                    object_voxels_us=round(ov_us, 2), object_voxels_total=ov_total,
                    object_voxels_passes=dict(zip(STAGE, ov_pass)),
                    single_frame_us=round(sum(single["frame"]), 2),
                    single_object_points_us=round(sum(single["points"]), 2),
                    single_object_voxels_us=round(sum(single["voxels"]), 2),
                    single_object_points_each=[round(v, 2) for v in single["points"]],
                    single_object_voxels_each=[round(v, 2) for v in single["voxels"]])
        print(json.dumps(line), flush=True)
        lines.append(line)
    # the segmented table alone on the batch's coords, next to §14's table on composite cells built
    # ahead of time: the difference is what the starts, the composite pass and the finish cost
    ps, _ = gpu.batch_ranges()
    coords = gpu.downloadVoxelCoords()
    frame_of = np.repeat(np.arange(N, dtype=np.uint64), np.diff(ps.astype(np.int64)))
    comp = np.where(coords < cells, frame_of * cells + coords, 0xFFFFFFFF).astype(np.uint32)
    d_coords, d_ps, d_comp = (hiprt.DeviceArray.from_numpy(x) for x in (coords, ps, comp))
    seg.set_stream(gpu.stream())
    seg_us = median_us(timer, lambda: seg.voxel_table_segments(d_coords.ptr, n, d_ps.ptr, N, cells),
                       a.calls, a.warmup)
    G, _ = seg.voxel_table_counts()
    comp_us = median_us(timer, lambda: seg.voxel_table(d_comp.ptr, n, N * cells), a.calls, a.warmup)
    line = dict(cloud=f"{a.size}_batch{N}_table", frames=N, n=n, G=G, cells=cells, calls=a.calls,
                table_segments_us=round(seg_us, 2), table_on_composites_us=round(comp_us, 2))
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
