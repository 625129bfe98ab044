#!/usr/bin/env python3
"""How much of the px mask / emit kernels' work the crop box discards, counted on the CPU.

No GPU and no oracle: the synthetic frames of the benchmark (synth), the launch-default crop box
and the px kernels' mapping of pixels to work units - a segment is 256 consecutive pixels of a
camera row (the last one of a row shorter), and wave w of its two waves owns columns
64w..64w+63 and 128+64w..128+64w+63 of it.  Per workload, four fractions:

  rings_today    pixels that enter the flying-pixel rings with the crop evaluated last
                 (depth != 0 and inside max_distance), of all pixels
  rings_crop     the same with the crop evaluated first (... and inside the crop box)
  waves_empty    waves without a single such pixel (they leave the ring loop at its first
                 wave-uniform exit), of the waves that own a pixel
  segs_empty     segments without one (k_emit_px2's blocks with nothing to write; the flying
                 filter can only empty more), of all segments

The point arithmetic is the kernels' in float32 (z = d * scale, x = xn z, y = yn z, the crop
rows as ((m0 x + m1 y) + m2 z) + m3); a pixel on the very edge of the box may fall differently
than on the GPU, which does not move a fraction's printed digits.

  python tools/crop_stats.py            # the four workloads of the DESIGN table
  python tools/crop_stats.py --json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEGW = 256
MAX_DIST_SQ = np.float32(np.uint32(0x42C80001).view(np.float32))  # sqrt(pp) > 10 <=> pp > this
WORKLOADS = (("VGA dense", 640, 480, "dense", 8), ("VGA stress", 640, 480, "stress", 8),
             ("720p dense", 1280, 720, "dense", 4), ("4K dense", 3840, 2160, "dense", 1))


def live_masks(cam, depth, crop_min, crop_max):
    """(before the crop, after it): the pixels of one depth map that enter the rings."""
    f32 = np.float32
    H, W = depth.shape
    xn = ((np.arange(W, dtype=f32) - f32(cam.cx)) / f32(cam.fx)).astype(f32)
    yn = ((np.arange(H, dtype=f32) - f32(cam.cy)) / f32(cam.fy)).astype(f32)
    z = depth.astype(f32) * f32(cam.depth_scale)
    x, y = xn[None, :] * z, yn[:, None] * z
    pp = (x * x + y * y) + z * z
    live = (depth != 0) & ~(pp > MAX_DIST_SQ)
    T = np.asarray(cam.T_crop, f32)
    out = np.zeros(depth.shape, bool)
    for ax in range(3):
        q = ((T[ax, 0] * x + T[ax, 1] * y) + T[ax, 2] * z) + T[ax, 3]
        out |= (q < f32(crop_min[ax])) | (q > f32(crop_max[ax]))
    return live, live & ~out


def unit_counts(kept):
    """(waves that own a pixel, of them empty, segments, of them empty) of one H x W mask."""
    H, W = kept.shape
    waves = waves_empty = segs = segs_empty = 0
    for x0 in range(0, W, SEGW):
        seg = kept[:, x0:x0 + SEGW]
        n = seg.shape[1]
        segs += H
        segs_empty += int(np.count_nonzero(~seg.any(axis=1)))
        for w in range(2):
            if 64 * w >= n:
                continue
            cols = np.r_[64 * w:64 * w + 64, 128 + 64 * w:128 + 64 * w + 64]
            own = seg[:, cols[cols < n]]
            waves += H
            waves_empty += int(np.count_nonzero(~own.any(axis=1)))
    return waves, waves_empty, segs, segs_empty


def crop_stats(width, height, workload="dense", frames=1, camera=0, crop_min=None, crop_max=None):
    """The four fractions over `frames` frames of camera `camera`."""
    from ros_gpu_depthmap_fusion_amd import synth
    from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams
    p = ComponentParams()
    lo = p.crop_min if crop_min is None else crop_min
    hi = p.crop_max if crop_max is None else crop_max
    cam = synth.make_camera(camera, width, height)
    tot = np.zeros(7, np.int64)  # pixels, live, live & crop, waves, empty, segments, empty
    for f in range(frames):
        live, kept = live_masks(cam, synth.WORKLOADS[workload](cam, camera, f), lo, hi)
        tot += (live.size, np.count_nonzero(live), np.count_nonzero(kept), *unit_counts(kept))
    return {"rings_today": tot[1] / tot[0], "rings_crop": tot[2] / tot[0],
            "waves_empty": tot[4] / tot[3], "segs_empty": tot[6] / tot[5]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    args = ap.parse_args()
    rows = {name: crop_stats(W, H, wl, n) for name, W, H, wl, n in WORKLOADS}
    if args.json:
        print(json.dumps({k: {m: round(float(v), 4) for m, v in r.items()} for k, r in rows.items()}))
        return
    print("camera 0, launch defaults; share of the px kernels' work units without a pixel "
          "inside the crop box")
    print("%-12s %7s %12s %12s %12s %12s" % ("frames", "count", "rings today", "crop first",
                                              "empty waves", "empty segs"))
    for (name, _, _, _, n) in WORKLOADS:
        r = rows[name]
        print("%-12s %7d %11.1f%% %11.1f%% %11.1f%% %11.1f%%" % (
            name, n, 100 * r["rings_today"], 100 * r["rings_crop"], 100 * r["waves_empty"],
            100 * r["segs_empty"]))


if __name__ == "__main__":
    main()
