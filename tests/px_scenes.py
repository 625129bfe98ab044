"""Scenes for the two-pixel compaction kernels (k_mask_px / k_mask_px_o8 / k_emit_px2 and the
640-pixel and emit-partition forms), importable without a GPU: depth maps, cameras, parameters,
the oracle's per-frame results, and per scene the assertion - from the oracle's stage masks, on
the CPU - that the scene holds the case it was built for.  tests/test_px_scenes.py builds every
scene and checks those assertions without a GPU; tests/test_gpu_px_shapes.py and
tests/test_gpu_crop_first.py run the scenes through the engine.

How the engine picks the kernels (gdf_engine.cpp upload_depthmaps, gdf_kernels.hip mask_kernel /
emit_kernel): a camera's rows are split into nchunk = ceil(W / seg_items) segments of
segw = roundup64(ceil(W / nchunk)) pixels, seg_items = GDF_SEG_ITEMS, or 256 for launches over
1 Mi depth pixels, else 1024.  The 256-pixel px kernels run when the widest segment of the launch
is 256 (F = 4, no rot45, no debug masks): under GDF_SEG_ITEMS=256 that is W in 193..256,
385..512, 577..768.  The 640 forms run at segw = 640 with at least 1024 segments.  In a segment
at column x0 thread t of SEGW / 2 owns the pixels x0 + t and x0 + t + SEGW / 2; wave w's pixel j
is validity word w + (SEGW / 128) j.
"""
import dataclasses
import functools

import numpy as np

from oracle import OracleFusion
from ros_gpu_depthmap_fusion_amd import synth
from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams

PX_ENV = {"GDF_SEG_ITEMS": "256"}  # the knob every small px scene runs under
K_MASK_O8, K_MASK_PX, K_EMIT_PX = "k_mask_px_o8<2,256>", "k_mask_px<2,256>", "k_emit_px2<256>"
K_EMIT_PARTS = "k_emit_px2_parts<256>"
K_MASK_640, K_EMIT_640 = "k_mask_px<2,640>", "k_emit_px2<640>"
K_MASK, K_EMIT = "k_mask<false,4>", "k_emit"

NEAR, PLANE = 1000, 3000  # mm: in front of the crop boxes of the plane scenes (x < 2 m) / inside


def segments(W, seg_items):
    """[(x0, len)] of a row's compaction segments, and segw (the engine's split, see above)."""
    nchunk = (W + seg_items - 1) // seg_items
    segw = ((W + nchunk - 1) // nchunk + 63) // 64 * 64
    return [(x0, min(segw, W - x0)) for x0 in range(0, nchunk * segw, segw)], segw


def px_eligible(W, seg_items=256):
    return segments(W, seg_items)[1] == 256


def wave_columns(x0, length, wave, segw=256):
    """The columns wave `wave` of the px kernels owns in the segment (x0, length)."""
    half = segw // 2
    t = np.arange(64 * wave, 64 * wave + 64)
    c = np.concatenate([t, t + half])
    return x0 + c[c < length]


def cam_args(cam, depth):
    return (depth, *cam.intrinsics(), cam.T_world, cam.T_crop)


def box_params(lo, hi):
    """Launch defaults with the crop box (lo, hi); the voxel grid keeps its default bounds."""
    p = ComponentParams()
    p.crop_min, p.crop_max = lo, hi
    return p


def run_oracle(frames_of_cams, p):
    """Frame by frame through the oracle (one engine, the grid's history carried on): per frame
    its results and stage masks (maskB: after the flying filter, maskA: after the crop), copied."""
    orc = OracleFusion(threads=8)
    out = []
    for args in frames_of_cams:
        orc.clear()
        for a in args:
            orc.addDepthmap(*a)
        orc.processFrame(p)
        st = orc.stage_arrays()
        out.append({"points": orc.downloadPoints().copy(), "keys": orc.downloadVoxelCoords().copy(),
                    "vox": orc.downloadVoxelizedPoints()[:, :3].copy(),
                    "grid": orc.downloadVoxelOccupancyGrid().copy(),
                    "hist": orc.historic_grid().copy(),
                    "maskA": st["maskA"].copy() != 0, "maskB": st["maskB"].copy() != 0})
    return out


@dataclasses.dataclass
class Scene:
    params: ComponentParams
    frames: list  # per frame the cameras' addDepthmap arguments
    ref: list     # the oracle's per-frame results (run_oracle)

    def __iter__(self):  # (params, frames, ref)
        return iter((self.params, self.frames, self.ref))

    def masks(self, frame=0):
        """Per camera of the frame its (maskA, maskB) as H x W images."""
        out, o = [], 0
        for a in self.frames[frame]:
            H, W = a[0].shape
            r = self.ref[frame]
            out.append((r["maskA"][o:o + H * W].reshape(H, W), r["maskB"][o:o + H * W].reshape(H, W)))
            o += H * W
        return out


# ---- the crop-first scenes (tests/test_gpu_crop_first.py) ---------------------------------------
# The camera looks along world +x from 1 m above the ground: a fronto-parallel plane at depth d
# has world x = d and z = 1 - yn d, so the plane at 3 m has z = 1 - 3 (v - H / 2) / (0.6 W) in row
# v.  A box 2..6 x -20..20 x zlo..zhi keeps whole rows of it, on a smooth surface - the flying
# filter passes across the cut.  Per width the box that keeps rows 10..28 of a 32-row image and
# crops rows 0..9 (too high) and 29..31 (too low), and the one that keeps rows 5..11 of 16 rows:
#   W = 320 (fy 192):   rows 10..28: 0.8 .. 1.1,    rows 5..11: 0.95 .. 1.06
#   W = 448 (fy 268.8): rows 10..28: 0.86 .. 1.07,  rows 5..11: 0.96 .. 1.04
CROP_H, CROP_H2 = 32, 16
BATCH_Z = {320: (0.8, 1.1), 448: (0.86, 1.07)}
TWOCAM_Z = {320: (0.95, 1.06), 448: (0.96, 1.04)}
ROWS_KEPT = (10, 28)
MID_ROW = 6           # scene 1: cropped, with clean rows 2..10 around it
WAVE_ROWS = (12, 22)  # scene 3: rows whose wave-0 columns stand at 1 m
ZERO_ROW, NOISE_ROW = 20, 25  # scene 5, frame 1
SEG = 256             # the first segment of a row at both widths' px layout


def crop_layout(W):
    """(segments of a row, wave 0's columns, wave 1's columns of the first segment) as the px
    kernels see a row of W pixels under GDF_SEG_ITEMS=256.  W = 320 is not px-eligible (one
    k_mask segment of 320): its scene keeps the column sets of the 256-pixel layout, as geometry
    only."""
    segs = segments(W, 256)[0] if px_eligible(W) else [(0, SEG), (SEG, W - SEG)]
    return segs, wave_columns(0, SEG, 0), wave_columns(0, SEG, 1)


def batch_frames(W):
    H = CROP_H
    segs, wave0, _ = crop_layout(W)
    f0 = np.full((H, W), PLANE, np.uint16)
    f0[WAVE_ROWS[0]:WAVE_ROWS[1] + 1, wave0] = NEAR
    if px_eligible(W):  # the same in the row's last segment (192 pixels: wave 1 has no second pixel)
        x0, n = segs[-1]
        f0[WAVE_ROWS[0]:WAVE_ROWS[1] + 1, wave_columns(x0, n, 0)] = NEAR
    f1 = np.full((H, W), PLANE, np.uint16)
    f1[ZERO_ROW, :SEG] = 0
    # a sawtooth of 0.3 m steps with period 5 (2.6 .. 3.8 m, inside the box): the left and right
    # neighbours of every ring stand at different depths, no pixel finds a surface
    f1[NOISE_ROW, :SEG] = (2600 + 300 * (np.arange(SEG) % 5)).astype(np.uint16)
    f2 = np.full((H, W), PLANE, np.uint16)
    f2[14:19, 40:90] = 0  # a hole, so that the last frame is not a copy of a plane
    return [f0, f1, f2]


@functools.lru_cache(maxsize=None)
def crop_scene(name, W=448):
    """The crop-first scenes at width W: "batch" (three W x 32 frames), "nocrop" (a dense W x 32
    frame, the box at +-1e9), "twocam" (two W x 16 cameras in one frame)."""
    if name == "batch":
        cam = synth.make_camera(0, W, CROP_H)
        zlo, zhi = BATCH_Z[W]
        p = box_params((2.0, -20.0, zlo), (6.0, 20.0, zhi))
        frames = [[cam_args(cam, d)] for d in batch_frames(W)]
    elif name == "nocrop":
        cam = synth.make_camera(0, W, CROP_H)
        p = box_params((-1e9, -1e9, -1e9), (1e9, 1e9, 1e9))
        frames = [[cam_args(cam, synth.dense_frame(cam, 0, 3))]]
    elif name == "twocam":
        cams = synth.cameras(2, W, CROP_H2)
        zlo, zhi = TWOCAM_Z[W]
        p = box_params((-10.0, -20.0, zlo), (30.0, 20.0, zhi))
        d = np.full((CROP_H2, W), PLANE, np.uint16)
        frames = [[cam_args(c, d) for c in cams]]
    else:
        raise KeyError(name)
    sc = Scene(p, frames, run_oracle(frames, p))
    crop_scene_contents(name, W, sc)
    return sc


def crop_scene_contents(name, W, sc):
    """The cases the crop-first scenes must contain, asserted from the oracle's stage masks
    (maskB: after the flying filter, maskA: after the crop) and the depth maps."""
    frames, ref = sc.frames, sc.ref
    H = CROP_H
    segs, WAVE0, WAVE1 = crop_layout(W)
    if name == "nocrop":
        r = ref[0]
        assert np.array_equal(r["maskA"], r["maskB"]) and r["maskA"].any()  # 6: the crop is off
        for x0, n in segs:  # (every segment of a row keeps pixels somewhere)
            assert r["maskA"].reshape(H, W)[:, x0:x0 + n].any()
        return
    if name == "twocam":
        r = ref[0]
        A = r["maskA"].reshape(2, CROP_H2, W)
        B = r["maskB"].reshape(2, CROP_H2, W)
        for k in range(2):
            assert A[k, 5:12].any() and not A[k, :5].any() and not A[k, 12:].any()
            # 7: empty segments of both cameras that only the crop empties
            assert B[k, 4, 4:SEG].all() and B[k, 4, SEG:W - 4].all()
        return
    depth = [f[0][0] for f in frames]
    A = [r["maskA"].reshape(H, W) for r in ref]
    B = [r["maskB"].reshape(H, W) for r in ref]
    # 1: a mid-frame segment, every pixel valid, flying-clean (columns 4.. of the row's first
    # segment, columns ..W-5 of its last), nothing kept
    assert (depth[0][MID_ROW, :SEG] != 0).all()
    assert B[0][MID_ROW, 4:SEG].all() and not A[0][MID_ROW, :SEG].any()
    assert (depth[0][MID_ROW, SEG:] != 0).all()
    assert B[0][MID_ROW, SEG:W - 4].all() and not A[0][MID_ROW, SEG:].any()
    # 2: the first segment of frames 1 and 2, and the last segment of the last frame: valid
    # depth, outside the box (the plane of their rows is cropped: their clean neighbours in the
    # rows next to them are), nothing kept
    for f in (1, 2):
        assert (depth[f][0, :SEG] != 0).all() and not A[f][0, :SEG].any()
        assert B[f][4, 4:SEG].all() and not A[f][:ROWS_KEPT[0]].any()
    assert (depth[2][H - 1, SEG:] != 0).all() and not A[2][H - 1, SEG:].any()
    assert B[2][H - 5, 4:W - 4].all() and not A[2][ROWS_KEPT[1] + 1:].any()
    # 3: wave 0's 128 pixels valid and cropped, wave 1 keeps pixels, in one segment
    y = (WAVE_ROWS[0] + WAVE_ROWS[1]) // 2
    assert len(WAVE0) == 128 and len(WAVE1) == 128
    assert (depth[0][y, WAVE0] == NEAR).all() and not A[0][y, WAVE0].any()
    assert B[0][y, WAVE0[8:56]].all() and B[0][y, WAVE0[72:120]].all()  # (clean away from steps)
    assert A[0][y, WAVE1].sum() >= 64
    if px_eligible(W):
        # 3b: the same in the row's last, shorter segment: wave 0's pixels (both of each thread)
        # cropped, wave 1 - whose second pixels lie past the row's end - keeps pixels away from
        # the steps (4 columns at either end of its 64 fail the filter)
        x0, n = segs[-1]
        w0, w1 = wave_columns(x0, n, 0), wave_columns(x0, n, 1)
        assert n < SEG and len(w0) == 128 and len(w1) == 64
        assert (depth[0][y, w0] == NEAR).all() and not A[0][y, w0].any()
        assert A[0][y, w1].sum() >= 48
    # 4: kept pixels with a depth-valid neighbour outside the crop (flying-clean and not kept:
    # the crop alone removed it) within 4 pixels in a row or a column
    out = B[0] & ~A[0]
    near = np.zeros((H, W), bool)
    for i in range(1, 5):
        near[i:, :] |= out[:-i, :]
        near[:-i, :] |= out[i:, :]
        near[:, i:] |= out[:, :-i]
        near[:, :-i] |= out[:, i:]
    assert np.count_nonzero(A[0] & near) >= 50
    # 5: a segment without depth, and one with depth, inside the box, emptied by the filter
    assert not depth[1][ZERO_ROW, :SEG].any() and not A[1][ZERO_ROW, :SEG].any()
    d = depth[1][NOISE_ROW, :SEG].astype(np.float64) * 1e-3
    z = 1.0 - (NOISE_ROW - H / 2) / (0.6 * W) * d
    zlo, zhi = BATCH_Z[W]
    assert (d > 2.1).all() and (d < 5.9).all() and (z > zlo + 0.01).all() and (z < zhi - 0.01).all()
    assert not B[1][NOISE_ROW, :SEG].any()
    assert A[1][NOISE_ROW + 1, SEG:W - 4].all()  # (the rows around it still keep pixels)


# ---- small shapes for the 256-pixel px kernels (tests/test_gpu_px_shapes.py) --------------------
WIDTHS = (193, 199, 256, 385, 391, 448, 449, 512, 577)
WIDTH_H = 24
HEIGHTS = (1, 4, 5, 8, 9, 12)
HEIGHT_W = 391


WRAP_K = 2  # the synthetic camera of the width scenes (yaw 90 degrees: depth at both image edges)
WRAP_THRESHOLDS = (-0.3, -0.4, -0.5, -0.6, -0.7) + tuple(round(-0.71 - 0.01 * i, 2) for i in range(10)) + \
    (-0.85, -0.9, -0.95)


def _width_frames(W):
    cam = synth.make_camera(WRAP_K, W, WIDTH_H)
    return [[cam_args(cam, synth.dense_frame(cam, WRAP_K, 0))]]


@functools.lru_cache(maxsize=None)
def width_scene(W, wrap=False):
    """A dense synthetic W x 24 frame.  wrap False: the launch defaults, for the row tails.
    wrap True: the same frame with a flying-pixel threshold under which the row-start columns
    0..3 keep points.  Their left neighbours are the previous row's LAST pixels (linear index), so
    right - left spans the whole image backwards and the surface normal through them points away
    from the camera: cos = -0.7 .. -1 on a real surface, and no depth map passes the launch
    default 0.3 there at these focal lengths (the angle between the rays of columns x and x + 4
    is 4 / fx < asin 0.3).  The threshold is the first of WRAP_THRESHOLDS under which every one of
    the four columns keeps a point in some row >= 4, and, where one exists, not in every row (so
    that the values read across the wrap decide, not only their validity)."""
    assert px_eligible(W)
    frames = _width_frames(W)
    if not wrap:
        p = ComponentParams()
        sc = Scene(p, frames, run_oracle(frames, p))
        width_scene_contents(W, sc, wrap)
        return sc
    full = None
    for thr in WRAP_THRESHOLDS:
        p = ComponentParams()
        p.flying_threshold = thr
        sc = Scene(p, frames, run_oracle(frames, p))
        kept = sc.masks()[0][0][4:WIDTH_H - 4, :4].sum(axis=0)
        if kept.all() and not (kept == WIDTH_H - 8).all():
            full = sc
            break
        if kept.all() and full is None:
            full = sc
    assert full is not None, "no threshold keeps the wrap columns"
    width_scene_contents(W, full, wrap)
    return full


def width_scene_contents(W, sc, wrap):
    """wrap False: the oracle keeps at least 64 points in the last segment of some row - or all
    that can be kept where the segment is shorter than 68: its last four columns are the row's,
    which fail the filter's bounds test (W = 577: tail 65, 61 points).  wrap True: the row-start
    segments of rows >= 4 (the kRowStart waves) keep a point in each of the columns 0..3."""
    (A, _), = sc.masks()
    segs, _ = segments(W, 256)
    x0, n = segs[-1]
    if wrap:
        assert A[4:, :4].any(axis=0).all()
    else:
        assert A[:, x0:x0 + n].sum(axis=1).max() >= min(64, n - 4)


def textured_plane(W, H, base, salt):
    """A plane at `base` mm with smooth bumps of +-20 mm and 0.4 % single-pixel holes."""
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    d = base + 12.0 * np.sin(x / 9.0 + 0.7 * y + salt) + 8.0 * np.cos(x / 23.0 - 0.3 * y)
    h = synth.splitmix64(np.uint64(0xD1CE0000 + salt) ^ np.arange(W * H, dtype=np.uint64))
    return np.where(synth.uniform01(h).reshape(H, W) < 0.004, 0.0, np.rint(d)).astype(np.uint16)


def stripe_camera(k, W, H, rows_below):
    """synth.make_camera with the principal point rows_below rows farther down: the camera sees
    the stripe of a taller image that ends rows_below rows above that image's centre line.  The
    flying filter reads the neighbours above rows 0..3 of a camera that is not its frame's first
    from the previous camera's last rows (linear index); they pass as a surface only if those
    pixels' points lie above this camera's - as the stripe above it of one sensor does."""
    c = synth.make_camera(k, W, H)
    return dataclasses.replace(c, cy=float(H / 2 + rows_below))


@functools.lru_cache(maxsize=None)
def height_scene(H, two):
    """391 x H: a single camera, or (two) the second of two equal cameras in one frame - the two
    stripes of one 391 x 2H image - whose rows 0..3 read the first camera's last rows by linear
    index."""
    W = HEIGHT_W
    p = ComponentParams()
    img = textured_plane(W, 2 * H, 1500, 1)
    lower = synth.make_camera(0, W, H)
    cams = [cam_args(lower, img[H:])]
    if two:
        cams.insert(0, cam_args(stripe_camera(0, W, H, H), img[:H]))
    sc = Scene(p, [cams], run_oracle([cams], p))
    (A, _) = sc.masks()[-1]
    if not two and H <= 8:  # no row has four rows above and below it
        assert len(sc.ref[0]["points"]) == 0 and not sc.ref[0]["grid"].any()
    if two and H >= 5:  # the kGeneral rows of the px kernel
        assert A[:4].sum() >= 16
    if H >= 9:
        assert A[4:H - 4].any()
    return sc


@functools.lru_cache(maxsize=None)
def mixed_scene(h0=7):
    """Three cameras in one frame, in this order: 199 x h0, 448 x 12, 96 x 10, each looking at
    the stripe above the next one's.  The first camera's pixel count is odd (the next staged map
    starts at a 2-byte-odd offset), the third has 128-pixel segments inside the 256-thread launch.
    h0 = 7, the stated case: no row of the first camera has four rows above and below it, so it
    keeps nothing; h0 = 9: every camera keeps points."""
    p = ComponentParams()
    shapes = [(199, h0, h0 / 2 + 20), (448, 12, 30), (96, 10, 0)]
    assert (shapes[0][0] * shapes[0][1]) % 2 == 1
    assert segments(96, 256)[1] == 128 and max(segments(s[0], 256)[1] for s in shapes) == 256
    cams = []
    for k, (W, H, below) in enumerate(shapes):
        cams.append(cam_args(stripe_camera(k, W, H, below), textured_plane(W, H, 1000, 3 + k)))
    sc = Scene(p, [cams], run_oracle([cams], p))
    m = sc.masks()
    assert m[1][0].any() and m[2][0].any()
    assert m[1][0][:4].any()  # camera 1's rows 0..3: neighbours in camera 0 by linear index
    if h0 >= 9:
        assert m[0][0].any()
    else:
        assert not m[0][0].any()
    return sc


@functools.lru_cache(maxsize=None)
def replay_scene(W=449, n=4):
    """The W x 24 frame of width_scene n times in a row, as single frames (not a batch): the
    engine launches the first directly, captures the second into a graph and replays that from
    the third on; the oracle carries the grid's history through the n frames."""
    p = ComponentParams()
    frames = _width_frames(W) * n
    return Scene(p, frames, run_oracle(frames, p))


DEVICE_OFFSETS = (2, 6, 14)  # bytes: where the 391 x 12 map starts, modulo 16


def device_scene():
    """The 391 x 12 single-camera map of height_scene, taken through device pointers."""
    return height_scene(12, False)


@functools.lru_cache(maxsize=None)
def empty_batch_scene(all_empty):
    """448 x 16, four frames: frames 1 and 3 all-zero depth, or every frame."""
    W, H = 448, 16
    p = ComponentParams()
    cam = synth.make_camera(0, W, H)
    zero = np.zeros((H, W), np.uint16)
    maps = [zero if all_empty or j % 2 else synth.dense_frame(cam, 0, j) for j in range(4)]
    frames = [[cam_args(cam, d)] for d in maps]
    sc = Scene(p, frames, run_oracle(frames, p))
    for j, r in enumerate(sc.ref):
        if all_empty or j % 2:
            assert len(r["points"]) == 0 and len(r["vox"]) == 0
        else:
            assert len(r["points"]) >= 256
    return sc


# ---- the 640-pixel forms at their product shapes (no knob) --------------------------------------
P640_W = 1211


@functools.lru_cache(maxsize=None)
def p640_scene(ncams):
    """One camera 1211 x 720 (segments of 640 + 571, 1440 segments) or two cameras 1211 x 400:
    the fronto-parallel plane at 3 m of the crop-first scenes, a box that keeps a band of rows,
    a nearer patch and a hole inside the band."""
    W = P640_W
    H = 720 if ncams == 1 else 400
    keep = (250, 500) if ncams == 1 else (100, 300)
    fy = float(np.float32(0.6 * W))

    def z(v):
        return 1.0 - 3.0 * (v - H / 2) / fy
    p = box_params((-10.0, -20.0, z(keep[1] + 0.5)), (30.0, 20.0, z(keep[0] - 0.5)))
    d = np.full((H, W), PLANE, np.uint16)
    ym = (keep[0] + keep[1]) // 2
    d[ym:ym + 20, 600:700] = 2900  # (a step across the segment boundary at column 640)
    d[ym + 40:ym + 50, 1100:1211] = 0
    cams = [cam_args(c, d) for c in synth.cameras(ncams, W, H)]
    sc = Scene(p, [cams], run_oracle([cams], p))
    segs, segw = segments(W, 1024)
    assert segw == 640 and H * len(segs) * ncams >= 1024 and W * H * ncams < (1 << 20)
    # at least 30 % of the segments are empty by the crop alone (valid depth in every pixel,
    # pixels that pass the flying filter, nothing kept), the frame's last segment among them
    empty, total, last = 0, 0, False
    for k, (A, B) in enumerate(sc.masks()):
        assert A[keep[0]:keep[1] + 1].any()
        for y in range(H):
            for x0, n in segs:
                # (the first and last four rows fail the filter's bounds test: there the rows
                # next to them show that only the crop empties the plane)
                clean = B[y, x0:x0 + n].any() if 4 <= y < H - 4 else not keep[0] <= y <= keep[1]
                last = bool(not A[y, x0:x0 + n].any() and clean and (d[y, x0:x0 + n] != 0).all())
                empty += last
                total += 1
    assert total == H * len(segs) * ncams and empty >= 0.3 * total and last
    return sc
