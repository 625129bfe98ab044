"""Built scenes of the segmentation tests (test_seg_scenes.py on the CPU, test_gpu_segment_shapes.py
on the GPU): uint8 grids (L, H, W) aimed at the edges of the kernels of gdf_segment.hip, which
random blobs meet by chance or not at all.  The kernel constants the scenes aim at are restated
below; test_seg_scenes.py proves that every scene still holds its case.

`census(layer)` counts the raster scan's events by kind (seg_ref.external_contours' census hook):
the scan of k_cc_contours reads a row SCAN_STEP padded columns at a time and keeps the row's last
marked run start (lnbd) and its value across those steps, so what matters is in which step lnbd
lies when a start is judged.
"""
import numpy as np

import seg_ref

TILE = 32           # pixels per side of a k_cc_local / k_cc_merge tile (16 blocks of 2 x 2)
WAVE_COLS, WAVE_ROWS = 64, 8   # k_cc_pixels: one wave per 64 columns x 8 rows
SCAN_STEP = seg_ref.SCAN_STEP  # k_cc_contours: padded columns per step of the row scan
ROW_FLAGS = 64      # k_cc_contours: padded rows per row-flag ballot
RANK_WAVES, RANK_STEP = 16, 64  # k_cc_rank: 16 waves, 64 blocks per step
MERGE_CHUNK = 1024  # k_cc_merge_layers: threads = labels per stride / per scan chunk
PACK_THREADS = 256  # k_cc_pack_contours: layers summed per pass
LDS_MAX = 160 * 1024
assert SCAN_STEP == 256


def contour_image_bytes(W, H):
    """The staged image of k_cc_contours: H + 2 rows of pitch roundup4(W + 2), then H + 2 row
    flags rounded up to 4 (gdf_segment.hip, contour_image_bytes)."""
    pitch = (W + 2 + 3) // 4 * 4
    return pitch * (H + 2) + (H + 2 + 3) // 4 * 4


def census(layer) -> dict:
    """Event counts of the raster scan of one layer (H, W); see seg_ref.external_contours."""
    c = {"taken": 0, "skipped": 0, "skipped_lnbd_earlier_step": 0, "taken_lnbd_earlier_step": 0,
         "second_start_stale_lnbd": 0, "skipped_lnbd_run_start_earlier_step": 0,
         "start_at_step_edge": {SCAN_STEP - 1: 0, 0: 0, 1: 0}}
    seg_ref.external_contours(np.asarray(layer), census=c)
    return c


def tiles_of(mask):
    """The set of (tile row, tile column) holding a pixel of the boolean mask."""
    ys, xs = np.nonzero(mask)
    return set(zip((ys // TILE).tolist(), (xs // TILE).tolist()))


def _ring(g, y0, y1, x0, x1, v=1):
    g[y0, x0:x1 + 1] = v
    g[y1, x0:x1 + 1] = v
    g[y0:y1 + 1, x0] = v
    g[y0:y1 + 1, x1] = v


# ---- tiles ------------------------------------------------------------------------------------------
def tile_diagonals():
    """20-pixel one-pixel diagonals about the tile corner (32, 32): z = 4 * direction + 2 * dx + dy;
    direction 0 runs down-right from (22 + dy, 22 + dx), direction 1 down-left from
    (22 + dy, 45 + dx).  The main diagonals with dx == dy pass exactly through the corner (pixels
    (31, 31) and (32, 32): the up-left link of k_cc_merge with lx == ly == 0) and so lie in two
    tiles; every other layer lies in three (its links cross one border as a diagonal and the
    other one block later)."""
    g = np.zeros((8, 70, 70), np.uint8)
    i = np.arange(20)
    for dx in (0, 1):
        for dy in (0, 1):
            g[2 * dx + dy, 22 + dy + i, 22 + dx + i] = 1
            g[4 + 2 * dx + dy, 22 + dy + i, 45 + dx - i] = 1
    return g


def tile_corner_antidiagonals():
    """The anti-diagonals that tile_diagonals lacks: down-left from (22 + dy, 41 + dx), x + y =
    63 + dx + dy; the first passes exactly through the corner (pixels (31, 32) and (32, 31): the
    up-right link with lx == 15 and ly == 0)."""
    g = np.zeros((4, 70, 70), np.uint8)
    i = np.arange(20)
    for dx in (0, 1):
        for dy in (0, 1):
            g[2 * dx + dy, 22 + dy + i, 41 + dx - i] = 1
    return g


NEAR_MISS_PAIRS = [((10, 30), (10, 32)), ((30, 10), (32, 10)), ((30, 30), (32, 32)),
                   ((31, 40), (33, 42))]


def tile_near_misses():
    """Pixel pairs two apart across x = 32, across y = 32, across the corner, and diagonally across
    y = 32 away from the corner: no pair is linked."""
    g = np.zeros((1, 70, 70), np.uint8)
    for a, b in NEAR_MISS_PAIRS:
        g[0][a] = 1
        g[0][b] = 1
    return g


def serpentine():
    """Full rows every second line, joined alternately at the right and left ends; layer 1 is
    layer 0 flipped vertically."""
    H, W = 67, 97
    a = np.zeros((H, W), np.uint8)
    a[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        a[y, W - 1 if k % 2 == 0 else 0] = 1
    return np.stack([a, a[::-1]])


def combs():
    """Teeth on even columns, joined by a full bottom row (layer 0) or a full top row (layer 1)."""
    g = np.zeros((2, 70, 131), np.uint8)
    g[:, :, 0::2] = 1
    g[0, 69] = 1
    g[1, 0] = 1
    return g


def interlocked_combs():
    """Comb A: teeth on x = 0 (mod 4), rows 0..36, joined on row 0; comb B: teeth on x = 2 (mod 4),
    rows 3..39, joined on row 39."""
    g = np.zeros((1, 40, 131), np.uint8)
    g[0, 0:37, 0::4] = 1
    g[0, 0] = 1
    g[0, 3:40, 2::4] = 1
    g[0, 39] = 1
    return g


ROOT_SHAPES = [(64, 64), (64, 66), (1, 2050), (2, 2049)]   # (H, W): 1024, 1056, 1025, 1025 blocks


def every_block_a_root(H, W):
    """Cells at even x and even y: every 2 x 2 block is a component of its own."""
    g = np.zeros((1, H, W), np.uint8)
    g[0, 0::2, 0::2] = 1
    return g


def root_blocks(H, W):
    return ((H + 1) // 2) * ((W + 1) // 2)


def root_labels(H, W):
    """Closed form of every_block_a_root's labels: block rank + 1 on the cells."""
    BW = (W + 1) // 2
    y, x = np.mgrid[0:H, 0:W]
    lab = (y // 2) * BW + x // 2 + 1
    return np.where((y % 2 == 0) & (x % 2 == 0), lab, 0).astype(np.uint16)


BAR_WIDTHS = [63, 64, 65, 129]
BAR_H = 17


def wave_bars(W):
    """Full-width bars on rows 7 and 8 (one component across the 8-row wave edge), a full-width bar
    on row 15 and a half-width bar on row 16 below it (a second component, rows of unequal runs)."""
    g = np.zeros((1, BAR_H, W), np.uint8)
    g[0, 7:9] = 1
    g[0, 15] = 1
    g[0, 16, :W // 2] = 1
    return g


def wave_bars_closed_form(W):
    """(stats [3, 5], centroids [3, 2]) of wave_bars(W) from sums over the bars."""
    h = W // 2
    s = lambda n: n * (n - 1) // 2          # 0 + 1 + ... + (n - 1)
    a1, a2 = 2 * W, W + h
    a0 = BAR_H * W - a1 - a2
    sx1, sy1 = 2 * s(W), 7 * W + 8 * W
    sx2, sy2 = s(W) + s(h), 15 * W + 16 * h
    sx0, sy0 = BAR_H * s(W) - sx1 - sx2, W * s(BAR_H) - sy1 - sy2
    stats = np.array([[0, 0, W, BAR_H, a0], [0, 7, W, 2, a1], [0, 15, W, 2, a2]], np.int32)
    cent = np.array([[sx0 / a0, sy0 / a0], [sx1 / a1, sy1 / a1], [sx2 / a2, sy2 / a2]], np.float64)
    return stats, cent


# ---- the row scan's steps ---------------------------------------------------------------------------
def rings_across_step():
    """Six nested one-pixel rings whose left sides lie in the first scan step and whose right sides
    in the second, and a 2 x 4 island in the innermost hole right of the step edge: every start
    inside the outer ring is skipped, most of them on lnbd's cached value."""
    g = np.zeros((1, 40, 300), np.uint8)
    for k in range(0, 12, 2):
        _ring(g[0], 2 + k, 37 - k, 230 + k, 290 - k)
    g[0, 19:21, 258:262] = 1
    return g


def thick_ring_across_step():
    """A ring with walls three pixels thick, its left wall (x 240..242) in the first scan step, and
    a 2 x 4 island in its hole right of the step edge.  Only the wall's outer pixels are marked,
    so on the island's rows lnbd is set where the marked run BEGINS and never again (the run's
    last pixel is unmarked): the island is skipped on the value cached at that statement alone.
    (With one-pixel walls, as in rings_across_step, the end of the run caches it again.)"""
    g = np.zeros((1, 18, 300), np.uint8)
    g[0, 1:17, 240:291] = 1
    g[0, 4:14, 243:288] = 0
    g[0, 8:10, 258:262] = 1
    return g


def mouth_islands(right):
    """A thick C open to the right (wall at x 200..203) or to the left (wall at x 276..279) with an
    isolated pixel and a 2 x 4 block in its mouth: both are external and must be found."""
    g = np.zeros((1, 30, 300), np.uint8)
    g[0, 2:5, 200:280] = 1
    g[0, 25:28, 200:280] = 1
    if right:
        g[0, 2:28, 200:204] = 1
    else:
        g[0, 2:28, 276:280] = 1
    g[0, 14, 260] = 1
    g[0, 10:12, 254:258] = 1
    return g


STEP_EDGE_W = 600
STEP_EDGE_X = [253, 509, 254, 510, 255, 511, 256, 512, 257, 513, STEP_EDGE_W - 1]


def step_edge_pixels():
    """Row k holds one run starting at STEP_EDGE_X[k] (neighbouring rows far apart), of 1 pixel for
    even k and 2 for odd k; row 11 holds two isolated pixels right of x = 256.  Layer 1 has the
    same behind a one-pixel column at x = 100, which the first row's trace marks on every row."""
    g = np.zeros((2, 12, STEP_EDGE_W), np.uint8)
    for k, x in enumerate(STEP_EDGE_X):
        g[:, k, x:min(x + 1 + k % 2, STEP_EDGE_W)] = 1
    g[:, 11, 300] = 1
    g[:, 11, 400] = 1
    g[1, :, 100] = 1
    return g


ROW_FLAG_ROWS = [62, 63, 64, 65, 127, 128, 130]


def row_flag_steps():
    """Content only on rows 62..65, 127, 128 and 130 (padded rows 63, 64 | 65, 66 and 128 | 129,
    131): separate bars, one or two per row, so that every row has a start of its own."""
    g = np.zeros((1, 131, 40), np.uint8)
    for k, y in enumerate(ROW_FLAG_ROWS[:-1]):
        x = 2 + 12 * (k % 3)
        g[0, y, x:x + 4] = 1
        if k % 2:
            g[0, y, 38:40] = 1
    g[0, 130] = 1
    return g


LDS_SHAPES = [(157, 1022), (158, 1022)]   # (H, W): 162976 <= LDS_MAX < 164000 bytes


def lds_limit(H, W):
    """The step scenes repeated at x offsets 0, 256 and 512 (the rings, the two mouths; their
    content lies in x 200..299, so the copies do not meet) and step_edge_pixels' second layer at
    offsets 0 and 256, a pixel at x = W - 1, the thick ring at the three offsets and pixels in the
    last row's corners; layer 1 is layer 0 flipped vertically."""
    a = np.zeros((H, W), np.uint8)
    y = 0
    for sc in (rings_across_step()[0], mouth_islands(True)[0], mouth_islands(False)[0]):
        h, w = sc.shape
        for off in (0, 256, 512):
            a[y:y + h, off:off + w] |= sc
        y += h + 2
    st = step_edge_pixels()[1]
    for off in (0, 256):
        a[y:y + 12, off:off + STEP_EDGE_W] |= st
        y += 14
    a[y + 2, W - 1] = 1
    sc = thick_ring_across_step()[0]
    for off in (0, 256, 512):
        a[138:138 + sc.shape[0], off:off + sc.shape[1]] |= sc
    a[H - 1, 0] = 1
    a[H - 1, W - 1] = 1
    return np.stack([a, a[::-1]])


# ---- layers -----------------------------------------------------------------------------------------
def zigzag_layers():
    """Six 5-pixel bars per layer on row 1, at x = 6k on even layers and x = 6k + 3 on odd ones:
    one chain through all layers, which the reference's single up and single down pass do not
    close."""
    g = np.zeros((6, 4, 40), np.uint8)
    for z in range(6):
        for k in range(6):
            x = 6 * k + 3 * (z % 2)
            g[z, 1, x:x + 5] = 1
    return g


def wide_merge():
    """Layers 0 and 2: isolated cells at even x and y (1089 components each); layer 1: 3-pixel bars
    on the even rows at x = 4m .. 4m + 2, each bridging two neighbouring cells of the outer
    layers (the cells of column 64 stay alone)."""
    g = np.zeros((3, 66, 66), np.uint8)
    g[0, 0::2, 0::2] = 1
    g[2, 0::2, 0::2] = 1
    for m in range(16):
        g[1, 0::2, 4 * m:4 * m + 3] = 1
    return g


def many_layers():
    """300 layers of 5 x 6: z % 3 == 0 empty, z % 7 == 3 full (an empty background label), the
    others a pixel and a 3-pixel bar whose places depend on z."""
    g = np.zeros((300, 5, 6), np.uint8)
    for z in range(300):
        if z % 7 == 3:
            g[z] = 1
        elif z % 3:
            g[z, z % 5, z % 6] = 1
            g[z, (z + 2) % 5, (z % 4):(z % 4) + 3] = 1
    return g


def cell_values():
    """Shapes drawn with the values 127, 128, 200 and 255 (as int8: 127, -128, -56, -1; the scan's
    marks are 2 and -126), touching each other: one component whatever the values."""
    g = np.zeros((2, 9, 20), np.uint8)
    _ring(g[0], 1, 7, 1, 9, 128)
    g[0, 4, 4:7] = 255          # island in the ring's hole
    g[0, 1, 10:15] = 127        # bar continuing the ring's top side
    g[0, 5, 16] = 200
    g[0, 6, 17] = 2
    g[0, 8, 19] = 130           # (-126 as int8)
    g[1, 2:7, 3:12] = 200
    g[1, 3:6, 5:10] = 255
    g[1, 4, 7] = 0
    g[1, 0, 0] = 128
    g[1, 8, 12:20] = 127
    g[1, 7, 19] = 254
    return g


def label_limit(cleared):
    """A (1, 512, 512) layer with cells at even x and y: 65536 components, or 65535 with one cell
    (of the middle) cleared."""
    g = np.zeros((1, 512, 512), np.uint8)
    g[0, 0::2, 0::2] = 1
    if cleared:
        g[0, 256, 300] = 0
    return g


BUILDERS = {
    "tile_diagonals": tile_diagonals,
    "tile_corner_antidiagonals": tile_corner_antidiagonals,
    "tile_near_misses": tile_near_misses,
    "serpentine": serpentine,
    "combs": combs,
    "interlocked_combs": interlocked_combs,
    **{f"every_block_a_root_{H}x{W}": (lambda H=H, W=W: every_block_a_root(H, W))
       for H, W in ROOT_SHAPES},
    **{f"wave_bars_{W}": (lambda W=W: wave_bars(W)) for W in BAR_WIDTHS},
    "rings_across_step": rings_across_step,
    "thick_ring_across_step": thick_ring_across_step,
    "mouth_islands_right": lambda: mouth_islands(True),
    "mouth_islands_left": lambda: mouth_islands(False),
    "step_edge_pixels": step_edge_pixels,
    "row_flag_steps": row_flag_steps,
    **{f"lds_limit_{H}": (lambda H=H, W=W: lds_limit(H, W)) for H, W in LDS_SHAPES},
    "zigzag_layers": zigzag_layers,
    "wide_merge": wide_merge,
    "many_layers": many_layers,
    "cell_values": cell_values,
}
NAMES = list(BUILDERS)
ROOT_NAMES = [f"every_block_a_root_{H}x{W}" for H, W in ROOT_SHAPES]
BAR_NAMES = [f"wave_bars_{W}" for W in BAR_WIDTHS]
SCAN_NAMES = ["rings_across_step", "thick_ring_across_step", "mouth_islands_right", "mouth_islands_left", "step_edge_pixels",
              "row_flag_steps", "lds_limit_157", "lds_limit_158"]

_built, _oracle = {}, {}


def get(name):
    """A scene's grid by name, built on first use (read-only)."""
    if name not in _built:
        g = np.ascontiguousarray(BUILDERS[name](), np.uint8)
        g.setflags(write=False)
        _built[name] = g
    return _built[name]


def oracle(name):
    """The C oracle's result of a scene, computed once and shared by the tests."""
    if name not in _oracle:
        import oracle as oracle_mod
        _oracle[name] = oracle_mod.object_segmentation_front(get(name))
    return _oracle[name]
