"""Built inputs for the segmented partition and the segmented voxel table, aimed at
the kernels' edges: segment borders at lane, wave and tile offsets, empty segments, starts that
decrease or pass the capacity, the pass-count switches of the composite key, and equal cells on the
two sides of a border.  Every scene carries the property it was built for (`holds`), which
tests/test_object_segments_ref.py checks on the CPU."""
import numpy as np

NONE = 0xFFFFFFFF
TILE = 2048                      # kOpTile of csrc/gdf_object_points.hpp
ROW = 2048                       # cells per counted bitmap row (csrc/gdf_voxel_table.hpp)
SCAN_ONE = 8192                  # rows the scan takes in one launch
MAX_GROUPS = 1 << 24             # kOpMaxObjects
MAX_CELLS = 1 << 28              # kVtMaxCells
BORDERS = (1, 63, 64, 65, 511, 512, 513, TILE - 1, TILE, TILE + 1)


def odd_points(rng, n):
    """n float4 rows of distinct bit patterns, with NaN payloads, -0.0 and a denormal."""
    p = rng.integers(0, 2**32, (n, 4), dtype=np.uint64).astype(np.uint32)
    p[:, 3] = (np.arange(n, dtype=np.uint64) * 2654435761 % 2**32).astype(np.uint32)
    if n:
        p[0::5, 0] = 0x80000000
        p[1::5, 1] = 0x7FC00123
        p[2::5, 2] = 0xFF800001
        p[3::5, 0] = 0x00000001
    return p.view(np.float32)


def u32(a):
    return np.asarray(a, np.uint64).astype(np.uint32)


def partition_scenes() -> dict:
    """name -> dict(ids, starts, nobj, keep or None, holds)"""
    rng = np.random.default_rng(15)
    out = {}

    def add(name, ids, starts, nobj, keep=None, holds=lambda s: True):
        out[name] = dict(ids=u32(ids), starts=u32(starts), nobj=int(nobj),
                         keep=None if keep is None else np.asarray(keep, np.uint8), holds=holds)

    for b in BORDERS:   # one border at a lane / wave / tile offset, the same ids on both sides of it
        n = b + 70
        ids = rng.integers(0, 3, n)
        ids[b - 1] = ids[b] = 1
        add(f"border {b}", ids, [0, b, n], 3,
            holds=lambda s, b=b: s["starts"][1] == b and s["ids"][b - 1] == s["ids"][b])
    n = BORDERS[-1] + 251
    add("every border", rng.integers(0, 5, n), [0, *BORDERS, n], 5,
        holds=lambda s: len(s["starts"]) == len(BORDERS) + 2)
    n = 300
    ids = rng.integers(0, 4, n)
    for name, starts in (("empty first", [0, 0, 0, 100, 200, n]), ("empty middle", [0, 100, 100, 100, 200, n]),
                         ("empty last", [0, 100, 200, n, n, n]), ("all but one empty", [0, 0, 0, n, n, n]),
                         ("all empty", [7, 7, 7, 7, 7, 7])):
        add(name, ids, starts, 4, holds=lambda s: (np.diff(s["starts"].astype(np.int64)) == 0).sum() >= 2)
    for nseg in (1, 2, 16, 64):
        n = 1000
        cuts = np.sort(rng.integers(0, n + 1, nseg - 1))
        add(f"nseg {nseg}", rng.integers(0, 7, n), [0, *cuts, n], 7,
            holds=lambda s, nseg=nseg: len(s["starts"]) == nseg + 1)
    n = 500
    ids = rng.integers(0, 6, n)
    add("starts decrease", ids, [0, 200, 100, 300, 250, n], 6,
        holds=lambda s: (np.diff(s["starts"].astype(np.int64)) < 0).any())
    add("starts pass the capacity", ids, [0, 200, n + 1, 1 << 31, NONE], 6,
        holds=lambda s: (s["starts"].astype(np.int64) > len(s["ids"])).sum() >= 3)
    add("rows before the first segment", ids, [70, 200, 333, n - 20], 6,
        holds=lambda s: s["starts"][0] > 0 and s["starts"][-1] < len(s["ids"]))
    # the pass-count switches of the composite key: 1 | 2 passes at 256 groups, 2 | 3 at 65 536
    for nseg, nobj in ((2, 128), (1, 257), (64, 1024), (1, 65537), (64, MAX_GROUPS // 64)):
        n = 40
        ids = rng.integers(0, nobj, n)
        ids[::7] = nobj - 1                               # the last group of a segment
        cuts = np.sort(rng.integers(0, n + 1, nseg - 1))
        cuts = np.minimum(cuts, n - 1)                    # (the last segment is not empty)
        add(f"groups {nseg} x {nobj}", ids, [0, *cuts, n], nobj,
            holds=lambda s, g=nseg * nobj: (len(s["starts"]) - 1) * s["nobj"] == g)
    n = 400
    ids = rng.integers(0, 5, n)
    keep = np.array([1, 1, 0, 1, 1], np.uint8)
    add("keep drops an object", ids, [0, 100, 250, n], 5, keep, holds=lambda s: (s["ids"] == 2).any())
    seg_ids = ids.copy()
    seg_ids[100:250] = 2
    add("keep drops a segment", seg_ids, [0, 100, 250, n], 5, keep,
        holds=lambda s: (s["ids"][100:250] == 2).all() and s["keep"][2] == 0)
    add("every row dropped", ids, [0, 100, 250, n], 5, np.zeros(5, np.uint8),
        holds=lambda s: not s["keep"].any())
    one = ids.copy()
    one[100:250] = 3
    add("one object holds a segment", one, [0, 100, 250, n], 5, holds=lambda s: (s["ids"][100:250] == 3).all())
    none = ids.copy()
    none[::3] = NONE
    none[99:102] = NONE
    add("ids of NONE", none, [0, 100, 250, n], 5, holds=lambda s: (s["ids"][99:102] == NONE).all())
    over = ids.copy()
    over[1::4] = rng.choice(np.array([5, 6, 1 << 24, 1 << 31, NONE - 1], np.uint64), len(over[1::4]))
    over[248:252] = 5
    add("ids at and above nobj", over, [0, 100, 250, n], 5, holds=lambda s: (s["ids"][248:252] == 5).all())
    return out


PARTITION_REFUSALS = ((1, MAX_GROUPS + 1), (64, MAX_GROUPS // 64 + 1), (0, 5), (65, 5), (3, 0))


def table_scenes() -> dict:
    """name -> dict(cells, starts, C, holds)"""
    rng = np.random.default_rng(16)
    out = {}

    def add(name, cells, starts, C, holds=lambda s: True):
        out[name] = dict(cells=u32(cells), starts=u32(starts), C=int(C), holds=holds)

    # the same cell on both sides of a border: inside a wave (so the two rows are adjacent lanes, which
    # §14's lane dedup would merge), at a wave edge and at a tile edge
    for b in (37, 64, 100, 256, 257, TILE, TILE + 1):
        n, C = b + 90, 5000
        cells = rng.integers(0, C, n)
        cells[b - 3:b + 3] = 1234
        add(f"same cell across border {b}", cells, [0, b, n], C,
            holds=lambda s, b=b: s["cells"][b - 1] == s["cells"][b] and s["starts"][1] == b and
            (b % 64 != 0) == (b in (37, 100, 257, TILE + 1)))
    n, C = 400, 777
    cells = rng.integers(0, C, n)
    cells[100:300] = 55
    add("a run over three segments", cells, [0, 150, 200, n], C, holds=lambda s: (s["cells"][100:300] == 55).all())
    cells = rng.integers(0, C, n)
    cells[148:152] = [C, C + 1, NONE, C]
    cells[199:201] = [1 << 31, C]
    add("outside cells at the borders", cells, [0, 150, 200, n], C,
        holds=lambda s: (s["cells"][[149, 150, 199, 200]] >= s["C"]).all())
    add("all outside", np.full(n, C, np.uint32), [0, 150, 200, n], C)
    for C in (1, 31, 32, 33, 2049):      # s * C is no multiple of 32: segments share bitmap words
        n = 700
        cells = rng.integers(0, C + 1, n)                 # (C itself: outside)
        cells[:3] = [0, C - 1, 0]
        cells[-3:] = [C - 1, 0, C - 1]
        cuts = np.sort(rng.integers(0, n + 1, 6))
        add(f"C {C}", cells, [0, *cuts, n], C, holds=lambda s: len(s["starts"]) == 8)
        every = np.resize(np.arange(C), max(n, 3 * C))    # every cell in every segment
        m = len(every)
        add(f"every cell, C {C}", every, [0, m // 3, 2 * (m // 3), m], C,
            holds=lambda s: s["starts"][1] >= s["C"])
    for nseg in (1, 2, 16, 64):
        n, C = 1500, 300
        cuts = np.sort(rng.integers(0, n + 1, nseg - 1))
        add(f"nseg {nseg}", rng.integers(0, C, n), [0, *cuts, n], C,
            holds=lambda s, nseg=nseg: len(s["starts"]) == nseg + 1)
    n, C = 600, 300
    cells = np.repeat(rng.integers(0, C, n // 4), 4)
    for name, starts in (("empty first", [0, 0, 0, 100, 200, n]), ("empty middle", [0, 100, 100, 100, 200, n]),
                         ("empty last", [0, 100, 200, n, n, n]), ("all but one empty", [0, 0, 0, n, n, n]),
                         ("starts decrease", [0, 200, 100, 300, 250, n]),
                         ("starts pass the capacity", [0, 200, n + 1, 1 << 31, NONE]),
                         ("rows before the first segment", [70, 200, 333, n - 20])):
        add(name, cells, starts, C)
    # the bound: nseg * C = 2^28, cells in the first and the last word of the composite bitmap
    C = MAX_CELLS // 64
    n = 64 * 5
    cells = rng.integers(0, C, n)
    cells[:2] = [0, C - 1]
    cells[-2:] = [0, C - 1]
    add("2^28 composite cells", cells, np.arange(65) * 5, C, holds=lambda s: 64 * s["C"] == MAX_CELLS)
    # §14's scan switch, reached through nseg * C: 8192 counted rows in one launch, 8193 in three
    for C in (SCAN_ONE * ROW // 2, SCAN_ONE * ROW // 2 + 1):
        n = 3000
        cells = np.concatenate([rng.integers(0, ROW, 300), rng.integers(C - ROW, C, 300),
                                rng.integers(0, C, n - 604), [0, C - 1, C, C + 1]])
        rng.shuffle(cells)
        add(f"scan switch, C {C}", cells, [0, 1400, n], C,
            holds=lambda s: (-(-2 * s["C"] // ROW) <= SCAN_ONE) == (2 * s["C"] == SCAN_ONE * ROW))
    return out


TABLE_REFUSALS = ((64, MAX_CELLS // 64 + 1), (1, MAX_CELLS + 1), (2, 0), (0, 100), (65, 100))
