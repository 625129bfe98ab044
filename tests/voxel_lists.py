"""Named (point, key) lists for the voxelize stage - TEST INFRASTRUCTURE.

The voxelize stage sorts voxel keys (k_sort_pass) and sums every voxel's points in list order
(k_group over sorted points, k_group_runs / k_group_runs_big over sorted runs of equal keys,
k_xruns_count / k_xruns_emit cutting a received list into runs).  Camera frames reach the
routing thresholds of those kernels only by luck; the scenes here are built to sit on them.

A scene is a description - groups (key, run lengths) in key order, plus an arrangement of the
runs in the input list - from which build() makes the keys, the points and the run decomposition
of the list.  "Item" below is a point where points are sorted (GDF_NO_XRUNS) and a run where runs
are sorted; both group kernels tile 256 sorted items, so scenes built from runs of ONE point are
the same tile geometry for both.  In such a scene no two neighbours of the input list share a key
(arrange() sees to it), so the runs the engine cuts from the list are the described ones.

census() restates the routing of k_group and of k_group_runs on the sorted list, as events
("kg.len=small", "kgr.extra=65", ...); tests/test_voxel_lists.py asserts that every scene holds
the events it is named for and that the scenes together reach every route on both sides of every
threshold.  The constants below restate the kernels'; the same test reads them out of the source.
"""
import heapq
import zlib
from dataclasses import dataclass, field, replace

import numpy as np

from voxel_ref import runs_of, voxelize_ref

# gdf_device.hpp / gdf_kernels.hip
kGroupThreads = 256   # sorted items per tile of k_group / k_group_runs
kStagePts = 512       # k_group: staged positions from the tile's first group start
kGatherChunk = 256    # k_group: points per gathered chunk of a wave
kExtraRuns = 64       # k_group_runs: run records read past the tile for its last group
kHugeGroup = 32768    # k_group_runs: queued groups of >= this many points go to the huge region
kHugeRuns = 2048      # ... or of >= this many runs
kRunPasses = 4        # k_group_runs<., 2>: staging windows per tile
kXRunTile = 4096      # k_xruns_count / k_xruns_emit: keys per tile
kSortThreads = 256    # k_sort_pass: a tile is kSortThreads * PT keys
kSortGroup = 8        # k_sort_pass: tiles per look-back group
kLookGranule = 64     # lookback2_wave / kScanGroup: tiles per granule of the group look-back


@dataclass(frozen=True)
class Knobs:
    """The Tuning values that decide a route (gdf_device.hpp Tuning's defaults)."""
    small_group: int = 32
    run_stage: int = 2048
    run_inblock: int = 1024
    group_scan_tiles: int = 1024
    run_wave: int = 2

    @property
    def stage(self):  # launch_voxelize: k_group_runs<2048, .> or <512, .>
        return 2048 if self.run_stage >= 2048 else 512

    @property
    def inblock(self):  # launch_voxelize's min(); WAVE 0 queues everything above small_group
        m = min(self.run_inblock, self.stage)
        return min(m, self.small_group) if self.run_wave == 0 else m


DEFAULT = Knobs()

# voxel grids (lower, upper, cell size) by the key width they give (gdf_engine.cpp set_grid:
# key_bits = bits of cells - 1); the cell sizes are no powers of two, so a corner's product rounds
GRIDS = {
    8: ((-1.0, -1.0, 0.0), (0.6, 0.5, 0.12), (0.1, 0.1, 0.12)),        # 16 x 15 x 1
    9: ((-1.0, -1.0, 0.0), (1.5, 1.0, 0.12), (0.1, 0.1, 0.12)),        # 25 x 20 x 1
    16: ((-10.0, -10.0, 0.0), (20.0, 10.0, 0.12), (0.1, 0.1, 0.12)),   # 300 x 200 x 1
    17: ((-10.0, -20.0, 0.0), (30.0, 10.0, 0.12), (0.1, 0.1, 0.12)),   # 400 x 300 x 1
    22: ((-10.0, -20.0, -1.0), (30.0, 20.0, 1.5), (0.1, 0.1, 0.12)),   # 400 x 400 x 21 (default)
    25: ((-10.0, -20.0, -1.0), (30.0, 20.0, 23.0), (0.1, 0.1, 0.12)),  # 400 x 400 x 200
    26: ((-10.0, -20.0, -1.0), (40.0, 30.0, 29.0), (0.1, 0.1, 0.12)),  # 500 x 500 x 250: 64 MiB u8
}

# knob sets of the GPU test: name -> (environment, Knobs for the census)
KNOB_SETS = {
    "scan2": ({"GDF_GROUP_SCAN_TILES": "2"}, replace(DEFAULT, group_scan_tiles=2)),
    "scan2_noscan": ({"GDF_GROUP_SCAN_TILES": "2", "GDF_NO_GROUP_SCAN": "1"},
                     replace(DEFAULT, group_scan_tiles=2)),
    "scan2_nofirst": ({"GDF_GROUP_SCAN_TILES": "2", "GDF_GROUP_FIRST": "0"},
                      replace(DEFAULT, group_scan_tiles=2)),
    "scan2_noscan_nofirst": ({"GDF_GROUP_SCAN_TILES": "2", "GDF_NO_GROUP_SCAN": "1",
                              "GDF_GROUP_FIRST": "0"}, replace(DEFAULT, group_scan_tiles=2)),
    "blocks2": ({"GDF_SORT_BLOCKS": "2", "GDF_GROUP_BLOCKS": "2"}, DEFAULT),
    "pt4": ({"GDF_SORT_PT": "4"}, DEFAULT),
    "pt8": ({"GDF_SORT_PT": "8"}, DEFAULT),
    "pt16": ({"GDF_SORT_PT": "16"}, DEFAULT),
    "wave0": ({"GDF_RUN_WAVE": "0"}, replace(DEFAULT, run_wave=0)),
    "wave1": ({"GDF_RUN_WAVE": "1"}, replace(DEFAULT, run_wave=1)),
    "wave2": ({"GDF_RUN_WAVE": "2"}, DEFAULT),
    "stage512": ({"GDF_RUN_STAGE": "512"}, replace(DEFAULT, run_stage=512)),
    "inblock512": ({"GDF_RUN_INBLOCK": "512"}, replace(DEFAULT, run_inblock=512)),
    "small1": ({"GDF_SMALL_GROUP": "1"}, replace(DEFAULT, small_group=1)),
    "small64": ({"GDF_SMALL_GROUP": "64"}, replace(DEFAULT, small_group=64)),
    "wavemode0": ({"GDF_RUN_WAVE_MODE": "0"}, DEFAULT),
    "wavemode1": ({"GDF_RUN_WAVE_MODE": "1"}, DEFAULT),
    "wavemode2": ({"GDF_RUN_WAVE_MODE": "2"}, DEFAULT),
    "q16_0": ({"GDF_RUN_Q16": "0"}, DEFAULT),
    "q16_1": ({"GDF_RUN_Q16": "1"}, DEFAULT),
    "bigblocks1": ({"GDF_RUN_BIG_BLOCKS": "1"}, DEFAULT),
}
KNOB_FAMILIES = ("ladder", "tile_edge", "staged", "runs_per_group", "long_run", "windows")

# Events that a knob set moves away from the scenes named for them (the knob changes that very
# threshold): under that knob set the census assertion for these events is waived - the pairing
# still runs on the GPU and is compared.  tests/test_voxel_lists.py asserts that the list is
# exact: every other needed event still holds under every knob set, and every event listed here
# is in fact lost by a scene that needs it.
_SCAN2 = {"kg.gather.len%chunk=0", "kg.gather.len%chunk=1", "kg.route.gather"}  # queued instead
OFF_EDGE = {
    "scan2": _SCAN2, "scan2_noscan": _SCAN2, "scan2_nofirst": _SCAN2, "scan2_noscan_nofirst": _SCAN2,
    # WAVE 0 / 1 stage one window; WAVE 0's in-block limit is small_group
    "wave0": {"kgr.pts=inblock", "kgr.pts=inblock+1", "kgr.windows=4", "kgr.queue.windows",
              "kgr.short_next_window"},
    "wave1": {"kgr.windows=4", "kgr.queue.windows", "kgr.short_next_window"},
    # the in-block limit is min(run_inblock, stage) = 512, below the scenes' 1024 / 2048; a tile
    # whose first group is past the limit and longer than the stage gets no window at all
    "stage512": {"kgr.pts=inblock", "kgr.pts=inblock+1", "kgr.pts=stage", "kgr.pts=stage+1",
                 "kgr.windows=4", "kgr.short_next_window"},
    "inblock512": {"kgr.pts=inblock", "kgr.pts=inblock+1", "kgr.windows=4"},
    "small1": {"kg.len=small+1", "kgr.pts=small+1"},
    "small64": {"kg.len=small", "kg.len=small+1", "kgr.pts=small", "kgr.pts=small+1"},
}


def on_edge_needs(scene, knob_name):
    """The scene's needed events that must still hold under the knob set."""
    return {e for e in scene.needs if e not in OFF_EDGE.get(knob_name, ())}


# ---- point values ---------------------------------------------------------------------------------
def point_values(rng, n):
    """(n, 4) float32, each component sign * U(1, 2) * 2^k with k an integer in [-6, 6]: the f32
    chain over such terms depends on their order, so a summer that takes a group's points in
    another order, skips one or takes one twice changes the result's bits."""
    m = rng.uniform(1.0, 2.0, (n, 4))
    k = rng.integers(-6, 7, (n, 4))
    s = rng.integers(0, 2, (n, 4)) * 2 - 1
    return (s * m * np.exp2(k)).astype(np.float32)


def reversal_changes(keys, pts):
    """(changed, of): among the groups of >= 8 points, how many change the reference's bits when
    the points inside every group are reversed."""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    lead = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if len(sk) else order
    size = np.diff(np.concatenate([lead, [len(sk)]]))
    if not (size >= 8).any():
        return 0, 0
    rev = pts.copy()
    for a, n in zip(lead[size > 1], size[size > 1]):
        rev[order[a:a + n]] = pts[order[a:a + n][::-1]]
    r0, r1 = voxelize_ref(keys, pts)[1], voxelize_ref(keys, rev)[1]
    ch = (r0.view(np.uint32) != r1.view(np.uint32)).any(axis=1)[size >= 8]
    return int(ch.sum()), len(ch)


def _seed(name):
    return zlib.crc32(name.encode())


# ---- arrangement ----------------------------------------------------------------------------------
def arrange(nruns_by_group, rng):
    """An order of all runs (group ids, each group's runs in their own order) in which no two
    neighbours belong to one group: always a run of the group with the most runs left that is not
    the previous one's, ties in seeded random order.  Fails when a group has more runs than all
    others together plus one."""
    tie = rng.permutation(len(nruns_by_group))
    heap = [(-c, int(tie[g]), g) for g, c in enumerate(nruns_by_group) if c > 0]
    heapq.heapify(heap)
    out = np.empty(int(sum(nruns_by_group)), np.int64)
    held = None  # the previous run's group, kept out of the heap for one step
    for i in range(len(out)):
        if not heap:
            raise ValueError("arrange: a group has more runs than the others can separate")
        c, t, g = heapq.heappop(heap)
        out[i] = g
        if held is not None:
            heapq.heappush(heap, held)
        held = (c + 1, t, g) if c + 1 < 0 else None
    return out


# ---- scenes ---------------------------------------------------------------------------------------
@dataclass
class Scene:
    name: str
    family: str
    needs: frozenset = frozenset()      # census events the scene is named for (default knobs)
    lens: list = None                   # structure scenes: run lengths per group, in key order
    keyfn: object = None                # key-list scenes: (ncells, rng) -> keys of the list
    single_runs: bool = field(default=False)  # every described run holds one point

    def build(self, ncells):
        """{keys, pts, run_keys, run_starts, groups}: the input list, its maximal runs and the
        description [(key, [run lengths])] in key order, for a grid of ncells cells."""
        rng = np.random.default_rng(_seed(self.name))
        if self.keyfn is not None:
            keys = np.asarray(self.keyfn(ncells, rng), np.uint32)
            rk, rs = runs_of(keys)
        else:
            G = len(self.lens)
            if G > ncells:
                raise ValueError(f"{self.name}: {G} groups in {ncells} cells")
            step = max((ncells - 1) // max(G - 1, 1), 1)
            gkey = (np.arange(G, dtype=np.int64) * step).astype(np.uint32)
            order = arrange([len(r) for r in self.lens], rng)
            nth = np.zeros(G, np.int64)
            rlen = np.empty(len(order), np.int64)
            for i, g in enumerate(order):
                rlen[i] = self.lens[g][nth[g]]
                nth[g] += 1
            rk = gkey[order]
            rs = np.concatenate([[0], np.cumsum(rlen)]).astype(np.uint32)
            keys = np.repeat(rk, rlen)
            rk2, rs2 = runs_of(keys)  # (the arrangement keeps the described runs maximal)
            assert np.array_equal(rk, rk2) and np.array_equal(rs, rs2), self.name
        assert len(keys) == 0 or int(keys.max()) < ncells, self.name
        # (a scene with a handful of such groups can draw one that sums alike both ways: redrawn)
        for _ in range(16):
            pts = point_values(rng, len(keys))
            ch, of = reversal_changes(keys, pts)
            if ch >= 0.9 * of:
                break
        else:
            raise ValueError(f"{self.name}: point values not order sensitive")
        # the description in key order: a stable sort of the runs by key
        o = np.argsort(rk, kind="stable")
        sk, sl = rk[o], np.diff(rs.astype(np.int64))[o]
        groups = []
        if len(sk):
            lead = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
            for a, b in zip(lead, np.concatenate([lead[1:], [len(sk)]])):
                groups.append((int(sk[a]), sl[a:b].tolist()))
        return {"name": self.name, "keys": keys, "pts": pts, "run_keys": rk, "run_starts": rs,
                "groups": groups}


LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192,
           8193, 16383, 16384, 16385)
LADDER = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047,
          2048, 2049)
RUNS_PER_GROUP = (1, 2, 255, 256, 257, 320, 321, 2047, 2048)
LONG_RUNS = (1024, 1025, 2048, 2049, 32767, 32768)
ONE = [1]

# the thresholds a ladder length is aimed at, by (length, tile offset) or length alone
_LADDER_NEEDS = {
    32: {"kg.len=small", "kgr.pts=small"}, 33: {"kg.len=small+1", "kgr.pts=small+1"},
    (255, 0): {"tile.end=tile-1"}, (256, 0): {"tile.end=tile"}, (257, 0): {"tile.end=tile+1"},
    (2, 255): {"tile.end=tile+1"},
    (512, 0): {"kg.end=staged"}, (513, 0): {"kg.end=staged+1"}, (257, 255): {"kg.end=staged"},
    (511, 255): {"kg.route.gather"}, (512, 255): {"kg.gather.len%chunk=0"},
    (513, 255): {"kg.gather.len%chunk=1"}, (1024, 255): {"kg.gather.len%chunk=0"},
    (1025, 255): {"kg.gather.len%chunk=1"},
    1024: {"kgr.pts=inblock"}, 1025: {"kgr.pts=inblock+1"},
    2047: {"kgr.runs=huge-1"}, 2048: {"kgr.runs=huge", "kgr.pts=stage"}, 2049: {"kgr.pts=stage+1"},
}


def _digit_scenes():
    N = 2500  # three sort tiles at PT = 4, ten group tiles; no multiple of a tile

    def top_shift(ncells):  # the last radix pass's first bit (radix_passes, gdf_device.hpp)
        bits = max(int(ncells - 1).bit_length(), 1)
        passes = 1 if bits <= 9 else (bits + 6) // 8 if bits <= 25 else (bits + 7) // 8
        return 8 * (passes - 1)

    def equal(nc, rng):
        return np.full(N, nc // 3, np.uint32)

    def top_digit(nc, rng):
        sh = top_shift(nc)
        return (rng.integers(0, ((nc - 1) >> sh) + 1, N) << sh).astype(np.uint32)

    def high_half(nc, rng):  # key 256: bit 8, the high half of a 9-bit digit (8-bit grids: bit 7)
        return (rng.integers(0, 2, N) * (256 if nc > 256 else 128)).astype(np.uint32)

    def ends(nc, rng):
        return (rng.integers(0, 2, N) * (nc - 1)).astype(np.uint32)

    def descending(nc, rng):
        m = min(N, nc)
        return (nc - 1 - np.arange(m) * ((nc - 1) // max(m - 1, 1))).astype(np.uint32)

    def mod257(nc, rng):
        return (np.arange(N) % min(257, nc)).astype(np.uint32)

    def alternating(nc, rng):
        return np.where(np.arange(N) % 2 == 0, nc - 2, nc // 2).astype(np.uint32)

    def uniform(nc, rng):
        return rng.integers(0, nc, N).astype(np.uint32)

    fns = [("equal", equal), ("top_digit", top_digit), ("high_half", high_half), ("ends", ends),
           ("descending", descending), ("mod257", mod257), ("alternating", alternating),
           ("uniform", uniform)]
    return [Scene(f"digits_{nm}", "digits", keyfn=fn) for nm, fn in fns]


def _length_scenes():
    out = []
    for n in LENGTHS:
        out.append(Scene(f"len_{n}_range50", "lengths", frozenset({f"n={n}"}),
                         keyfn=lambda nc, rng, n=n: rng.integers(0, min(50, nc), n)))
        out.append(Scene(f"len_{n}_whole", "lengths", frozenset({f"n={n}"}),
                         keyfn=lambda nc, rng, n=n: rng.integers(0, nc, n)))
    return out


def _structure_scenes():
    S = []

    def add(name, family, lens, needs=(), single=False):
        S.append(Scene(name, family, frozenset(needs), lens=lens, single_runs=single))

    # the ladder: a group of L items (runs of one point) at tile offset 0 and at 255, singletons
    # around it (as many behind as keep its items apart in the input list)
    for L in LADDER:
        for off in (0, 255):
            needs = {f"g:{L}@{off}"} if L > 1 else {f"groups={off + 301}"}
            needs |= _LADDER_NEEDS.get(L, set()) | _LADDER_NEEDS.get((L, off), set())
            add(f"ladder_{L}_at{off}", "ladder", [ONE] * off + [ONE * L] + [ONE] * max(L, 300),
                needs, single=True)
    # tile edges
    for d, ev in ((155, "tile.end=tile-1"), (156, "tile.end=tile"), (157, "tile.end=tile+1")):
        add(f"edge_group_ends_{ev[9:]}", "tile_edge", [ONE] * 100 + [ONE * d] + [ONE] * 300,
            {ev, f"g:{d}@100"}, single=True)
    add("edge_last_group_at_multiple", "tile_edge", [ONE] * 472 + [ONE * 40],
        {"n=512", "last.end=tile"}, single=True)
    add("edge_last_group_past_multiple", "tile_edge", [ONE] * 472 + [ONE * 41],
        {"n=513", "last.end=tile+1"}, single=True)
    add("edge_three_tiles_no_start", "tile_edge", [ONE] * 100 + [ONE * 1000] + [ONE] * 1200,
        {"tile.nostart>=3", "g:1000@100"}, single=True)
    for n in (1, 256, 257, 70000):  # the whole list one group (one run: its points are adjacent)
        add(f"edge_one_group_{n}", "tile_edge", [[n]], {f"n={n}", "groups=1"})
    # staged window of k_group: tile 1's first group start at offset 200 (S0 = 456); its last
    # group ends at S0 + 512 / S0 + 513
    for d, ev in ((468, "kg.end=staged"), (469, "kg.end=staged+1")):
        add(f"staged_first_at_200_{ev[7:]}", "staged",
            [ONE * 456, ONE * 10] + [ONE] * 34 + [ONE * d] + [ONE] * 1000,
            {"tile.first_at=200", ev, f"g:{d}@244"}, single=True)
    # a long group first, short groups behind it past the staged positions of k_group_runs (they
    # take the next window, or the queue under GDF_RUN_WAVE 0 / 1).  k_group has no such case: a
    # tile's 256 items end within 512 positions of its first group start (census: never seen).
    add("staged_short_past_stage", "staged", [[1000, 1000]] + [[30]] * 60 + [ONE] * 300,
        {"kgr.short_next_window", "kgr.pts=inblock+"})
    # runs per group: a group of R runs at tile offset 0, a partner of R runs to keep its runs
    # apart in the input list, singletons behind
    for rl in (1, 16):
        for R in RUNS_PER_GROUP:
            needs = {f"gr:{R}@0"} if R > 1 else {"groups=302"}
            needs |= {320: {"kgr.extra=64"}, 321: {"kgr.extra=65"}, 2047: {"kgr.runs=huge-1"},
                      2048: {"kgr.runs=huge"}}.get(R, set())
            add(f"runs_{R}_of_{rl}", "runs_per_group", [[rl] * R, [rl] * R] + [ONE] * 300, needs,
                single=rl == 1)
    # single long runs
    for n in LONG_RUNS:
        needs = {1024: {"kgr.pts=inblock"}, 1025: {"kgr.pts=inblock+1"}, 2048: {"kgr.pts=stage"},
                 2049: {"kgr.pts=stage+1"}, 32767: {"kgr.pts=huge-1"}, 32768: {"kgr.pts=huge"}}[n]
        add(f"long_run_{n}", "long_run", [ONE] * 5 + [[n]] + [ONE] * 300, needs | {f"gp:{n}@5"})
    # staging windows of k_group_runs
    add("windows_256_groups_of_40", "windows", [[40]] * 256 + [ONE] * 300,
        {"kgr.windows=4", "kgr.queue.windows"})
    add("windows_8_groups_of_1024", "windows", [[1024]] * 8 + [ONE] * 548,
        {"kgr.windows=4", "kgr.pts=inblock"})
    # size estimate of a group continuing past the tile's records
    add("estimate_low_huge_by_runs", "estimate",
        [ONE] * 246 + [[1] * 10 + [20] * 2100, [1] * 2110] + [ONE] * 300, {"kgr.huge.est_low"})
    add("estimate_high_short_beyond", "estimate",
        [ONE] * 246 + [[400] * 10 + [1] * 100, [1] * 110] + [ONE] * 300, {"kgr.huge.est_only"})
    # more than group_scan_tiles tiles of capacity at the default knobs: k_group_count, tile
    # offsets, k_group_big's queue and the tile_first search without a knob
    add("big_default_scan", "big",
        [[3000], [2] * 700] + [[6, 6]] * 22000 + [[40]] * 300,
        {"kg.scan", "kg.route.queue", "kgr.scan"})
    return S


def scenes():
    return _length_scenes() + _digit_scenes() + _structure_scenes()


# ---- census ---------------------------------------------------------------------------------------
def _starts(sk):
    n = len(sk)
    lead = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if n else np.zeros(0, np.int64)
    return lead.astype(np.int64), np.concatenate([lead[1:], [n]]).astype(np.int64) if n else lead


def _tile_census(s, e, n, ev, prefix_items):
    """Events of the tile geometry shared by both kernels (s, e: group borders in items)."""
    T = kGroupThreads
    ntiles = (n + T - 1) // T
    per_tile = np.bincount(s // T, minlength=ntiles) if ntiles else np.zeros(0, np.int64)
    ev.add(f"n={n}")
    ev.add(f"groups={len(s)}")
    run, best = 0, 0
    for c in per_tile:
        run = run + 1 if c == 0 else 0
        best = max(best, run)
    if best >= 1:
        ev.add("tile.nostart")
    if best >= 3:
        ev.add("tile.nostart>=3")
    first = np.full(ntiles, -1, np.int64)
    first[(s // T)[::-1]] = (s % T)[::-1]
    if (first[1:] == 200).any():
        ev.add("tile.first_at=200")
    big = e - s > 1  # (singletons end everywhere)
    for d, nm in ((0, "tile.end=tile"), (T - 1, "tile.end=tile-1"), (1, "tile.end=tile+1")):
        if (big & (e % T == d) & (e < n)).any():
            ev.add(nm)
    if len(s) and e[-1] - s[-1] > 1:
        if n % T == 0:
            ev.add("last.end=tile")
        if n % T == 1:
            ev.add("last.end=tile+1")
    for L, o in zip((e - s)[big].tolist(), (s % T)[big].tolist()):
        ev.add(f"{prefix_items}:{L}@{o}")
    return per_tile


def census_points(sorted_keys, knobs=DEFAULT):
    """k_group on sorted point keys: per tile the group starts, per group its length, tile offset,
    whether it crosses the tile, and its route; the events."""
    sk = np.asarray(sorted_keys)
    n = len(sk)
    ev = set()
    s, e = _starts(sk)
    per_tile = _tile_census(s, e, n, ev, "g")
    T = kGroupThreads
    queue_on = (max(n, 1) + T - 1) // T > knobs.group_scan_tiles  # tile offsets: bigq in use
    ev.add("kg.scan" if queue_on else "kg.lookback")
    tile = s // T
    S0 = s[np.searchsorted(s, tile * T)] if len(s) else s  # the tile's first group start
    staged = np.minimum(n - S0, kStagePts)
    L = e - s
    inside = e - S0 <= staged
    small = L <= knobs.small_group
    route = np.where(inside & small, "thread",
                     np.where(~inside & queue_on, "queue", np.where(inside, "stretch", "gather")))
    for r in np.unique(route):
        ev.add(f"kg.route.{r}")
    full = staged == kStagePts
    for cond, nm in ((inside & (L == knobs.small_group), "kg.len=small"),
                     (inside & (L == knobs.small_group + 1), "kg.len=small+1"),
                     (full & (e - S0 == kStagePts), "kg.end=staged"),
                     (e - S0 == kStagePts + 1, "kg.end=staged+1"),
                     (~inside & small, "kg.short_past_stage"),
                     ((route == "gather") & (L % kGatherChunk == 0), "kg.gather.len%chunk=0"),
                     ((route == "gather") & (L % kGatherChunk == 1), "kg.gather.len%chunk=1")):
        if cond.any():
            ev.add(nm)
    return {"events": ev, "tile_starts": per_tile, "start": s, "items": L, "points": L,
            "offset": s % T, "crosses": e > (tile + 1) * T, "extra": np.zeros_like(L),
            "route": route}


def census_runs(sorted_run_keys, sorted_run_lens, knobs=DEFAULT, npoints=None):
    """k_group_runs<stage, WAVE> on sorted runs: per tile the group starts, per group its runs,
    points, tile offset, whether it crosses the tile, the run records past the tile it needs, its
    route (thread / lanes / wave / queue.<reason>, + .huge) and window; the events."""
    sk = np.asarray(sorted_run_keys)
    rl = np.asarray(sorted_run_lens, np.int64)
    n = len(sk)
    ev = set()
    s, e = _starts(sk)
    per_tile = _tile_census(s, e, n, ev, "gr")
    T = kGroupThreads
    P = np.concatenate([[0], np.cumsum(rl)])  # points before sorted run i
    npoints = int(P[-1]) if npoints is None else npoints
    ev.add("kgr.scan" if (max(npoints, 1) + T - 1) // T > knobs.group_scan_tiles else "kgr.lookback")
    pts = P[e] - P[s]
    R = e - s
    tile = s // T
    route = np.empty(len(s), object)
    window = np.full(len(s), -1, np.int64)
    extra = np.zeros(len(s), np.int64)
    stage, inblock, small, W = knobs.stage, knobs.inblock, knobs.small_group, knobs.run_wave
    for L, o in zip(pts[pts > 1].tolist(), (s % T)[pts > 1].tolist()):
        ev.add(f"gp:{L}@{o}")
    for t in np.unique(tile):
        gi = np.flatnonzero(tile == t)
        t0, tend = t * T, min(n, (t + 1) * T)
        hi = e[gi[-1]]
        over = hi - tend
        nx = over if 0 < over <= kExtraRuns else 0
        if over > 0:
            extra[gi[-1]] = over
            if over == kExtraRuns:
                ev.add("kgr.extra=64")
            if over == kExtraRuns + 1:
                ev.add("kgr.extra=65")
        rend = tend + nx
        gs, ge = P[s[gi]], P[e[gi]]
        has = e[gi] <= rend  # the group's runs all have records in the block
        gp = ge - gs
        elig = has & (gp <= inblock)
        done = np.zeros(len(gi), bool)
        if W == 2:
            base = gs[0]
            used = 0
            for p in range(kRunPasses):
                inw = elig & ~done & (gs >= base) & (ge - base <= stage)
                if not inw.any():
                    break
                used = p + 1
                window[gi[inw]] = p
                done |= inw
                if p > 0 and (inw & (gp <= small)).any():
                    ev.add("kgr.short_next_window")
                left = elig & ~done
                if not left.any():
                    break
                base = gs[left].min()
            ev.add(f"kgr.windows={used}")
        else:
            done = elig & (ge - gs[0] <= stage)
            window[gi[done]] = 0
        nin = tend - s[gi]
        pin = P[tend] - gs
        est = np.where(has, gp, R[gi] * pin // np.maximum(nin, 1))
        huge = (W == 2) & ((est >= kHugeGroup) | (R[gi] >= kHugeRuns))
        for k, g in enumerate(gi):
            if done[k]:
                route[g] = "thread" if gp[k] <= small else ("lanes" if W == 2 else "wave")
                continue
            why = "cross" if not has[k] else "long" if gp[k] > inblock else \
                "windows" if W == 2 else "stage"
            route[g] = f"queue.{why}" + (".huge" if huge[k] else "")
            if why in ("windows", "stage") and gp[k] <= small:
                ev.add("kgr.queue.short")
            if huge[k] and not has[k]:
                if est[k] < kHugeGroup <= gp[k] and R[g] >= kHugeRuns:
                    ev.add("kgr.huge.est_low")
                if est[k] >= kHugeGroup > gp[k] and R[g] < kHugeRuns:
                    ev.add("kgr.huge.est_only")
    for r in set(route.tolist()):
        ev.add(f"kgr.route.{r}")
        if r.startswith("queue.windows"):
            ev.add("kgr.queue.windows")
    for cond, nm in ((pts == small, "kgr.pts=small"), (pts == small + 1, "kgr.pts=small+1"),
                     (pts == inblock, "kgr.pts=inblock"), (pts == inblock + 1, "kgr.pts=inblock+1"),
                     (pts > inblock, "kgr.pts=inblock+"),
                     (pts == stage, "kgr.pts=stage"), (pts == stage + 1, "kgr.pts=stage+1"),
                     (pts == kHugeGroup - 1, "kgr.pts=huge-1"), (pts == kHugeGroup, "kgr.pts=huge"),
                     (R == kHugeRuns - 1, "kgr.runs=huge-1"), (R == kHugeRuns, "kgr.runs=huge")):
        if cond.any():
            ev.add(nm)
    return {"events": ev, "tile_starts": per_tile, "start": s, "items": R, "points": pts,
            "offset": s % T, "crosses": e > (tile + 1) * T, "extra": extra, "route": route,
            "window": window}


def census(built, knobs=DEFAULT, run_keys=None, run_starts=None):
    """Both censuses of a built scene, from its sorted list alone: "points" (GDF_NO_XRUNS) and
    "runs" (the list's maximal runs, or the given run lists), and the union of their events."""
    keys = built["keys"]
    cp = census_points(np.sort(keys, kind="stable"), knobs)
    rk = built["run_keys"] if run_keys is None else run_keys
    rs = built["run_starts"] if run_starts is None else run_starts
    o = np.argsort(rk, kind="stable")
    cr = census_runs(np.asarray(rk)[o], np.diff(np.asarray(rs, np.int64))[o], knobs, len(keys))
    return {"points": cp, "runs": cr, "events": cp["events"] | cr["events"]}
