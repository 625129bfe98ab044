"""The voxelize stage on built key lists (tests/voxel_lists.py): gdf_voxelize_points,
gdf_voxelize_runs and gdf_voxelize_runs_marked on lists that sit on the edges of k_sort_pass,
k_group, k_group_runs / k_group_runs_big and k_xruns_count / k_xruns_emit, at seven key widths,
with runs cut from the list and with sorted points (GDF_NO_XRUNS), means and corners, under the
knob sets that switch kernels, at unaligned addresses, split over sources, with batch keys, on a
reused engine.  The reference is tests/voxel_ref.py (tied to the C oracle and proved on the CPU by
tests/test_voxel_lists.py).  Every comparison is bit for bit; there is no tolerance anywhere."""
import os

import numpy as np
import pytest

import voxel_lists as vl
from ros_gpu_depthmap_fusion_amd import hiprt, synth
from ros_gpu_depthmap_fusion_amd.gdf import ComponentParams, GDFError
from voxel_ref import Grid, cut_runs, expand_runs, marks_ref, runs_of, voxelize_ref

pytestmark = pytest.mark.gpu

SCENES = vl.scenes()
BY_NAME = {s.name: s for s in SCENES}
WIDTH_SCENES = [s for s in SCENES if s.family in ("lengths", "digits")]
STRUCT_SCENES = [s for s in SCENES if s.family not in ("lengths", "digits")]
KNOB_SCENES = [s for s in SCENES if s.family in vl.KNOB_FAMILIES]
RUN_SCENES = [s for s in SCENES if s.family in ("runs_per_group", "long_run", "windows",
                                                "estimate", "staged")]
GRID = {b: Grid(*g) for b, g in vl.GRIDS.items()}
NO_XRUNS = {"GDF_NO_XRUNS": "1"}
CANARY = 0xA5C3F00D

_built, _ref, _queue = {}, {}, {}


def built(scene, bits=22):
    k = (scene.name, bits)
    if k not in _built:
        _built[k] = scene.build(GRID[bits].ncells)
    return _built[k]


def ref(scene, bits, average):
    """(distinct keys, rows) of the scene at that width: computed once, shared, never changed."""
    k = (scene.name, bits, average)
    if k not in _ref:
        b = built(scene, bits)
        d, r = voxelize_ref(b["keys"], b["pts"], average=average, grid=GRID[bits])
        r.setflags(write=False)
        _ref[k] = (d, r)
    return _ref[k]


def queue_counts(scene, bits, knobs, runs=None):
    """(queued, huge) groups of k_group_runs by the census, for the list's maximal runs or the
    given (tag, run_keys, run_starts)."""
    k = (scene.name, bits, knobs, runs[0] if runs else None)
    if k not in _queue:
        c = vl.census(built(scene, bits), knobs, *(runs[1:] if runs else ()))["runs"]
        huge = sum(1 for r in c["route"] if r.endswith(".huge"))
        _queue[k] = (sum(1 for r in c["route"] if r.startswith("queue.")) - huge, huge)
    return _queue[k]


@pytest.fixture(scope="module")
def Engine(gpu_engine_factory):
    return gpu_engine_factory


def cam_args(cam, depth):
    return (depth, *cam.intrinsics(), cam.T_world, cam.T_crop)


def make_engine(Engine, bits, env=None, nframes=1, knobs=vl.DEFAULT):
    """An engine created under `env` (`knobs`: what the census needs of it) whose voxel grid (set
    by tiny frames - a batch of them for nframes > 1) has the wanted key width."""
    env = env or {}
    os.environ.update(env)
    try:
        gpu = Engine()
    finally:
        for k in env:
            os.environ.pop(k, None)
    p = ComponentParams()
    p.voxel_min, p.voxel_max, p.voxel_size = vl.GRIDS[bits]
    cam = synth.make_camera(0, 64, 48)
    gpu.clear()
    for f in range(nframes):
        if f:
            gpu.nextFrameInBatch()
        gpu.addDepthmap(*cam_args(cam, synth.dense_frame(cam, 0, f)))
    gpu.processFrame(p)
    assert gpu.grid_size() == (GRID[bits].gs, GRID[bits].ncells)
    gpu.knobs, gpu.xruns = knobs, "GDF_NO_XRUNS" not in env
    return gpu


def upload(a, offset_bytes=0):
    """(device array, pointer): the array `offset_bytes` past the allocation's (aligned) start."""
    a = np.ascontiguousarray(a)
    raw = np.concatenate([np.zeros(offset_bytes, np.uint8), a.reshape(-1).view(np.uint8)])
    d = hiprt.DeviceArray.from_numpy(raw)
    return d, d.ptr + offset_bytes


def assert_rows(got, want, keys, tag):
    assert len(got) == len(want), (tag, "rows", len(got), "distinct keys", len(want))
    if len(want) == 0:
        return
    g = np.ascontiguousarray(got, np.float32).view(np.uint32)
    w = np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert len(bad) == 0, (tag, f"{len(bad)} of {len(w)} rows differ; first: row {bad[0]}, "
                           f"key {keys[bad[0]]}", got[bad[0]], want[bad[0]])


def check_points(gpu, scene, bits, average, tag, koff=0, poff=0):
    b = built(scene, bits)
    dk, kp = upload(b["keys"], koff)
    dp, pp = upload(b["pts"], poff)
    gpu.voxelize_points(pp, kp, len(b["keys"]), average)
    got = gpu.downloadVoxelizedPoints()
    keys, want = ref(scene, bits, average)
    assert_rows(got, want, keys, (tag, scene.name, bits, "mean" if average else "corner"))
    # the groups k_group_runs queued are the census's (none for corners or sorted points)
    expect = queue_counts(scene, bits, gpu.knobs) if gpu.xruns and average else (0, 0)
    assert gpu.last_group_queue() == expect, (tag, scene.name, bits, "queued, huge groups")
    return got


# ---- every scene x {runs cut from the list, sorted points} x {means, corners} ----------------------
@pytest.mark.parametrize("xruns", [True, False], ids=["xruns", "points"])
@pytest.mark.parametrize("bits", sorted(vl.GRIDS))
def test_digits_and_lengths_at_every_width(Engine, bits, xruns):
    """The sort's digit scenes and the list lengths at key widths 8, 9, 16, 17, 22, 25, 26: one
    8-bit pass, one 9-bit pass, 8+8, 8+9, 8+8+8, 8+8+9 and four passes.  n = 0 gives zero rows."""
    gpu = make_engine(Engine, bits, None if xruns else NO_XRUNS)
    for sc in WIDTH_SCENES:
        for average in (True, False):
            got = check_points(gpu, sc, bits, average, "widths")
            if len(built(sc, bits)["keys"]) == 0:
                assert len(got) == 0
    gpu.close()


@pytest.mark.parametrize("xruns", [True, False], ids=["xruns", "points"])
def test_structure_scenes(Engine, xruns):
    """The ladder, tile-edge, staged-window, runs-per-group, long-run, staging-window, estimate
    and default-scan scenes at 22 bits."""
    gpu = make_engine(Engine, 22, None if xruns else NO_XRUNS)
    for sc in STRUCT_SCENES:
        for average in (True, False):
            check_points(gpu, sc, 22, average, "structure")
    gpu.close()


# ---- knob sets ------------------------------------------------------------------------------------
# (a knob set of k_group_runs knobs alone is not paired with sorted points, which never reach it)
KNOB_PAIRS = [(k, x) for k in sorted(vl.KNOB_SETS) for x in (True, False)
              if x or not all(v.startswith("GDF_RUN_") for v in vl.KNOB_SETS[k][0])]


@pytest.mark.parametrize("knob,xruns", KNOB_PAIRS,
                         ids=[f"{k}-{'xruns' if x else 'points'}" for k, x in KNOB_PAIRS])
def test_knob_sets(Engine, knob, xruns):
    """The structure scenes under every knob set that switches a kernel, a route or a grid size.
    Whether a scene still sits on its edge under a knob set is a property of the census:
    tests/test_voxel_lists.py asserts it for every pairing but the events vl.OFF_EDGE lists, and
    here every pairing runs and is compared, on its edge or off it."""
    env, knobs = vl.KNOB_SETS[knob]
    gpu = make_engine(Engine, 22, dict(env, **({} if xruns else NO_XRUNS)), knobs=knobs)
    for sc in KNOB_SCENES:
        for average in (True, False):
            check_points(gpu, sc, 22, average, knob)
    gpu.close()


# ---- unaligned lists ------------------------------------------------------------------------------
@pytest.mark.parametrize("xruns", [True, False], ids=["xruns", "points"])
def test_unaligned_lists(Engine, xruns):
    """The key pointer 4, 8 and 12 bytes past a 16-byte border (the scalar path of the run
    cutting), the point pointer 16 bytes past the allocation's start."""
    gpu = make_engine(Engine, 22, None if xruns else NO_XRUNS)
    names = [f"len_{n}_{r}" for n in (4095, 4096, 4097) for r in ("range50", "whole")]
    names.append("ladder_513_at255")
    for nm in names:
        for koff in (4, 8, 12, 0):
            for poff in (16, 0):
                check_points(gpu, BY_NAME[nm], 22, True, ("unaligned", koff, poff), koff, poff)
    gpu.close()


# ---- gdf_voxelize_runs ----------------------------------------------------------------------------
def source_borders(R, S, rng, inside=None):
    """Run-index borders of S sources over R runs (S + 1 entries): for S >= 2 the first source is
    empty, for S >= 5 one in the middle and the last are empty too; `inside` (a run index) is made
    a border when there is room."""
    if S == 1:
        return np.array([0, R])
    free = S - (1 if S < 5 else 3) - 1  # inner borders to choose
    cand = rng.choice(np.arange(1, R), min(free, R - 1), replace=False) if R > 1 and free else []
    inner = sorted(set(int(c) for c in cand))
    if inside is not None and 0 < inside < R and inner:
        inner[0] = inside
        inner = sorted(set(inner))
    b = [0, 0] + inner
    if S >= 5 and inner:  # an empty source in the middle
        m = inner[len(inner) // 2]
        b = sorted(b + [m])
    b = b + [R] * (S + 1 - len(b))
    return np.array(b)


def call_runs(gpu, pts, rk, rs, borders, average=True, marks=None, stride=0):
    """gdf_voxelize_runs[_marked] on the run lists split at `borders`: each source's run starts
    relative to its first point, as gdf_partition_runs writes them."""
    rs = np.asarray(rs, np.int64)
    pb = rs[borders]
    src = np.searchsorted(borders, np.arange(len(rk)), side="right") - 1
    rel = np.concatenate([rs[:-1] - pb[src], [0]]).astype(np.uint32)  # (R + 1 entries)
    dp, dk, ds = upload(pts), upload(rk), upload(rel)
    args = (dp[1] if len(pts) else 0, dk[1] if len(rk) else 0, ds[1], pb.astype(np.uint32),
            borders.astype(np.uint32))
    if marks is None:
        gpu.voxelize_runs(*args, average)
    else:
        gpu.voxelize_runs_marked(*args, marks, stride, average)
    return gpu.downloadVoxelizedPoints()


@pytest.mark.parametrize("nsources", [1, 2, 5, 32])
def test_voxelize_runs_over_sources(Engine, nsources):
    """Every runs scene as run lists - the list's maximal runs, and those cut further at random
    points - split over 1, 2, 5 and 32 sources with empty sources at the start, in the middle and
    at the end and a border inside a maximal run: the rows of gdf_voxelize_points on the same
    points, and the reference's."""
    gpu = make_engine(Engine, 22)
    rng = np.random.default_rng(7 + nsources)
    for sc in RUN_SCENES:
        b = built(sc)
        keys, want = ref(sc, 22, True)
        n = len(b["keys"])
        base = check_points(gpu, sc, 22, True, "runs: points call")
        cuts = np.random.default_rng(vl._seed(sc.name)).integers(1, max(n, 2), max(n // 7, 3))
        ck, cs = cut_runs(b["run_keys"], b["run_starts"], cuts)  # (one cut list per scene)
        assert np.array_equal(expand_runs(ck, cs), b["keys"])
        same = np.flatnonzero(ck[1:] == ck[:-1]) + 1  # borders inside a maximal run
        for tag, rk, rs, inside in (("maximal", b["run_keys"], b["run_starts"], None),
                                    ("cut", ck, cs, int(same[len(same) // 2]) if len(same) else None)):
            borders = source_borders(len(rk), nsources, rng, inside)
            assert len(borders) == nsources + 1 and (np.diff(borders) >= 0).all()
            got = call_runs(gpu, b["pts"], rk, rs, borders)
            assert_rows(got, want, keys, ("runs", tag, sc.name, nsources))
            assert gpu.last_group_queue() == queue_counts(sc, 22, gpu.knobs, (tag, rk, rs)), (tag, sc.name)
            assert np.array_equal(got.view(np.uint32), base.view(np.uint32))
    # no runs at all
    got = call_runs(gpu, np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), np.zeros(1, np.uint32),
                    np.zeros(nsources + 1, np.int64))
    assert len(got) == 0
    gpu.close()


@pytest.mark.parametrize("bits", [9, 22])
def test_voxelize_runs_marked(Engine, bits):
    """gdf_voxelize_runs_marked: the marks equal the occupancy bitmask of the distinct keys, and a
    canary pattern in the words past the grid's mark words stays untouched."""
    gpu = make_engine(Engine, bits)
    words = GRID[bits].mark_words
    extra = 64
    scenes = [s for s in WIDTH_SCENES if s.family == "digits"]
    if bits == 22:
        scenes += [BY_NAME[n] for n in ("ladder_33_at255", "runs_321_of_16", "windows_256_groups_of_40",
                                        "estimate_low_huge_by_runs", "long_run_2049")]
    for sc in scenes:
        for average in (True, False):
            b = built(sc, bits)
            keys, want = ref(sc, bits, average)
            host = np.concatenate([np.zeros(words, np.uint32), np.full(extra, CANARY, np.uint32)])
            dm = hiprt.DeviceArray.from_numpy(host)
            R = len(b["run_keys"])
            got = call_runs(gpu, b["pts"], b["run_keys"], b["run_starts"], np.array([0, R // 2, R]),
                            average, dm.ptr, words)
            assert_rows(got, want, keys, ("marked", sc.name, bits, average))
            m = dm.to_numpy(np.uint32, words + extra)
            assert np.array_equal(m[:words], marks_ref(keys, words)), (sc.name, "marks")
            assert (m[words:] == CANARY).all(), (sc.name, "canary")
    gpu.close()


# ---- batch keys -----------------------------------------------------------------------------------
def batch_list(bits, per_frame):
    """The frames' scenes (None: an empty frame) as one list whose keys carry the frame above
    key_bits, the frames' points interleaved in blocks; and the reference rows and voxel starts."""
    kb = GRID[bits].key_bits
    keys, pts, rows, dist, vs = [], [], [], [], [0]
    for f, sc in enumerate(per_frame):
        if sc is not None:
            b = built(sc, bits)
            keys.append(b["keys"] | np.uint32(f << kb))
            pts.append(b["pts"])
            d, r = ref(sc, bits, True)
            rows.append(r)
            dist.append(d)
        vs.append(vs[-1] + (len(ref(sc, bits, True)[0]) if sc is not None else 0))
    # blocks of 100 points, frames in turn (each frame keeps its own order)
    chunks = []
    for k, p in zip(keys, pts):
        chunks.append([(k[i:i + 100], p[i:i + 100]) for i in range(0, len(k), 100)])
    order = []
    for i in range(max(len(c) for c in chunks)):
        order += [c[i] for c in reversed(chunks) if i < len(c)]
    return (np.concatenate([o[0] for o in order]), np.concatenate([o[1] for o in order]),
            np.concatenate(rows), np.concatenate(dist), np.array(vs, np.uint32))


@pytest.mark.parametrize("xruns", [True, False], ids=["xruns", "points"])
@pytest.mark.parametrize("bits,nframes", [(9, 3), (22, 3), (22, 8)])
def test_batch_keys(Engine, bits, nframes, xruns):
    """After a batch of tiny frames, lists whose keys carry the frame above key_bits (22 bits and
    8 frames: 25-bit sort keys, a 9-bit last digit): rows per frame and batch_ranges()'s voxel
    starts, with frame 1 empty, the last frame empty, and all points in frame 0."""
    gpu = make_engine(Engine, bits, None if xruns else NO_XRUNS, nframes)
    A, B, C = BY_NAME["digits_uniform"], BY_NAME["len_1025_range50"], BY_NAME["len_4097_whole"]
    if bits == 22:
        B, C = BY_NAME["ladder_33_at255"], BY_NAME["runs_321_of_1"]
    fill = [A, B, C, A, C, B, A, B][:nframes]
    cases = {"frame 1 empty": [fill[0], None] + fill[2:],
             "last frame empty": fill[:-1] + [None],
             "all in frame 0": [C] + [None] * (nframes - 1),
             "every frame": fill}
    for tag, per_frame in cases.items():
        keys, pts, rows, dist, vs = batch_list(bits, per_frame)
        dk, dp = upload(keys), upload(pts)
        gpu.voxelize_points(dp[1], dk[1], len(keys))
        got = gpu.downloadVoxelizedPoints()
        _, gvs = gpu.batch_ranges()
        assert np.array_equal(gvs, vs), (tag, gvs, vs)
        for f in range(nframes):
            assert_rows(got[vs[f]:vs[f + 1]], rows[vs[f]:vs[f + 1]], dist[vs[f]:vs[f + 1]],
                        ("batch", tag, "frame", f))
        assert len(got) == vs[-1]
        if not xruns:
            continue
        # the same list as run lists over two sources, every frame's marks at its stride
        words, extra = GRID[bits].mark_words, 64
        stride = words + 3
        host = np.full(nframes * stride + extra, CANARY, np.uint32)
        for f in range(nframes):
            host[f * stride:f * stride + words] = 0
        outside = host == CANARY
        dm = hiprt.DeviceArray.from_numpy(host)
        rk, rs = runs_of(keys)
        got = call_runs(gpu, pts, rk, rs, np.array([0, len(rk) // 3, len(rk)]), True, dm.ptr, stride)
        assert np.array_equal(gpu.batch_ranges()[1], vs), tag
        assert_rows(got, rows, dist, ("batch runs", tag))
        m = dm.to_numpy(np.uint32, len(host))
        for f in range(nframes):
            assert np.array_equal(m[f * stride:f * stride + words],
                                  marks_ref(dist[vs[f]:vs[f + 1]], words)), (tag, "marks of frame", f)
        assert (m[outside] == CANARY).all(), (tag, "canary")
    gpu.close()


# ---- one engine reused ----------------------------------------------------------------------------
@pytest.mark.parametrize("xruns", [True, False], ids=["xruns", "points"])
def test_one_engine_reused(Engine, xruns):
    """All scenes of the 22-bit width twice on one engine, the largest and the smallest lists in
    turn: look-back epochs, self-resetting counters, the digit histogram the group kernel clears,
    buffers that only grow."""
    gpu = make_engine(Engine, 22, None if xruns else NO_XRUNS)
    by_size = sorted(SCENES, key=lambda s: len(built(s)["keys"]))
    order = []
    while by_size:
        order.append(by_size.pop())
        if by_size:
            order.append(by_size.pop(0))
    for rnd in range(2):
        for i, sc in enumerate(order):
            check_points(gpu, sc, 22, (i + rnd) % 3 != 0, ("reuse", rnd))
    gpu.close()


# ---- refusals -------------------------------------------------------------------------------------
def test_voxelize_runs_refusals(Engine):
    """Malformed source lists are refused with GDF_ERR_ARG and leave the engine usable."""
    gpu = make_engine(Engine, 22)
    sc = BY_NAME["runs_257_of_16"]
    b = built(sc)
    keys, want = ref(sc, 22, True)
    R, n = len(b["run_keys"]), len(b["keys"])
    dp, dk = upload(b["pts"]), upload(b["run_keys"])
    ds = upload(b["run_starts"])
    u32 = lambda *v: np.array(v, np.uint32)
    mid_r = R // 2
    mid_p = int(b["run_starts"][mid_r])
    bad = {
        "0 sources": (dp[1], dk[1], ds[1], u32(0), u32(0)),
        "33 sources": (dp[1], dk[1], ds[1], np.linspace(0, n, 34).astype(np.uint32),
                       np.linspace(0, R, 34).astype(np.uint32)),
        "decreasing point bases": (dp[1], dk[1], ds[1], u32(0, mid_p + 1, mid_p, n), u32(0, mid_r, mid_r + 1, R)),
        "decreasing run bases": (dp[1], dk[1], ds[1], u32(0, mid_p, mid_p + 1, n), u32(0, mid_r + 1, mid_r, R)),
        "points without runs": (dp[1], dk[1], ds[1], u32(0, mid_p, n), u32(0, R, R)),
        "runs without points": (dp[1], dk[1], ds[1], u32(0, n, n), u32(0, mid_r, R)),
        "null points": (0, dk[1], ds[1], u32(0, n), u32(0, R)),
        "null run keys": (dp[1], 0, ds[1], u32(0, n), u32(0, R)),
        "null run starts": (dp[1], dk[1], 0, u32(0, n), u32(0, R)),
    }
    for tag, args in bad.items():
        with pytest.raises(GDFError) as ei:
            gpu.voxelize_runs(*args)
        assert ei.value.status == -1, (tag, ei.value)  # GDF_ERR_ARG
        # the engine is usable: a valid call afterwards is correct
        got = call_runs(gpu, b["pts"], b["run_keys"], b["run_starts"], np.array([0, mid_r, R]))
        assert_rows(got, want, keys, ("after refusal", tag))
    gpu.close()
