"""Shared drivers for parity tests: replay GPUDepthmapFusionComponent::processDepthmaps
(src/gpu_depthmap_fusion_component.cpp:92-300) on either engine — the GPU engine
(ros_gpu_depthmap_fusion_amd.gdf.GPUDepthmapFusion) or the CPU oracle (oracle.OracleFusion) —
through their common method names, and compare the results.
"""
import numpy as np

from oracle import ros_time_minus


def stagewise_frame(eng, cams, params, T_world_move=None, T_crop_move=None):
    """The component's per-frame call sequence, one engine method per reference method."""
    eng.clear()
    for c in cams:
        eng.addDepthmap(*c)
    if not (len(cams) > 0 or eng.numCollectedPointSequencePoints() > 0):
        return False
    eng.uploadPointSequences()
    eng.filterNewPointSequences(params.ps_filter_threshold, params.ps_filter_size)
    eng.insertNewPointSequencesInRollbuffer()
    st = eng.rollbuffer_state()
    st = st.as_tuple() if hasattr(st, "as_tuple") else st
    last = (st[8], st[9])
    latest = earliest = (0, 0)
    if last != (0, 0):
        latest = last
        earliest = ros_time_minus(last[0], last[1], float(np.float32(params.ps_timespan)))
        assert earliest is not None
    eng.rollPointSequenceRollbufferCPU(*earliest)
    if T_world_move is not None:
        eng.selectPointSequenceTimespanCPU(earliest[0], earliest[1], latest[0], latest[1])
        eng.preparePointAndMaskBuffers()
        eng.insertSelectedPointSequence(T_world_move, T_crop_move)
        eng.transformPointSequence()
    else:
        eng.preparePointAndMaskBuffers()
    eng.uploadDepthmaps()
    eng.convertDepthmaps()
    eng.filterFlyingPixels(params.flying_filter_size, params.flying_threshold, params.flying_rot45)
    eng.cropPoints(params.crop_min, params.crop_max)
    eng.applyPointMask()
    if params.enable_voxel_filter:
        eng.computeVoxelCoords(params.voxel_min, params.voxel_max, params.voxel_size)
        eng.voxelize(params.voxel_average)
        eng.voxelOccupancyGrid(params.occupancy_lifetime)
    return True


def engine_with(Engine, **env):
    """An engine created with the given GDF_* environment knobs (read at creation)."""
    import os
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Engine()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_batch(gpu, p, frames):
    """One processFrame over `frames`: per frame the addDepthmap arguments of its cameras."""
    gpu.clear()
    for j, args in enumerate(frames):
        if j:
            gpu.nextFrameInBatch()
        for a in args:
            gpu.addDepthmap(*a)
    gpu.processFrame(p)


def compare_frames(gpu, ref, tag):
    """Every frame of the batch the engine just ran against the oracle's frame (ref: per frame a
    dict of the oracle's points, keys, vox, grid, and hist for the last): points, voxel keys,
    voxel means and grid bit for bit, and batch_ranges consistent with them."""
    pts, keys, vox = gpu.downloadPoints(), gpu.downloadVoxelCoords(), gpu.downloadVoxelizedPoints()
    B = len(ref)
    if B == 1:
        ps, vs = [0, len(pts)], [0, len(vox)]
    else:
        ps, vs = gpu.batch_ranges()
        assert len(ps) == B + 1 and len(vs) == B + 1, tag
        assert ps[0] == 0 and vs[0] == 0 and ps[B] == len(pts) and vs[B] == len(vox), tag
    for j, r in enumerate(ref):
        assert ps[j + 1] - ps[j] == len(r["points"]), (tag, j, ps[j + 1] - ps[j], len(r["points"]))
        assert vs[j + 1] - vs[j] == len(r["vox"]), (tag, j)
        assert np.array_equal(pts[ps[j]:ps[j + 1]].view(np.uint32), r["points"].view(np.uint32)), (tag, j)
        assert np.array_equal(keys[ps[j]:ps[j + 1]], r["keys"]), (tag, j)
        assert np.array_equal(vox[vs[j]:vs[j + 1], :3].view(np.uint32), r["vox"].view(np.uint32)), (tag, j)
        grid = gpu.downloadBatchVoxelOccupancyGrid(j) if B > 1 else gpu.downloadVoxelOccupancyGrid()
        assert np.array_equal(grid, r["grid"]), (tag, j)
    assert np.array_equal(gpu.downloadVoxelOccupancyGrid(), ref[-1]["grid"]), tag
    assert np.array_equal(gpu.historic_grid(), ref[-1]["hist"]), tag


def voxelize_parts_and_compare(gpu, nparts, B, sp, srk, srs, cnt, want, want_keys, tag):
    """The send lists of a key-range partition (gdf_partition_runs or gdf_set_emit_partition:
    points sp, run keys srk, run starts srs, counts cnt, all hiprt.DeviceArray) of the B-frame
    batch the engine just ran: every part voxelized on its own with gdf_voxelize_runs_marked (as
    two sources split at a run boundary), the parts' voxels concatenated in part order, equal
    want[j] (frame j's voxel means) bit for bit, and the parts' marks, each confined to its own
    word slice, unite to the marks of want_keys[j] (frame j's voxel keys)."""
    from ros_gpu_depthmap_fusion_amd import hiprt, multi
    c = cnt.to_numpy(np.uint32, 2 * nparts)
    pts, runs = c[:nparts].astype(np.int64), c[nparts:].astype(np.int64)
    n = int(pts.sum())
    assert (runs <= pts).all() and ((runs > 0) == (pts > 0)).all()
    P0, R0 = np.concatenate([[0], np.cumsum(pts)]), np.concatenate([[0], np.cumsum(runs)])
    h_rs = srs.to_numpy(np.uint32, max(n, 1))
    # every part's voxel marks (gdf_voxelize_runs_marked): frame j at j * stride words; part q's
    # keys are whole mark words [q S, (q + 1) S) (the fused step all-gathers those slices)
    ncells = int(gpu.grid_size()[1])
    words = (ncells + 31) // 32
    S = multi.part_slice_words(nparts, ncells)
    stride = S * nparts
    union = np.zeros((B, stride), np.uint32)
    want_marks = np.zeros((B, words), np.uint32)
    for j in range(B):
        k = np.unique(want_keys[j].astype(np.int64))
        np.bitwise_or.at(want_marks[j], k >> 5, (np.uint32(1) << (k & 31).astype(np.uint32)))
    got = [[] for _ in range(B)]
    for q in range(nparts):
        if pts[q] == 0:
            continue
        rs = h_rs[R0[q]:R0[q + 1]]
        assert rs[0] == 0 and (np.diff(rs.astype(np.int64)) > 0).all() and rs[-1] < pts[q]
        # the part as two sources split at a run boundary (a key range from two ranks)
        cut = len(rs) // 2
        pb = np.array([0, rs[cut], pts[q]] if cut else [0, pts[q]], np.uint32)
        rb = np.array([0, cut, len(rs)] if cut else [0, len(rs)], np.uint32)
        local = rs.astype(np.uint32).copy()
        if cut:
            local[cut:] -= rs[cut]
        drs = hiprt.DeviceArray.from_numpy(np.concatenate([local, np.zeros(1, np.uint32)]))
        dmk = hiprt.DeviceArray.from_numpy(np.zeros(B * stride, np.uint32))
        gpu.voxelize_runs_marked(sp.ptr + 16 * int(P0[q]), srk.ptr + 4 * int(R0[q]), drs.ptr, pb, rb,
                                 dmk.ptr, stride)
        gpu.synchronize()
        mk = dmk.to_numpy(np.uint32, B * stride).reshape(B, stride)
        outside = np.ones(stride, bool)
        outside[q * S:(q + 1) * S] = False
        assert not mk[:, outside].any(), (tag, q)
        union |= mk
        vox = gpu.downloadVoxelizedPoints()[:, :3]
        if B > 1:
            _, vs = gpu.batch_ranges()
            for j in range(B):
                got[j].append(vox[vs[j]:vs[j + 1]])
        else:
            got[0].append(vox)
    for j in range(B):
        g = np.concatenate(got[j]) if got[j] else np.zeros((0, 3), np.float32)
        assert len(g) == len(want[j]) > 0, (tag, j)
        assert np.array_equal(g.view(np.uint32), want[j].view(np.uint32)), (tag, j)
        assert np.array_equal(union[j, :words], want_marks[j]), (tag, j)
        assert not union[j, words:].any()


def bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return a.view(np.uint32)


def compare_results(gpu, orc, voxel=True, exact_points=True, tag=""):
    pg, po = gpu.downloadPoints(), orc.downloadPoints()
    assert len(pg) == len(po), f"{tag} point count gpu {len(pg)} oracle {len(po)}"
    if exact_points:
        bad = np.flatnonzero((bits(pg) != bits(po)).any(axis=1))
        assert len(bad) == 0, f"{tag} {len(bad)} points differ, first {bad[:5]}: {pg[bad[:3]]} vs {po[bad[:3]]}"
    else:
        np.testing.assert_allclose(pg[:, :3], po[:, :3], atol=1e-5, rtol=0)
    if not voxel:
        return
    cg, co = gpu.downloadVoxelCoords(), orc.downloadVoxelCoords()
    np.testing.assert_array_equal(cg, co, err_msg=f"{tag} voxel coords")
    vg, vo = gpu.downloadVoxelizedPoints(), orc.downloadVoxelizedPoints()
    assert len(vg) == len(vo), f"{tag} voxelized count gpu {len(vg)} oracle {len(vo)}"
    bad = np.flatnonzero((bits(vg[:, :3]) != bits(vo[:, :3])).any(axis=1))
    assert len(bad) == 0, f"{tag} {len(bad)} voxel means differ: {vg[bad[:3]]} vs {vo[bad[:3]]}"
    gg, go = gpu.downloadVoxelOccupancyGrid(), orc.downloadVoxelOccupancyGrid()
    assert gg.shape == go.shape
    nd = np.count_nonzero(gg != go)
    assert nd == 0, f"{tag} occupancy grid: {nd} cells differ"
    hg, ho = gpu.historic_grid(), orc.historic_grid()
    np.testing.assert_array_equal(hg, ho, err_msg=f"{tag} historic grid")
