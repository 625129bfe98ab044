"""GPU segmentation front end on the built scenes of tests/seg_scenes.py, bit for bit against the
oracle (oracle/seg_oracle.c): tile corners and near-misses, the 1024/1025-block split of the
ranking, wave edges of the pixel pass, the 256-column steps and 64-row ballots of the contour scan
on both sides of the LDS limit, more than 256 layers, more than 1024 labels in the merge, cell
values >= 128, flags, unaligned grid pointers, buffer reuse and the 65535/65536 label limit.
test_seg_scenes.py (no GPU) proves that every scene holds its case."""
import numpy as np
import pytest

import seg_scenes as S
from conftest import gpu_available
from test_gpu_segment import assert_objects, gpu_front
from test_segment_kat import assert_same

pytestmark = pytest.mark.gpu

ALL_KEYS = ("labels", "num_labels", "stats", "centroids", "labels_to_contours",
            "contours_per_layer", "contour_sizes", "contour_points", "connections",
            "connection_starts", "merged", "num_objects")
BASE_KEYS = ALL_KEYS[:4]
CONTOUR_KEYS = ALL_KEYS[4:8]
CONNECTION_KEYS = ALL_KEYS[8:]


@pytest.fixture(scope="module")
def seg():
    if not gpu_available():
        pytest.fail("-m gpu test run without a visible GPU")
    from ros_gpu_depthmap_fusion_amd import build_library
    from ros_gpu_depthmap_fusion_amd.gdf import Segmenter
    build_library()
    s = Segmenter(0)
    yield s
    s.close()


def assert_all(r, o):
    assert set(r.keys()) == set(ALL_KEYS) == set(o.keys())
    assert_same(r, o, ALL_KEYS)


@pytest.mark.parametrize("name", S.NAMES)
def test_scene_bit_exact(seg, name):
    r = gpu_front(seg, S.get(name).copy())
    assert_all(r, S.oracle(name))


@pytest.mark.parametrize("H,W", S.ROOT_SHAPES)
def test_every_block_a_root_closed_form(seg, H, W):
    r = gpu_front(seg, S.get(f"every_block_a_root_{H}x{W}").copy())
    assert r["num_labels"].tolist() == [S.root_blocks(H, W) + 1]
    assert np.array_equal(r["labels"][0], S.root_labels(H, W))
    assert (r["stats"][1:, 2:] == 1).all()   # every component one cell


@pytest.mark.parametrize("W", S.BAR_WIDTHS)
def test_wave_bars_closed_form(seg, W):
    r = gpu_front(seg, S.get(f"wave_bars_{W}").copy())
    stats, cent = S.wave_bars_closed_form(W)
    assert r["num_labels"].tolist() == [3]
    assert np.array_equal(r["stats"], stats) and np.array_equal(r["centroids"], cent)


@pytest.mark.parametrize("name", ["zigzag_layers", "wide_merge"])
def test_objects_of_layer_scenes(seg, name):
    o = S.oracle(name)
    r = gpu_front(seg, S.get(name).copy())
    assert r["num_objects"] == o["num_objects"]
    assert_objects(seg, o)


@pytest.mark.parametrize("flags", [1, 2, 0])   # SEG_CONTOURS, SEG_CONNECTIONS, neither
@pytest.mark.parametrize("name", ["rings_across_step", "zigzag_layers"])
def test_flags(seg, name, flags):
    import torch
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONNECTIONS, SEG_CONTOURS, GDFError
    assert (SEG_CONTOURS, SEG_CONNECTIONS) == (1, 2)
    g, o = S.get(name), S.oracle(name)
    t = torch.from_numpy(g.copy()).cuda()
    torch.cuda.synchronize()
    L, H, W = g.shape
    seg.label_layers(t.data_ptr(), W, H, L, flags)
    con, cnn = bool(flags & SEG_CONTOURS), bool(flags & SEG_CONNECTIONS)
    r = seg.results(contours=con, connections=cnn)
    keys = BASE_KEYS + (CONTOUR_KEYS if con else ()) + (CONNECTION_KEYS if cnn else ())
    assert set(r.keys()) == set(keys)
    assert_same(r, o, keys)
    if not con:
        with pytest.raises(GDFError, match="contours were not requested"):
            seg.results(contours=True, connections=False)
    if not cnn:
        with pytest.raises(GDFError, match="connections were not requested"):
            seg.results(contours=False, connections=True)
        with pytest.raises(GDFError, match="connections were not requested"):
            seg.merge_labels()
        with pytest.raises(GDFError, match="connections were not requested"):
            seg.create_objects((0, 0, 0), (1, 1, 1))
    del t


GUARD = 64


@pytest.mark.parametrize("offset", [1, 4, 15])
@pytest.mark.parametrize("name", ["rings_across_step", "zigzag_layers", "step_edge_pixels"])
def test_unaligned_grid(seg, name, offset):
    """The grid at a byte offset inside a larger tensor of 0xFF: layer 0 takes the scalar staging
    path; a chunk load that reads a neighbour's bytes sees occupied cells."""
    import torch
    g = S.get(name)
    L, H, W = g.shape
    n = g.size
    host = np.full(GUARD + n + GUARD, 0xFF, np.uint8)
    start = 16 + offset
    host[start:start + n] = g.ravel()
    big = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    assert big.data_ptr() % 16 == 0
    view = big[start:start + n]
    assert view.data_ptr() % 16 == offset
    seg.label_layers(view.data_ptr(), W, H, L)
    r = seg.results()
    assert_all(r, S.oracle(name))
    back = big.cpu().numpy()
    assert (back[:start] == 0xFF).all() and (back[start + n:] == 0xFF).all()
    del view, big


def test_reuse_across_shapes(seg):
    """One segmenter, growing and shrinking shapes: grow-only buffers, reused contour scratch."""
    from ros_gpu_depthmap_fusion_amd.gdf import Segmenter
    s = Segmenter(0)
    try:
        for name in ("wide_merge", "tile_near_misses", "lds_limit_158", "cell_values", "wide_merge"):
            assert_all(gpu_front(s, S.get(name).copy()), S.oracle(name))
    finally:
        s.close()


@pytest.fixture(scope="module")
def limit_oracle():
    import oracle as oracle_mod
    return oracle_mod.object_segmentation_front(S.label_limit(True))


def test_label_limit_65536_raises(seg):
    import torch
    from ros_gpu_depthmap_fusion_amd.gdf import GDFError
    t = torch.from_numpy(S.label_limit(False)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(GDFError, match="65535"):
        seg.label_layers(t.data_ptr(), 512, 512, 1, 0)
    with pytest.raises(GDFError):
        seg.counts()
    del t


def test_label_limit_65535_passes(seg, limit_oracle):
    import torch
    t = torch.from_numpy(S.label_limit(True)).cuda()
    torch.cuda.synchronize()
    seg.label_layers(t.data_ptr(), 512, 512, 1, 0)
    r = seg.results(contours=False, connections=False)
    assert_same(r, limit_oracle, BASE_KEYS)
    assert r["labels"].max() == 65535 and r["num_labels"].tolist() == [65536]
    del t


def test_label_limit_65535_with_contours(seg, limit_oracle):
    """65535 single-point traces by one wave: labelling and downloads measured at 0.07 s on an
    MI355X (0.001 s without contours).  No connections: a single layer has none."""
    import torch
    from ros_gpu_depthmap_fusion_amd.gdf import SEG_CONTOURS
    t = torch.from_numpy(S.label_limit(True)).cuda()
    torch.cuda.synchronize()
    seg.label_layers(t.data_ptr(), 512, 512, 1, SEG_CONTOURS)
    r = seg.results(contours=True, connections=False)
    assert_same(r, limit_oracle, BASE_KEYS + CONTOUR_KEYS)
    assert r["contours_per_layer"].tolist() == [65535]
    assert (r["labels_to_contours"][1:] == np.arange(65535)[::-1]).all()
    del t
