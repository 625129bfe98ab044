"""The scenes of tests/px_scenes.py hold the cases they were built for (no GPU): every scene is
built, run through the oracle, and its content assertion - a condition on the INPUTS, read from
the oracle's stage masks - checked.  The GPU tests (test_gpu_px_shapes.py, test_gpu_crop_first.py)
run exactly these scenes; a scene that lost its case would leave them passing and testing nothing.
"""
import numpy as np
import pytest

import px_scenes as S


def test_segment_split_and_px_eligible_widths():
    """The engine's split under GDF_SEG_ITEMS=256: px-eligible (widest segment 256) are exactly
    193..256, 385..512 and 577..768 of the widths up to 768; the scenes' widths are among them,
    257 and 320 are not."""
    ok = {W for W in range(1, 769) if S.px_eligible(W)}
    assert ok == set(range(193, 257)) | set(range(385, 513)) | set(range(577, 769))
    assert all(W in ok for W in S.WIDTHS + (S.HEIGHT_W, 448))
    assert S.segments(257, 256) == ([(0, 192), (192, 65)], 192)
    assert S.segments(320, 256)[1] == 192 and S.segments(320, 1024) == ([(0, 320)], 320)
    assert S.segments(449, 256) == ([(0, 256), (256, 193)], 256)
    assert S.segments(577, 256) == ([(0, 256), (256, 256), (512, 65)], 256)
    assert S.segments(1211, 1024) == ([(0, 640), (640, 571)], 640)
    # thread t owns x0 + t and x0 + t + 128
    assert np.array_equal(S.wave_columns(256, 192, 0), np.r_[256:320, 384:448])
    assert np.array_equal(S.wave_columns(256, 192, 1), np.r_[320:384])


@pytest.mark.parametrize("W", [320, 448])
@pytest.mark.parametrize("name", ["batch", "nocrop", "twocam"])
def test_crop_first_scenes(name, W):
    sc = S.crop_scene(name, W)
    assert len(sc.ref) == len(sc.frames) == (3 if name == "batch" else 1)
    if name == "batch":
        assert all(len(r["points"]) > 0 for r in sc.ref)  # (the partition test needs every frame)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("W", S.WIDTHS)
def test_width_scenes(W, wrap):
    sc = S.width_scene(W, wrap)
    S.width_scene_contents(W, sc, wrap)
    assert (sc.params.flying_threshold == 0.3) == (not wrap)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("H", S.HEIGHTS)
def test_height_scenes(H, two):
    sc = S.height_scene(H, two)
    assert len(sc.frames[0]) == (2 if two else 1)
    assert all(a[0].shape == (H, S.HEIGHT_W) for a in sc.frames[0])


@pytest.mark.parametrize("h0", [7, 9])
def test_mixed_camera_scenes(h0):
    sc = S.mixed_scene(h0)
    assert [a[0].shape for a in sc.frames[0]] == [(h0, 199), (12, 448), (10, 96)]


def test_device_scene_is_the_391x12_map():
    sc = S.device_scene()
    (depth, *_), = sc.frames[0]
    assert depth.shape == (12, 391) and len(sc.ref[0]["points"]) > 0
    # the padding value of the device test (3000 mm) differs from every pixel of the map: a chunk
    # load that leaks a neighbour changes a depth
    assert (depth != 3000).all()


@pytest.mark.parametrize("all_empty", [False, True])
def test_empty_batch_scenes(all_empty):
    sc = S.empty_batch_scene(all_empty)
    assert len(sc.frames) == 4 and all(f[0][0].shape == (16, 448) for f in sc.frames)


@pytest.mark.parametrize("ncams", [1, 2])
def test_640_scenes(ncams):
    sc = S.p640_scene(ncams)
    assert [a[0].shape for a in sc.frames[0]] == [(720 if ncams == 1 else 400, 1211)] * ncams
