"""tools/crop_stats.py: the share of the px kernels' work the crop box discards (CPU only)."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import crop_stats  # noqa: E402


@pytest.mark.parametrize("workload", ["dense", "stress"])
def test_fractions_of_a_small_camera(workload):
    r = crop_stats.crop_stats(64, 48, workload, frames=2)
    assert set(r) == {"rings_today", "rings_crop", "waves_empty", "segs_empty"}
    for k, v in r.items():
        assert 0.0 <= v <= 1.0, (k, v)
    assert r["rings_crop"] <= r["rings_today"]
    # a 64-pixel row is one segment with one wave: the two unit fractions coincide
    assert r["waves_empty"] == r["segs_empty"]


def test_an_empty_box_discards_everything():
    r = crop_stats.crop_stats(64, 48, "dense", crop_min=(100.0, 100.0, 100.0),
                              crop_max=(101.0, 101.0, 101.0))
    assert r["rings_crop"] == 0.0 and r["waves_empty"] == 1.0 and r["segs_empty"] == 1.0
    assert r["rings_today"] > 0.0
