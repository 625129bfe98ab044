"""CPU restatement of the segmented radius outlier filter (include/gdf_filter.h): the rule of
radius_ref.py applied to every segment [start[s], start[s + 1]) on its own, the results
concatenated in segment order.  Rows behind start[nseg] are never looked at.  Also the sparse cell
plan in Python doubles."""
import numpy as np

import radius_ref as R


def reference_segments(pts, starts, lower, upper, radius, min_neighbors):
    """(keep flags [start[nseg]] bool, out_start [nseg + 1] uint32): keep per input row below
    start[nseg], and the number of kept rows before each segment's start."""
    p = R._f32(pts)
    starts = [int(s) for s in starts]
    assert starts[0] == 0 and all(a <= b for a, b in zip(starts, starts[1:])) and starts[-1] <= len(p)
    keep = np.zeros(starts[-1], bool)
    for a, b in zip(starts, starts[1:]):
        if b > a:
            keep[a:b] = R.reference(p[a:b], lower, upper, radius, min_neighbors)[0]
    out_start = np.array([keep[:s].sum() for s in starts], np.uint32)
    return keep, out_start


def apply_segments(pts, keep):
    """The output: the kept rows below start[nseg] in input order, all four words."""
    return R._f32(pts)[:len(keep)][np.asarray(keep, bool)]


def plan_sparse_py(lower, upper, radius):
    """The sparse plan: the per-axis rule of the dense plan with no cap on the product."""
    r32 = np.float32(radius)
    r = float(r32)
    tiny = float(np.float32(r32 * r32)) < 2.0 ** -100
    ext = [float(np.float32(u)) - float(np.float32(l)) for l, u in zip(lower, upper)]
    cells = []
    for e in ext:
        c = 1 if tiny or e > 2.0 ** 100 else int(min(max(1, np.floor(e / (r * (1 + 2.0 ** -10)))), 1024))
        cells.append(c)
    return tuple(cells), [e / c for e, c in zip(ext, cells)]
