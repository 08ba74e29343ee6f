"""The depth runs' and the depth profile's contracts once more (tests/runs_ref.py, tests/depth_ref.py), for contigs too long
for a per-position array: from the breakpoints of reads of one M operation each.  Integers throughout.  Nothing here calls
the library."""
import numpy as np

import runs_ref


def depth(start, end, extent):
    """reads [start[i], end[i]) -> (points, depth): the sorted distinct points 0, starts and ends below the extent, and the
    depth of [points[i], points[i + 1]) -- the last stretch ends at the extent"""
    start = np.asarray(start, np.int64).reshape(-1)
    end = np.asarray(end, np.int64).reshape(-1)
    assert start.shape == end.shape and np.all(start >= 0) and np.all(end >= start)
    pts = np.unique(np.concatenate((np.zeros(1, np.int64), start, end)))
    pts = pts[pts < extent]
    n = pts.shape[0]
    # a start or an end at or beyond the extent falls into slot n, which nobody reads
    step = (np.bincount(np.searchsorted(pts, start), minlength=n + 1).astype(np.int64)
            - np.bincount(np.searchsorted(pts, end), minlength=n + 1).astype(np.int64))
    d = np.cumsum(step[:n])
    assert n == 0 or int(d.min()) >= 0
    return pts, d.astype(np.uint64)


def runs(start, end, extent, edges=None):
    """(start, value) as runs_ref.runs gives them for the per-position depth of these reads"""
    pts, d = depth(start, end, extent)
    v = runs_ref.values(d, edges)
    if v.shape[0] == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    keep = np.concatenate(([True], v[1:] != v[:-1]))
    return pts[keep].astype(np.uint32), v[keep].astype(np.uint32)


def _one(start, end, extent, n_bins, window):
    pts, d = depth(start, end, extent)
    d = d.astype(np.int64)
    length = np.diff(np.concatenate((pts, np.asarray([extent], np.int64))))
    area = length * d
    hist = np.zeros(n_bins, np.int64)
    np.add.at(hist, np.minimum(d, n_bins - 1), length)
    win = None
    if window:
        n_windows = -(-extent // window)
        if extent:
            before = np.concatenate((np.zeros(1, np.int64), np.cumsum(area)))      # F(points[i])
            x = np.minimum(np.arange(n_windows + 1, dtype=np.int64) * window, extent)
            i = np.searchsorted(pts, x, side="right") - 1
            win = np.diff(before[i] + (x - pts[i]) * d[i]).astype(np.uint64)     # F: the integral of the depth, piecewise linear
        else:
            win = np.zeros(0, np.uint64)
    return hist.astype(np.uint64), int(area.sum()), win


def profile(raw, qc, extent, n_bins, window):
    """raw, qc: (start, end) of all reads and of those that pass the quality thresholds -> the dict of depth_ref.profile"""
    out = dict(n_bins=n_bins, window=window, extent=extent, n_windows=-(-extent // window) if window else 0)
    for k, (s, e) in (("raw", raw), ("qc", qc)):
        out["hist_" + k], out["sum_" + k], win = _one(s, e, extent, n_bins, window)
        if window:
            out["win_" + k] = win
    return out
