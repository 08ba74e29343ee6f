"""The rule of cl_contig_targets (include/callable_loci.h) in numpy, over per-position arrays: raw[p], qc[p] and
state[p] for p < extent.  Prefix sums, so that thousands of targets cost one pass; held against a per-position Python
loop on tiny inputs in tests/test_targets_host.py."""
import numpy as np

STATE_COLUMNS = ("ref_n", "callable", "no_coverage", "low_coverage", "excessive_coverage", "poor_mapping_quality")
FIELDS = ("start", "end", "len", "sum_raw", "sum_qc", "state", "ge_raw", "ge_qc")


def clip(starts, ends, extent):
    e = np.minimum(np.asarray(ends, np.int64), extent)
    s = np.minimum(np.asarray(starts, np.int64), e)
    return s, e


def window_edge_targets(extent, w, T=2048):
    """(starts, ends) of five targets at the edges of the per-window rebuild of the depths, around engine window w >= 1
    (T positions) of a contig of `extent` positions: an empty one, one inside a single thread's 16 positions, one that
    starts on the window's first position, one that crosses the seam from window w - 1, one clipped by the extent"""
    W = w * T
    assert w >= 1 and W + 700 < extent
    return [W + 40, W + 18, W, W - 70, extent - 100], [W + 40, W + 30, W + 700, W + 80, extent + 5000]


def oracle_state(so, eo, engine_state, extent):
    """the oracle's states end at its last column eo: behind it the engine's own, up to the extent"""
    return np.concatenate((np.asarray(so[:eo], np.uint8), np.asarray(engine_state[eo:extent], np.uint8)))


def _cum(a):
    return np.concatenate(([0], np.cumsum(np.asarray(a, np.int64))))


def target_stats(raw, qc, state, starts, ends, thresholds):
    """raw, qc, state: one entry per position of [0, extent).  -> dict of arrays, one entry per target."""
    extent = len(raw)
    assert len(qc) == extent and len(state) == extent
    raw, qc, state = np.asarray(raw, np.int64), np.asarray(qc, np.int64), np.asarray(state, np.int64)
    s, e = clip(starts, ends, extent)
    n, k = len(s), len(thresholds)
    out = dict(start=s.astype(np.uint32), end=e.astype(np.uint32), len=(e - s).astype(np.uint32))
    c = _cum(raw); out["sum_raw"] = (c[e] - c[s]).astype(np.uint64)
    c = _cum(qc); out["sum_qc"] = (c[e] - c[s]).astype(np.uint64)
    out["state"] = np.zeros((n, 6), np.uint32)
    for st in range(6):
        c = _cum(state == st)
        out["state"][:, st] = c[e] - c[s]
    out["ge_raw"] = np.zeros((n, k), np.uint32)
    out["ge_qc"] = np.zeros((n, k), np.uint32)
    for j, t in enumerate(thresholds):
        c = _cum(raw >= t); out["ge_raw"][:, j] = c[e] - c[s]
        c = _cum(qc >= t); out["ge_qc"][:, j] = c[e] - c[s]
    return out


def target_stats_loop(raw, qc, state, starts, ends, thresholds):
    """the same, position by position"""
    extent = len(raw)
    n, k = len(starts), len(thresholds)
    out = dict(start=np.zeros(n, np.uint32), end=np.zeros(n, np.uint32), len=np.zeros(n, np.uint32), sum_raw=np.zeros(n, np.uint64),
               sum_qc=np.zeros(n, np.uint64), state=np.zeros((n, 6), np.uint32), ge_raw=np.zeros((n, k), np.uint32),
               ge_qc=np.zeros((n, k), np.uint32))
    for i in range(n):
        e = min(int(ends[i]), extent)
        s = min(int(starts[i]), e)
        out["start"][i], out["end"][i], out["len"][i] = s, e, e - s
        for p in range(s, e):
            out["sum_raw"][i] += int(raw[p]); out["sum_qc"][i] += int(qc[p])
            out["state"][i, int(state[p])] += 1
            for j, t in enumerate(thresholds):
                out["ge_raw"][i, j] += int(raw[p]) >= t
                out["ge_qc"][i, j] += int(qc[p]) >= t
    return out


def same(got, exp, what=""):
    """got: a TargetStats (or a dict of the same fields); exp: what target_stats gave"""
    for f in FIELDS:
        g = got[f] if isinstance(got, dict) else getattr(got, f)
        assert g.shape == exp[f].shape, (what, f, g.shape, exp[f].shape)
        bad = np.flatnonzero((np.asarray(g, np.uint64) != np.asarray(exp[f], np.uint64)).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, (what, f, bad[:5].tolist(), np.asarray(g)[bad[:5]].tolist(), np.asarray(exp[f])[bad[:5]].tolist())


def _fmt_line(head, length, sum_raw, sum_qc, state, ge_raw, ge_qc):
    cols = list(head) + [str(length)]
    cols += ["%.4f" % (sum_raw / length), "%.4f" % (sum_qc / length)] if length else ["NA", "NA"]
    cols += [str(state[1]), ("%.6f" % (state[1] / length)) if length else "NA"]
    cols += [str(state[0]), str(state[2]), str(state[3]), str(state[4]), str(state[5])]
    cols += [str(v) for v in ge_raw] + [str(v) for v in ge_qc]
    return "\t".join(cols) + "\n"


def table_text(contigs, thresholds):
    """contigs: (name, what target_stats gave, names) in output order -> the text of the per-target table"""
    head = ["#contig", "start", "end", "name", "length", "mean_raw", "mean_qc", "callable", "callable_frac", "ref_n", "no_coverage",
            "low_coverage", "excessive_coverage", "poor_mapping_quality"]
    head += ["raw_ge_%d" % t for t in thresholds] + ["qc_ge_%d" % t for t in thresholds]
    text = "\t".join(head) + "\n"
    k = len(thresholds)
    tot = dict(len=0, sum_raw=0, sum_qc=0, state=[0] * 6, ge_raw=[0] * k, ge_qc=[0] * k)
    for name, st, names in contigs:
        for i in range(len(st["len"])):
            row = dict(len=int(st["len"][i]), sum_raw=int(st["sum_raw"][i]), sum_qc=int(st["sum_qc"][i]), state=[int(v) for v in st["state"][i]],
                       ge_raw=[int(v) for v in st["ge_raw"][i]], ge_qc=[int(v) for v in st["ge_qc"][i]])
            text += _fmt_line([name, str(int(st["start"][i])), str(int(st["end"][i])), names[i]], row["len"], row["sum_raw"], row["sum_qc"],
                              row["state"], row["ge_raw"], row["ge_qc"])
            for f in ("len", "sum_raw", "sum_qc"):
                tot[f] += row[f]
            for f in ("state", "ge_raw", "ge_qc"):
                tot[f] = [a + b for a, b in zip(tot[f], row[f])]
    text += _fmt_line(["total", ".", ".", "."], tot["len"], tot["sum_raw"], tot["sum_qc"], tot["state"], tot["ge_raw"], tot["ge_qc"])
    return text
