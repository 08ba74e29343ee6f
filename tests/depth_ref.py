"""The depth profile's contract, restated in numpy from per-position arrays (include/callable_loci.h:
cl_contig_depth_profile; include/dut_coverage.h: dut_depth_stats and the three text files).  Nothing here calls the
library."""
import numpy as np

THRESHOLDS = (1, 5, 10, 15, 20, 30, 50, 100)


def profile(raw, qc, n_bins, window):
    """raw, qc: per-position depths of [0, extent).  hist[b] = positions with min(depth, n_bins - 1) == b; the sums are
    exact; win[i] = sum over [i * window, min((i + 1) * window, extent))."""
    raw = np.asarray(raw, np.uint64)
    qc = np.asarray(qc, np.uint64)
    extent = raw.shape[0]
    out = dict(n_bins=n_bins, window=window, extent=extent, sum_raw=int(raw.sum()), sum_qc=int(qc.sum()))
    for k, a in (("raw", raw), ("qc", qc)):
        out["hist_" + k] = np.bincount(np.minimum(a, n_bins - 1).astype(np.int64), minlength=n_bins).astype(np.uint64)
        if window:
            starts = np.arange(0, extent, window)
            out["win_" + k] = np.add.reduceat(a, starts).astype(np.uint64) if extent else np.zeros(0, np.uint64)
    out["n_windows"] = -(-extent // window) if window else 0
    return out


def pad(a, extent):
    """the oracle's dump ends at its last column; the engine classifies max(contig_len, last read end) positions"""
    out = np.zeros(extent, np.uint64)
    out[:len(a)] = a
    return out


def stats(hist, total):
    hist = [int(v) for v in hist]
    n_bins = len(hist)
    n = sum(hist)
    out = dict(positions=n, mean=(total / n if n else 0.0))
    for key, k in (("q1", 1), ("median", 2), ("q3", 3)):
        target = (n * k + 3) // 4                      # ceil(k / 4 * n)
        cum, d = 0, 0
        for d in range(n_bins):
            cum += hist[d]
            if cum >= target:
                break
        out[key] = (d, d == n_bins - 1) if n else (0, False)
    out["frac_at_least"] = {t: (None if t > n_bins - 1 else (sum(hist[t:]) / n if n else 0.0)) for t in THRESHOLDS}
    return out


def _entries(contigs):
    """contigs: [(name, profile)] in output order -> the same plus `total`"""
    n_bins = contigs[0][1]["n_bins"] if contigs else 0
    tot = dict(n_bins=n_bins, hist_raw=np.zeros(n_bins, np.uint64), hist_qc=np.zeros(n_bins, np.uint64), sum_raw=0, sum_qc=0)
    for _, p in contigs:
        tot["hist_raw"] = tot["hist_raw"] + p["hist_raw"]
        tot["hist_qc"] = tot["hist_qc"] + p["hist_qc"]
        tot["sum_raw"] += p["sum_raw"]
        tot["sum_qc"] += p["sum_qc"]
    return list(contigs) + [("total", tot)]


def dist_text(contigs):
    lines = ["#contig\tkind\tdepth\tpositions\tfraction_at_or_above"]
    for name, p in _entries(contigs):
        for kind in ("raw", "qc"):
            h = [int(v) for v in p["hist_" + kind]]
            n, below = sum(h), 0
            for b, v in enumerate(h):
                if v:
                    lines.append("%s\t%s\t%d%s\t%d\t%.6f" % (name, kind, b, "+" if b == len(h) - 1 else "", v, (n - below) / n))
                below += v
    return "\n".join(lines) + "\n"


def windows_text(contigs):
    lines = ["#contig\tstart\tend\tmean_raw\tmean_qc"]
    for name, p in contigs:
        for i in range(p["n_windows"]):
            s, e = i * p["window"], min((i + 1) * p["window"], p["extent"])
            lines.append("%s\t%d\t%d\t%.2f\t%.2f" % (name, s, e, int(p["win_raw"][i]) / (e - s), int(p["win_qc"][i]) / (e - s)))
    return "\n".join(lines) + "\n"


def summary_text(contigs):
    lines = ["#contig\tkind\tpositions\tsum\tmean\tq1\tmedian\tq3" + "".join("\tfrac_ge_%d" % t for t in THRESHOLDS)]
    for name, p in _entries(contigs):
        for kind in ("raw", "qc"):
            s = stats(p["hist_" + kind], p["sum_" + kind])
            q = ["%d%s" % (v, "+" if sat else "") for v, sat in (s["q1"], s["median"], s["q3"])]
            fr = ["NA" if s["frac_at_least"][t] is None else "%.6f" % s["frac_at_least"][t] for t in THRESHOLDS]
            lines.append("\t".join([name, kind, str(s["positions"]), str(p["sum_" + kind]), "%.4f" % s["mean"]] + q + fr))
    return "\n".join(lines) + "\n"
