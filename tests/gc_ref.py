"""The GC-bias profile's contract, restated in numpy from per-position arrays and reference bytes
(include/callable_loci.h: cl_contig_gc_bias; include/dut_coverage.h: dut_gc_bias_add, dut_gc_bias_stats and the two text
files).  Nothing here calls the library."""
from decimal import Decimal

import numpy as np

BINS = 101
IS_GC = np.zeros(256, np.int64)
IS_AT = np.zeros(256, np.int64)
for _c in b"GCgc":
    IS_GC[_c] = 1
for _c in b"ATat":
    IS_AT[_c] = 1
IS_INVALID = 1 - IS_GC - IS_AT
for _a in (IS_GC, IS_AT, IS_INVALID):
    _a.setflags(write=False)


def as_bytes(ref):
    if ref is None:
        return np.zeros(0, np.uint8)
    if isinstance(ref, (bytes, bytearray)):
        return np.frombuffer(bytes(ref), np.uint8)
    return np.asarray(ref, np.uint8).reshape(-1)


def bit_words(ref, n_words):
    """the two planes of cl_debug_gc_bits: bit i of word w <-> position 64 w + i; beyond the bases both bits are 0"""
    ref = as_bytes(ref)[:64 * n_words]
    gc = np.zeros(64 * n_words, np.uint8)
    va = np.zeros(64 * n_words, np.uint8)
    gc[:len(ref)] = IS_GC[ref]
    va[:len(ref)] = 1 - IS_INVALID[ref]
    pack = lambda b: np.packbits(b, bitorder="little").view("<u8").astype(np.uint64)   # noqa: E731
    return pack(gc), pack(va)


def window_counts(ref, extent, window):
    """g[p], v[p] for p in [0, extent): GC and invalid bases in [p - window // 2, p - window // 2 + window); positions
    below 0 and at or beyond len(ref) are invalid"""
    ref = as_bytes(ref)
    before = window // 2
    lo_pad, n = before, extent + window                       # classes of the positions [-before, extent + window - before)
    gc = np.zeros(n, np.int64)
    inv = np.ones(n, np.int64)
    have = max(0, min(len(ref), n - lo_pad))
    gc[lo_pad:lo_pad + have] = IS_GC[ref[:have]]
    inv[lo_pad:lo_pad + have] = IS_INVALID[ref[:have]]
    cg = np.concatenate(([0], np.cumsum(gc)))
    ci = np.concatenate(([0], np.cumsum(inv)))
    p = np.arange(extent)
    return cg[p + window] - cg[p], ci[p + window] - ci[p]


def profile(raw, qc, ref, window, max_invalid):
    """raw, qc: per-position depths of [0, extent)"""
    raw = np.asarray(raw, np.uint64)
    qc = np.asarray(qc, np.uint64)
    extent = raw.shape[0]
    g, v = window_counts(ref, extent, window)
    counted = v <= max_invalid
    b = (100 * g[counted]) // (window - v[counted])
    assert b.size == 0 or (0 <= b.min() and b.max() <= 100)
    r, q = raw[counted], qc[counted]
    # (weights are exact in f64 here: a sum stays far below 2^53; the tests' depths are small)
    assert float(raw.sum()) < 2 ** 52
    out = dict(window=window, max_invalid=max_invalid, extent=extent, n_skipped=int(extent - counted.sum()),
               positions=np.bincount(b, minlength=BINS).astype(np.uint64),
               sum_raw=np.bincount(b, weights=r.astype(np.float64), minlength=BINS).astype(np.uint64),
               sum_qc=np.bincount(b, weights=q.astype(np.float64), minlength=BINS).astype(np.uint64),
               zero_raw=np.bincount(b[r == 0], minlength=BINS).astype(np.uint64))
    return out


def as_dict(g):
    """a GcBias of the package, or a dict, as a dict of the compared fields"""
    if isinstance(g, dict):
        return g
    return dict(window=g.window, max_invalid=g.max_invalid, extent=g.extent, n_skipped=g.n_skipped, positions=g.positions,
                sum_raw=g.sum_raw, sum_qc=g.sum_qc, zero_raw=g.zero_raw)


def same(got, exp, what=""):
    got, exp = as_dict(got), as_dict(exp)
    for k in ("window", "max_invalid", "extent", "n_skipped"):
        assert int(got[k]) == int(exp[k]), (what, k, int(got[k]), int(exp[k]))
    wrong = {}
    for k in ("positions", "sum_raw", "sum_qc", "zero_raw"):
        a, b = np.asarray(got[k], np.uint64), np.asarray(exp[k], np.uint64)
        bad = np.flatnonzero(a != b)
        if bad.size:
            wrong[k] = [(int(i), int(a[i]), int(b[i])) for i in bad[:5]]       # (bin, got, expected)
    assert not wrong, (what, wrong)


def add(total, part):
    """dut_gc_bias_add on dicts; None: a zeroed total"""
    part = as_dict(part)
    if total is None:
        total = dict(window=part["window"], max_invalid=part["max_invalid"], extent=0, n_skipped=0,
                     **{k: np.zeros(BINS, np.uint64) for k in ("positions", "sum_raw", "sum_qc", "zero_raw")})
    assert (total["window"], total["max_invalid"]) == (part["window"], part["max_invalid"])
    out = dict(total)
    out["extent"] = min(total["extent"] + part["extent"], 0xFFFFFFFF)
    out["n_skipped"] = total["n_skipped"] + part["n_skipped"]
    for k in ("positions", "sum_raw", "sum_qc", "zero_raw"):
        out[k] = np.asarray(total[k], np.uint64) + np.asarray(part[k], np.uint64)
    return out


def stats(g):
    """dut_gc_bias_stats in the header's operation order, in Python floats (f64); None = not available"""
    g = as_dict(g)
    pos = [int(x) for x in g["positions"]]
    sr = [int(x) for x in g["sum_raw"]]
    sq = [int(x) for x in g["sum_qc"]]
    zr = [int(x) for x in g["zero_raw"]]
    P, Sr, Sq = sum(pos), sum(sr), sum(sq)
    quot = lambda a, b: float(a) / float(b) if b else None    # noqa: E731
    out = dict(positions=P, sum_raw=Sr, sum_qc=Sq, total_mean_raw=quot(Sr, P), total_mean_qc=quot(Sq, P))
    out["mean_raw"] = [quot(sr[b], pos[b]) for b in range(BINS)]
    out["mean_qc"] = [quot(sq[b], pos[b]) for b in range(BINS)]
    out["zero_frac"] = [quot(zr[b], pos[b]) for b in range(BINS)]
    out["norm_raw"] = [out["mean_raw"][b] / out["total_mean_raw"] if pos[b] and Sr else None for b in range(BINS)]
    out["norm_qc"] = [out["mean_qc"][b] / out["total_mean_qc"] if pos[b] and Sq else None for b in range(BINS)]

    def dropout(s, S, b0, b1):
        if not P or not S:
            return None
        acc = 0.0
        for b in range(b0, b1):
            d = float(pos[b]) / float(P) - float(s[b]) / float(S)
            if d > 0.0:
                acc += d
        return 100.0 * acc
    out["at_dropout_raw"], out["gc_dropout_raw"] = dropout(sr, Sr, 0, 51), dropout(sr, Sr, 51, BINS)
    out["at_dropout_qc"], out["gc_dropout_qc"] = dropout(sq, Sq, 0, 51), dropout(sq, Sq, 51, BINS)
    return out


def _f(fmt, v):
    return "NA" if v is None else fmt % v


BIAS_HEADER = "#contig\tgc\tpositions\tmean_raw\tmean_qc\tnorm_raw\tnorm_qc\tzero_frac\n"
SUMMARY_HEADER = ("#contig\twindow\tmax_invalid\tpositions\tskipped\tmean_raw\tmean_qc\tat_dropout_raw\tgc_dropout_raw\t"
                  "at_dropout_qc\tgc_dropout_qc\n")


def bias_lines(contig, g):
    g = as_dict(g)
    s = stats(g)
    out = []
    for b in range(BINS):
        if int(g["positions"][b]):
            out.append("\t".join([contig, str(b), str(int(g["positions"][b])), _f("%.4f", s["mean_raw"][b]), _f("%.4f", s["mean_qc"][b]),
                                  _f("%.6f", s["norm_raw"][b]), _f("%.6f", s["norm_qc"][b]), _f("%.6f", s["zero_frac"][b])]) + "\n")
    return "".join(out)


def summary_line(contig, g):
    g = as_dict(g)
    s = stats(g)
    return "\t".join([contig, str(int(g["window"])), str(int(g["max_invalid"])), str(s["positions"]), str(int(g["n_skipped"])),
                      _f("%.4f", s["total_mean_raw"]), _f("%.4f", s["total_mean_qc"])]
                     + [_f("%.6f", s[k]) for k in ("at_dropout_raw", "gc_dropout_raw", "at_dropout_qc", "gc_dropout_qc")]) + "\n"


def bias_text(contigs, total=True):
    """contigs: (name, record) in output order; the `total` block follows"""
    text, acc = BIAS_HEADER, None
    for name, g in contigs:
        text += bias_lines(name, g)
        acc = add(acc, g)
    if total and acc is not None:
        text += bias_lines("total", acc)
    return text


def summary_text(contigs, total=True):
    text, acc = SUMMARY_HEADER, None
    for name, g in contigs:
        text += summary_line(name, g)
        acc = add(acc, g)
    if total and acc is not None:
        text += summary_line("total", acc)
    return text


# which columns of a line are integers or names (compared exactly); the others are %.4f (1e-4) or %.6f (1e-6)
BIAS_TOL = (None, None, None, 1e-4, 1e-4, 1e-6, 1e-6, 1e-6)
SUMMARY_TOL = (None, None, None, None, None, 1e-4, 1e-4, 1e-6, 1e-6, 1e-6, 1e-6)


def same_text(got, exp, tol, what=""):
    """printed floats after parsing within one unit of their last printed digit (two correctly rounded printings of
    values an ulp apart differ by that at most); integer columns, names and NA exactly"""
    gl, el = got.split("\n"), exp.split("\n")
    assert len(gl) == len(el), (what, len(gl), len(el))
    assert gl[0] == el[0], (what, gl[0], el[0])
    for i, (a, b) in enumerate(zip(gl[1:], el[1:]), 1):
        if a == b:
            continue
        ca, cb = a.split("\t"), b.split("\t")
        assert len(ca) == len(cb) == len(tol), (what, i, a, b)
        for x, y, t in zip(ca, cb, tol):
            if t is None or x == "NA" or y == "NA":
                assert x == y, (what, i, a, b)
            else:
                # (as decimals: the difference of two printed numbers is exact)
                assert abs(Decimal(x) - Decimal(y)) <= Decimal(repr(t)), (what, i, a, b)
