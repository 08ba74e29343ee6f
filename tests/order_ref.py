"""The rule of cl_contig_target_order (include/callable_loci.h) in numpy, over per-position arrays: raw[p] and qc[p] for
p < extent.  Per target the sorted slice and five of its elements; held against a per-position Python loop on tiny
inputs in tests/test_target_order_host.py."""
import numpy as np

import targets_ref

FIELDS = ("start", "end", "len", "raw", "qc")
ORDER_COLUMNS = ("raw_min", "raw_q1", "raw_median", "raw_q3", "raw_max", "qc_min", "qc_q1", "qc_median", "qc_q3", "qc_max")


def ranks(length):
    """the elements of the sorted depths that are min, q1, median, q3, max: q_j is the smallest v with
    #{d <= v} >= ceil(j * length / 4)"""
    return [0] + [(j * length + 3) // 4 - 1 for j in (1, 2, 3)] + [length - 1]


def target_order(raw, qc, starts, ends):
    """raw, qc: one entry per position of [0, extent).  -> dict of arrays, one entry per target."""
    extent = len(raw)
    assert len(qc) == extent
    raw, qc = np.asarray(raw, np.int64), np.asarray(qc, np.int64)
    s, e = targets_ref.clip(starts, ends, extent)
    n = len(s)
    out = dict(start=s.astype(np.uint32), end=e.astype(np.uint32), len=(e - s).astype(np.uint32),
               raw=np.zeros((n, 5), np.uint32), qc=np.zeros((n, 5), np.uint32))
    for i in range(n):
        length = int(e[i] - s[i])
        if length:
            r = ranks(length)
            out["raw"][i] = np.sort(raw[s[i]:e[i]])[r]
            out["qc"][i] = np.sort(qc[s[i]:e[i]])[r]
    return out


def target_order_loop(raw, qc, starts, ends):
    """the same, position by position with a Python sort per target, the quartiles by their definition"""
    extent = len(raw)
    n = len(starts)
    out = dict(start=np.zeros(n, np.uint32), end=np.zeros(n, np.uint32), len=np.zeros(n, np.uint32),
               raw=np.zeros((n, 5), np.uint32), qc=np.zeros((n, 5), np.uint32))
    for i in range(n):
        e = min(int(ends[i]), extent)
        s = min(int(starts[i]), e)
        out["start"][i], out["end"][i], out["len"][i] = s, e, e - s
        if e == s:
            continue
        for kind, arr in (("raw", raw), ("qc", qc)):
            d = sorted(int(arr[p]) for p in range(s, e))
            five = [d[0]]
            for j in (1, 2, 3):
                need = -(-j * (e - s) // 4)                      # ceil(j * len / 4)
                five.append(next(v for v in d if sum(1 for x in d if x <= v) >= need))
            five.append(d[-1])
            out[kind][i] = five
    return out


def same(got, exp, what=""):
    """got: a TargetOrder (or a dict of the same fields); exp: what target_order gave"""
    for f in FIELDS:
        g = got[f] if isinstance(got, dict) else getattr(got, f)
        assert g.shape == exp[f].shape, (what, f, g.shape, exp[f].shape)
        bad = np.flatnonzero((np.asarray(g, np.uint64) != np.asarray(exp[f], np.uint64)).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, (what, f, bad[:5].tolist(), np.asarray(g)[bad[:5]].tolist(), np.asarray(exp[f])[bad[:5]].tolist())


def table_text(contigs, thresholds):
    """contigs: (name, what targets_ref.target_stats gave, names, what target_order gave of the same targets) in output
    order -> the text of the per-target table with the ten order columns behind the others: whole numbers, `NA` for a
    target of length 0 and on the `total` line"""
    lines = targets_ref.table_text([(n, st, nm) for n, st, nm, _ in contigs], thresholds).splitlines()
    tail = ["\t".join(ORDER_COLUMNS)]
    for _, st, _, od in contigs:
        assert np.array_equal(st["start"], od["start"]) and np.array_equal(st["end"], od["end"])
        for i in range(len(od["len"])):
            five = [int(v) for v in od["raw"][i]] + [int(v) for v in od["qc"][i]]
            tail.append("\t".join(str(v) for v in five) if int(od["len"][i]) else "\t".join(["NA"] * 10))
    tail.append("\t".join(["NA"] * 10))
    assert len(tail) == len(lines)
    return "".join(a + "\t" + b + "\n" for a, b in zip(lines, tail))
