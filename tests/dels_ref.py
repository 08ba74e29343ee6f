"""The independent reference of the deletion scan (include/callable_loci.h, cl_site_scan_dels): a plain Python walk of a
ContigRecords, read by read and CIGAR operation by CIGAR operation, written from the rule.  It shares no code with the
library.

    a read counts      iff 0 <= pos < contig_len, mapq >= min_quality and (flag & exclude_flags) == 0
    depth[p]           bases of M / = / X operations at p: query index < l_seq, p < min(contig_len, ref_len), and (no
                       base-quality filter, or the base has no quality value, or that value is >= min_base_quality)
    del[p]             reads with a D operation (op 2, never N) over p, p < min(contig_len, ref_len), whose carrier exists:
                       query index y - 1 with y = the query bases consumed before the operation, 1 <= y <= l_seq; under a
                       base-quality filter the carrier has no quality value or one >= min_base_quality
    strand             reverse iff flag & 0x10
    span               depth + del, strands summed
    low_depth          span < min_depth
    deleted            not low, del >= min_count and del / span >= per_10k / 10000   (fractions.Fraction, never a float)
    kept               everything else
"""
from fractions import Fraction

import numpy as np

LOW_DEPTH, KEPT, DELETED = 0, 1, 2


def walk(L, ref_len, rec, min_quality, exclude_flags=0, min_base_quality=None):
    """(depth, dels): two (2, L) int64 arrays, [0] forward, [1] reverse.  min_base_quality=None: no base-quality filter."""
    depth = np.zeros((2, L), np.int64)
    dels = np.zeros((2, L), np.int64)
    hi = min(L, int(ref_len))
    for r in range(rec.n):
        pos = int(rec.pos[r])
        if pos < 0 or pos >= L or int(rec.mapq[r]) < min_quality or (int(rec.flag[r]) & exclude_flags):
            continue
        strand = 1 if int(rec.flag[r]) & 0x10 else 0
        l_seq = int(rec.seq_off[r + 1]) - int(rec.seq_off[r])
        q0 = int(rec.qual_off[r])
        n_qual = int(rec.qual_off[r + 1]) - q0

        def passes(qi):
            return min_base_quality is None or qi >= n_qual or int(rec.qual[q0 + qi]) >= min_base_quality

        x, y = pos, 0
        for w in rec.cigar[int(rec.cigar_off[r]):int(rec.cigar_off[r + 1])].tolist():
            op, l = w & 15, w >> 4
            if op in (0, 7, 8):
                n = max(0, min(l, l_seq - y, hi - x))                 # query index < l_seq, position < ref_len (and < L)
                if n > 0 and min_base_quality is None:
                    depth[strand, x:x + n] += 1
                elif n > 0:
                    ok = np.ones(n, np.int64)
                    nq = max(0, min(n, n_qual - y))                   # the bases of this run that have a quality value
                    if nq > 0:
                        ok[:nq] = rec.qual[q0 + y:q0 + y + nq] >= min_base_quality
                    depth[strand, x:x + n] += ok
                x += l; y += l
            elif op == 2:
                if 1 <= y <= l_seq and passes(y - 1):
                    dels[strand, x:max(x, min(x + l, hi))] += 1
                x += l
            elif op == 3:
                x += l
            elif op in (1, 4):
                y += l
            if x >= hi:
                break
    return depth, dels


def classify(n_del, depth, min_depth, min_count, per_10k):
    """The class of one position."""
    n_del, depth = int(n_del), int(depth)
    span = n_del + depth
    if span < min_depth:
        return LOW_DEPTH
    if n_del >= min_count and Fraction(n_del, span) >= Fraction(per_10k, 10000):
        return DELETED
    return KEPT


def reduce(depth, dels, ref, L, min_depth, min_count, per_10k, start, end, stranded=True):
    """Classes and candidates of [start, end) from walk()'s arrays.  A candidate: (pos 1-based, ref, del, depth, del_fwd,
    del_rev, depth_fwd, depth_rev); stranded=False: the four strand counts are 0, as in the unfiltered form."""
    refb = np.full(L, ord("N"), np.uint8)
    refb[:min(ref.shape[0], L)] = ref[:L]
    refb &= np.uint8(0xDF)
    n = [0, 0, 0]
    cls = np.zeros(max(end - start, 0), np.int64)
    cand = []
    memo = {}                                                            # (del, depth) -> class: the rule is taken once per pair
    for p in range(start, end):
        df, dr, lf, lr = int(depth[0, p]), int(depth[1, p]), int(dels[0, p]), int(dels[1, p])
        key = (lf + lr, df + dr)
        if key not in memo:
            memo[key] = classify(lf + lr, df + dr, min_depth, min_count, per_10k)
        k = memo[key]
        n[k] += 1
        cls[p - start] = k
        if k == DELETED:
            cand.append((p + 1, chr(refb[p]), lf + lr, df + dr) + ((lf, lr, df, dr) if stranded else (0, 0, 0, 0)))
    assert sum(n) == max(end - start, 0)
    return dict(low_depth=n[LOW_DEPTH], kept=n[KEPT], deleted=n[DELETED], candidates=cand, cls=cls)


def events(cand):
    """Maximal runs of consecutive candidate positions.  An event: dict(start, end, length, ref, q, del, span, del_fwd,
    del_rev, max_del); q = the position of the run's smallest del, the first among equals."""
    out, run = [], []

    def close():
        if run:
            q = min(run, key=lambda c: (c[2], c[0]))
            out.append({"start": run[0][0], "end": run[-1][0], "length": len(run), "ref": "".join(c[1] for c in run), "q": q[0],
                        "del": q[2], "span": q[2] + q[3], "del_fwd": q[4], "del_rev": q[5], "max_del": max(c[2] for c in run)})
            run.clear()

    for c in cand:
        if run and c[0] != run[-1][0] + 1:
            close()
        run.append(c)
    close()
    return out


def expected_tsv(contig, exp, a, b, md, mq, mbq, exclude_flags, per_10k, min_count, k):
    """The TSV of find-deletions for reduce()'s result."""
    ev = events(exp["candidates"])
    out = [f"##contig={contig}", f"##range={a}-{b}", f"##min_depth={md}", f"##min_quality={mq}",
           f"##min_base_quality={'.' if mbq is None else mbq}", f"##exclude_flags=0x{exclude_flags:04x}",
           f"##min_del_fraction={per_10k // 10000}.{per_10k % 10000:04d}", f"##min_del_count={min_count}", f"##positions={b - a}",
           f"##low_depth={exp['low_depth']}", f"##kept={exp['kept']}", f"##deleted={exp['deleted']}", f"##events={len(ev)}",
           "#contig\tstart\tend\tlength\tref\tdel\tspan\tfreq\tmax_del\tdel_fwd\tdel_rev\tfilter"]
    for e in ev:
        ref = e["ref"] if e["length"] <= 64 else "."
        out.append(f"{contig}\t{e['start']}\t{e['end']}\t{e['length']}\t{ref}\t{e['del']}\t{e['span']}\t{e['del'] / e['span']:.4f}\t{e['max_del']}\t"
                   f"{e['del_fwd']}\t{e['del_rev']}\t{'strand' if min(e['del_fwd'], e['del_rev']) < k else 'PASS'}")
    return "\n".join(out) + "\n"
