"""The independent reference of the insertion scan (include/callable_loci.h, cl_site_scan_ins): a plain Python walk of a
ContigRecords, read by read and CIGAR operation by CIGAR operation, written from the rule.  It shares no code with the
library.

    a read counts      iff 0 <= pos < contig_len, mapq >= min_quality and (flag & exclude_flags) == 0
    depth[p]           bases of M / = / X operations at p: query index < l_seq, p < min(contig_len, ref_len), and (no
                       base-quality filter, or the base has no quality value, or that value is >= min_base_quality)
    ins[p]             I operations (op 1) anchored at p = x - 1, x = the reference position the walk has reached, that
                       count: the operation directly before is M / = / X (of at least one base: a match without a base has
                       no last base), the anchor base exists (query index y - 1 < l_seq, y = the query bases consumed
                       before the I), all inserted bases exist (y + len <= l_seq), p < min(contig_len, ref_len), and under
                       a base-quality filter the anchor base has no quality value or one >= min_base_quality
    strand             reverse iff flag & 0x10
    low_depth          depth < min_depth
    inserted           not low, ins >= min_count and ins / depth >= per_10k / 10000   (fractions.Fraction, never a float)
    kept               everything else
    observation        per counting insertion at a position of class inserted: (pos 1-based, len, key0, key1, strand);
                       the key holds the first min(len, 32) inserted 4-bit codes, base j in key[j // 16] at bits
                       60 - 4 * (j % 16)
    allele             the observations of a position with equal (len, key0, key1); the top allele has the most
                       observations, then the smaller len, then the smaller key
"""
from fractions import Fraction

import numpy as np

LOW_DEPTH, KEPT, INSERTED = 0, 1, 2
CODES = "=ACMGRSVTWYHKDBN"


def walk(L, ref_len, rec, min_quality, exclude_flags=0, min_base_quality=None):
    """(depth, ins, events): two (2, L) int64 arrays, [0] forward, [1] reverse, and per counting insertion
    (p 0-based, len, index of its first base in the numbering of seq_off, reverse).  min_base_quality=None: no
    base-quality filter."""
    depth = np.zeros((2, L), np.int64)
    ins = np.zeros((2, L), np.int64)
    events = []
    hi = min(L, int(ref_len))
    for r in range(rec.n):
        pos = int(rec.pos[r])
        if pos < 0 or pos >= L or int(rec.mapq[r]) < min_quality or (int(rec.flag[r]) & exclude_flags):
            continue
        strand = 1 if int(rec.flag[r]) & 0x10 else 0
        s0 = int(rec.seq_off[r])
        l_seq = int(rec.seq_off[r + 1]) - s0
        q0 = int(rec.qual_off[r])
        n_qual = int(rec.qual_off[r + 1]) - q0

        def passes(qi):
            return min_base_quality is None or qi >= n_qual or int(rec.qual[q0 + qi]) >= min_base_quality

        x, y = pos, 0
        before = None                                                    # the operation directly before: (op, length)
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
            elif op == 1:
                p = x - 1
                if (before is not None and before[0] in (0, 7, 8) and before[1] >= 1 and y - 1 < l_seq and y + l <= l_seq and p < hi
                        and passes(y - 1)):
                    ins[strand, p] += 1
                    events.append((p, l, s0 + y, strand))
                y += l
            elif op == 4:
                y += l
            elif op in (2, 3):
                x += l
            before = (op, l)
    return depth, ins, events


def classify(n_ins, depth, min_depth, min_count, per_10k):
    """The class of one position."""
    n_ins, depth = int(n_ins), int(depth)
    if depth < min_depth:
        return LOW_DEPTH
    if n_ins >= min_count and depth > 0 and Fraction(n_ins, depth) >= Fraction(per_10k, 10000):
        return INSERTED
    return KEPT


def reduce(depth, ins, ref, L, min_depth, min_count, per_10k, start, end, stranded=True):
    """Classes and candidates of [start, end) from walk()'s arrays.  A candidate: (pos 1-based, ref, ins, depth, ins_fwd,
    ins_rev, depth_fwd, depth_rev); stranded=False: the four strand counts are 0, as in the unfiltered form."""
    refb = np.full(L, ord("N"), np.uint8)
    refb[:min(ref.shape[0], L)] = ref[:L]
    refb &= np.uint8(0xDF)
    n = [0, 0, 0]
    cls = np.zeros(max(end - start, 0), np.int64)
    cand = []
    memo = {}                                                            # (ins, depth) -> class: the rule is taken once per pair
    for p in range(start, end):
        df, dr, nf, nr = int(depth[0, p]), int(depth[1, p]), int(ins[0, p]), int(ins[1, p])
        key = (nf + nr, df + dr)
        if key not in memo:
            memo[key] = classify(nf + nr, df + dr, min_depth, min_count, per_10k)
        k = memo[key]
        n[k] += 1
        cls[p - start] = k
        if k == INSERTED:
            cand.append((p + 1, chr(refb[p]), nf + nr, df + dr) + ((nf, nr, df, dr) if stranded else (0, 0, 0, 0)))
    assert sum(n) == max(end - start, 0)
    return dict(low_depth=n[LOW_DEPTH], kept=n[KEPT], inserted=n[INSERTED], candidates=cand, cls=cls)


def base_code(rec, i):
    """The 4-bit code of base i in the numbering of seq_off: two per byte of seq4, the even one in the high nibble."""
    byte = int(rec.seq4[i >> 1])
    return (byte & 15) if i & 1 else (byte >> 4)


def make_key(codes):
    """(key0, key1) of a sequence of 4-bit codes: the first 32 of them."""
    key = [0, 0]
    for j, c in enumerate(codes[:32]):
        key[j // 16] |= int(c) << (60 - 4 * (j % 16))
    return key[0], key[1]


def observations(events, rec, candidates, stranded=True):
    """One (pos 1-based, len, key0, key1, strand) per event of walk() at a candidate's position, sorted; stranded=False:
    strand is 0, as in the unfiltered form."""
    at = {c[0] for c in candidates}
    out = []
    for p, l, first, strand in events:
        if p + 1 in at:
            out.append((p + 1, l) + make_key([base_code(rec, first + j) for j in range(min(l, 32))]) + (strand if stranded else 0,))
    return sorted(out)


def key_text(length, key0, key1):
    return "".join(CODES[((key0, key1)[j // 16] >> (60 - 4 * (j % 16))) & 15] for j in range(min(length, 32)))


def alleles(obs):
    """The alleles of every position, as dicts (pos, len, key, seq, count, fwd, rev): ascending position; within a position
    the top allele first, the others behind it by (len, key)."""
    by_pos = {}
    for pos, l, k0, k1, strand in obs:
        a = by_pos.setdefault(pos, {}).setdefault((l, k0, k1), [0, 0])
        a[1 if strand else 0] += 1
    out = []
    for pos in sorted(by_pos):
        rest = sorted(by_pos[pos])
        top = min(rest, key=lambda k: (-sum(by_pos[pos][k]), k))
        rest.remove(top)
        for l, k0, k1 in [top] + rest:
            f, r = by_pos[pos][(l, k0, k1)]
            out.append(dict(pos=pos, len=l, key=(k0, k1), seq=key_text(l, k0, k1), count=f + r, fwd=f, rev=r))
    return out


def expected_tsv(contig, exp, obs, a, b, md, mq, mbq, exclude_flags, per_10k, min_count, k):
    """The TSV of find-insertions for reduce()'s result and its observations."""
    al = {}
    for x in alleles(obs):
        al.setdefault(x["pos"], []).append(x)
    out = [f"##contig={contig}", f"##range={a}-{b}", f"##min_depth={md}", f"##min_quality={mq}",
           f"##min_base_quality={'.' if mbq is None else mbq}", f"##exclude_flags=0x{exclude_flags:04x}",
           f"##min_ins_fraction={per_10k // 10000}.{per_10k % 10000:04d}", f"##min_ins_count={min_count}", f"##positions={b - a}",
           f"##low_depth={exp['low_depth']}", f"##kept={exp['kept']}", f"##inserted={exp['inserted']}",
           "#contig\tpos\tref\tins\tdepth\tfreq\talleles\tlength\tseq\tallele_count\tallele_fwd\tallele_rev\tins_fwd\tins_rev\tfilter"]
    for pos, ref, n_ins, depth, nf, nr, _df, _dr in exp["candidates"]:
        top = al[pos][0]
        seq = top["seq"] + ("..." if top["len"] > 32 else "")
        out.append(f"{contig}\t{pos}\t{ref}\t{n_ins}\t{depth}\t{n_ins / depth:.4f}\t{len(al[pos])}\t{top['len']}\t{seq}\t{top['count']}\t{top['fwd']}\t"
                   f"{top['rev']}\t{nf}\t{nr}\t{'strand' if min(nf, nr) < k else 'PASS'}")
    return "\n".join(out) + "\n"
