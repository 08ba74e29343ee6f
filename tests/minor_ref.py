"""The independent reference of the minor-allele scan (include/callable_loci.h, cl_site_scan_minor): plain numpy and
Python integers on top of scan_ref.stranded_hist.  It shares no code with the library.

    A C G T      the counters of codes 1, 2, 4, 8, strands summed;  depth = all 16 codes, both strands
    major        the largest of A C G T, the first in that order among equals     (a stable argsort of the negated counts)
    minor        the largest of the other three, the first in that order among equals   (the second of that argsort)
    low_depth    depth < min_depth
    minor        not low, c2 >= min_minor_count and c2 / depth >= per_10k / 10000   (fractions.Fraction, never a float)
    single       everything else
"""
from fractions import Fraction

import numpy as np

LOW_DEPTH, SINGLE, MINOR = 0, 1, 2
ACGT = "ACGT"
ACGT_CODES = (1, 2, 4, 8)


def rank(acgt):
    """(major index, minor index) of four counts."""
    order = np.argsort(-np.asarray(acgt, np.int64), kind="stable")
    return int(order[0]), int(order[1])


def classify(a, c, g, t, depth, min_depth, min_count, per_10k):
    """(class, major, minor) of one position."""
    cnt = (int(a), int(c), int(g), int(t))
    mi, ni = rank(cnt)
    depth = int(depth)
    if depth < min_depth:
        return LOW_DEPTH, ACGT[mi], ACGT[ni]
    c2 = cnt[ni]
    if c2 >= min_count and Fraction(c2, depth) >= Fraction(per_10k, 10000):
        return MINOR, ACGT[mi], ACGT[ni]
    return SINGLE, ACGT[mi], ACGT[ni]


def classify_arrays(acgt, depth, min_depth, min_count, per_10k):
    """The rule over arrays, for many positions at once: acgt (n, 4) and depth (n,) as integers.  Returns (class, major
    index, minor index).  All in int64: 10000 * c2 and per_10k * depth stay below 2^63 for counts below 2^32."""
    acgt = np.asarray(acgt).astype(np.int64)
    depth = np.asarray(depth).astype(np.int64)
    order = np.argsort(-acgt, axis=1, kind="stable")
    mi, ni = order[:, 0], order[:, 1]
    c2 = np.take_along_axis(acgt, ni[:, None], 1)[:, 0]
    low = depth < min_depth
    minor = ~low & (c2 >= min_count) & (10000 * c2 >= per_10k * depth)
    return np.where(low, LOW_DEPTH, np.where(minor, MINOR, SINGLE)), mi, ni


def reduce(h2, ref, L, min_depth, min_count, per_10k, start, end, stranded=True):
    """Classes and candidates of [start, end) from stranded_hist's (2, L, 16).  A candidate: (pos 1-based, ref, major,
    minor, A, C, G, T, depth, major_fwd, major_rev, minor_fwd, minor_rev); stranded=False: the four strand counts are 0,
    as in the unfiltered form."""
    both = h2[0].astype(np.int64) + h2[1].astype(np.int64)
    depth = both.sum(1)
    acgt = both[:, ACGT_CODES]
    order = np.argsort(-acgt, axis=1, kind="stable")
    refb = np.full(L, ord("N"), np.uint8)
    refb[:min(ref.shape[0], L)] = ref[:L]
    refb &= np.uint8(0xDF)
    n = [0, 0, 0]
    cls = np.zeros(max(end - start, 0), np.int64)
    cand = []
    for p in range(start, end):
        mi, ni = int(order[p, 0]), int(order[p, 1])
        d, c2 = int(depth[p]), int(acgt[p, ni])
        if d < min_depth:
            k = LOW_DEPTH
        elif c2 >= min_count and Fraction(c2, d) >= Fraction(per_10k, 10000):
            k = MINOR
        else:
            k = SINGLE
        n[k] += 1
        cls[p - start] = k
        if k == MINOR:
            mc, nc = ACGT_CODES[mi], ACGT_CODES[ni]
            strands = (int(h2[0, p, mc]), int(h2[1, p, mc]), int(h2[0, p, nc]), int(h2[1, p, nc])) if stranded else (0, 0, 0, 0)
            cand.append((p + 1, chr(refb[p]), ACGT[mi], ACGT[ni]) + tuple(int(x) for x in acgt[p]) + (d,) + strands)
    assert sum(n) == max(end - start, 0)
    return dict(low_depth=n[LOW_DEPTH], single=n[SINGLE], minor=n[MINOR], candidates=cand, cls=cls)


def expected_tsv(contig, exp, a, b, md, mq, mbq, exclude_flags, per_10k, min_count, k):
    """The TSV of find-minor-alleles for reduce()'s result."""
    out = [f"##contig={contig}", f"##range={a}-{b}", f"##min_depth={md}", f"##min_quality={mq}",
           f"##min_base_quality={'.' if mbq is None else mbq}", f"##exclude_flags=0x{exclude_flags:04x}",
           f"##min_minor_fraction={per_10k // 10000}.{per_10k % 10000:04d}", f"##min_minor_count={min_count}", f"##positions={b - a}",
           f"##low_depth={exp['low_depth']}", f"##single={exp['single']}", f"##minor={exp['minor']}",
           "#contig\tpos\tref\tmajor\tminor\tdepth\tA\tC\tG\tT\tminor_freq\tmajor_fwd\tmajor_rev\tminor_fwd\tminor_rev\tfilter"]
    for pos, r, major, minor, A, C, G, T, depth, mf, mr, nf, nr in exp["candidates"]:
        freq = dict(A=A, C=C, G=G, T=T)[minor] / depth
        out.append(f"{contig}\t{pos}\t{r}\t{major}\t{minor}\t{depth}\t{A}\t{C}\t{G}\t{T}\t{freq:.4f}\t{mf}\t{mr}\t{nf}\t{nr}\t"
                   f"{'strand' if min(nf, nr) < k else 'PASS'}")
    return "\n".join(out) + "\n"
