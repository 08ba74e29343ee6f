"""An independent restatement of the short-tandem-repeat rule (cl_site_str_lengths, dut_str_call, dut_str_units and the TSV
of find-strs), written from the rule table of the README and not from csrc/str_walk.h: every read is first expanded into
its per-reference-position events -- the set of positions one of its M/=/X operations covers, the set one of its N
operations covers, and its I operations as (position they stand at, length) -- and a locus is then counted from those
sets, position by position.  No interval arithmetic is shared with the library."""
from fractions import Fraction

import numpy as np

BINS = 128
LOW_DEPTH, MIXED, CALLED = range(3)
STATUS = ("low_depth", "mixed", "called")


def expand(rec):
    """Per read: dict(match=set of matched positions, skip=set of N positions, ins=[(x, l)], lo, hi = the first reference
    position consumed and one past the last; lo == hi: no reference span)."""
    out = []
    for r in range(rec.n):
        x = int(rec.pos[r])
        lo = x
        match, skip, ins = set(), set(), []
        for k in range(int(rec.cigar_off[r]), int(rec.cigar_off[r + 1])):
            w = int(rec.cigar[k])
            op, l = "MIDNSHP=X"[w & 15] if (w & 15) < 9 else "?", w >> 4
            if op in "M=X":
                match.update(range(x, x + l)); x += l
            elif op == "I":
                ins.append((x, l))
            elif op == "D":
                x += l
            elif op == "N":
                skip.update(range(x, x + l)); x += l
        out.append(dict(match=match, skip=skip, ins=ins, lo=lo, hi=x))
    return out


def measure_read(ev, s, e, F):
    """(spanning, delta) of one expanded read over [s, e) with flank F."""
    qlen = sum(1 for p in range(s, e) if p in ev["match"])
    m_left = sum(1 for p in range(s - F, s) if p in ev["match"])          # (positions below 0 are never matched)
    m_right = sum(1 for p in range(e, e + F) if p in ev["match"])
    i_left = i_right = 0
    for x, l in ev["ins"]:
        if s <= x <= e:
            qlen += l
        elif s - F < x < s:
            i_left += l
        elif e < x < e + F:
            i_right += l
    skipped = any(p in ev["skip"] for p in range(s, e))
    return (m_left == F and m_right == F and i_left == 0 and i_right == 0 and not skipped), qlen - (e - s)


def measure(events, rec, contig_len, loci, flank, min_quality, exclude_flags=None, cache=None):
    """hist (n, strands, 128) and partial (n) of the loci [(s, e), ...]; exclude_flags=None: one strand, flags take no part.
    cache: a dict the caller keeps for one `events` list -- what a read measures over a locus depends on neither gate."""
    cache = {} if cache is None else cache
    strands = 1 if exclude_flags is None else 2
    hist = np.zeros((len(loci), strands, BINS), np.uint32)
    partial = np.zeros(len(loci), np.uint32)
    takes = [0 <= int(rec.pos[r]) < contig_len and int(rec.mapq[r]) >= min_quality and events[r]["hi"] > events[r]["lo"]
             and (exclude_flags is None or (int(rec.flag[r]) & exclude_flags) == 0) for r in range(rec.n)]
    for i, (s, e) in enumerate(loci):
        s, e = int(s), int(e)
        for r in range(rec.n):
            ev = events[r]
            if not takes[r] or not (ev["lo"] < e and ev["hi"] > s):
                continue
            key = (r, s, e, flank)
            if key not in cache:
                cache[key] = measure_read(ev, s, e, flank)
            spanning, delta = cache[key]
            if not spanning:
                partial[i] += 1
                continue
            rev = 0 if exclude_flags is None else (int(rec.flag[r]) >> 4) & 1
            hist[i, rev, delta + 63 if -63 <= delta <= 63 else BINS - 1] += 1
    return hist, partial


def call(hist_fwd, hist_rev, min_depth, min_allele_per_10k):
    """dict(status, n, other, delta, count, fwd, rev, delta2, count2) by exact fractions."""
    both = [int(hist_fwd[b]) + (int(hist_rev[b]) if hist_rev is not None else 0) for b in range(BINS)]
    n = sum(both)
    order = sorted(range(BINS - 1), key=lambda b: (-both[b], b))           # the fullest first, the smallest delta among equals
    top, second = order[0], order[1]
    if n < min_depth:
        status = LOW_DEPTH
    elif Fraction(both[top], n) >= Fraction(min_allele_per_10k, 10000):
        status = CALLED
    else:
        status = MIXED
    return dict(status=status, n=n, other=both[BINS - 1], delta=top - 63, count=both[top], fwd=int(hist_fwd[top]),
                rev=int(hist_rev[top]) if hist_rev is not None else 0, delta2=second - 63, count2=both[second])


def units(span, delta, period):
    whole, rest = divmod(span + delta, period)
    return f"{whole}.{rest}" if rest else f"{whole}"


def signed(delta):
    return f"{delta:+d}" if delta else "0"


def expected_tsv(contig, loci, skipped, hist, partial, flank, min_depth, min_quality, exclude_flags, min_allele_per_10k):
    """The bytes of find-strs for loci = dicts of start, end, period, name."""
    lines, n_class = [], [0, 0, 0]
    for i, l in enumerate(loci):
        c = call(hist[i, 0], hist[i, 1] if hist.shape[1] == 2 else None, min_depth, min_allele_per_10k)
        n_class[c["status"]] += 1
        span = l["end"] - l["start"]
        cols = [contig, l["start"], l["end"], l["name"], l["period"], units(span, 0, l["period"]), c["n"], int(partial[i]), c["other"], STATUS[c["status"]]]
        if c["status"] == LOW_DEPTH or c["count"] == 0:
            cols += ["."] * 6
        else:
            cols += [units(span, c["delta"], l["period"]), signed(c["delta"]), c["count"], "%.4f" % (c["count"] / c["n"]), c["fwd"], c["rev"]]
        cols += ["."] * 3 if c["count2"] == 0 else [units(span, c["delta2"], l["period"]), signed(c["delta2"]), c["count2"]]
        lines.append("\t".join(str(x) for x in cols) + "\n")
    head = (f"##contig={contig}\n##loci={len(loci)}\n##loci_skipped={skipped}\n##flank={flank}\n##min_depth={min_depth}\n##min_quality={min_quality}\n"
            f"##exclude_flags=0x{exclude_flags:04x}\n##min_allele_fraction={min_allele_per_10k / 10000:.4f}\n##low_depth={n_class[0]}\n##mixed={n_class[1]}\n"
            f"##called={n_class[2]}\n")
    return (head + "#contig\tstart\tend\tname\tperiod\tref_units\tspanning\tpartial\tother\tstatus\tallele\tdelta\tcount\tfreq\tfwd\trev\tallele2\tdelta2\tcount2\n"
            + "".join(lines))
