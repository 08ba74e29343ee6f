"""The independent reference of the consensus scan (include/callable_loci.h, cl_site_scan_consensus) and of the assembly
behind it (include/dut_variants.h, dut_cons_assemble): numpy and plain Python.  The counts come from the references of the
scans the rule composes -- scan_ref.stranded_hist for the bases, dels_ref.walk for the deletions, ins_ref for the
insertions -- and the rule and the assembler are written here from their description.  It shares no code with the library.

    a, c, g, t, depth  the filtered scan's counters, strands summed; depth over all 16 codes
    del                dels_ref's count, strands summed; span = depth + del
    m                  the largest of a, c, g, t, the first in that order among equals
    low_depth  n       span < min_depth
    deleted    -       del >= min_del_count and del / span >= per_10k / 10000
    low_depth  n       depth < min_depth
    ref / alt  ACGT    m / depth >= 7 / 10; ref iff the base equals the upper-cased reference byte
    no_call    N       everything else
"""
from fractions import Fraction

import numpy as np

import dels_ref as D
import ins_ref as I
import scan_ref as S

LOW_DEPTH, DELETED, NO_CALL, REF, ALT = range(5)
NAMES = ("low_depth", "deleted", "no_call", "ref", "alt")


def classify(a, c, g, t, depth, n_del, ref_byte, min_depth, min_del_count, per_10k):
    """(class, byte as a str) of one position, in exact fractions."""
    a, c, g, t, depth, n_del = (int(x) for x in (a, c, g, t, depth, n_del))
    span = depth + n_del
    if span < min_depth:
        return LOW_DEPTH, "n"
    if n_del >= min_del_count and Fraction(n_del, span) >= Fraction(per_10k, 10000):
        return DELETED, "-"
    if depth < min_depth:
        return LOW_DEPTH, "n"
    m = max(a, c, g, t)
    base = "ACGT"[min(i for i, v in enumerate((a, c, g, t)) if v == m)]        # the first among equals
    if Fraction(m, depth) >= Fraction(7, 10):
        return (REF if base == chr(ref_byte & 0xDF) else ALT), base
    return NO_CALL, "N"


def counts(L, ref_len, rec, min_quality, exclude_flags=0, min_base_quality=None):
    """(acgt (L, 4), depth (L,), del (L,)) as int64."""
    h2 = S.stranded_hist(L, ref_len, rec, min_quality, exclude_flags, min_base_quality)
    both = h2[0].astype(np.int64) + h2[1]
    _depth, dels = D.walk(L, ref_len, rec, min_quality, exclude_flags, min_base_quality)
    return both[:, S.ACGT_CODES], both.sum(1), dels.sum(0)


def reduce(acgt, depth, n_del, ref, L, min_depth, min_del_count, per_10k, start, end):
    """The bytes and class counts of [start, end): dict(cons=uint8 array, counts=(low_depth, deleted, no_call, ref, alt),
    cls=int array).  Whole columns at once, in exact int64 cross-multiplication (every product is below 2^63); held against
    classify() count by count in tests/test_cons_host.py."""
    refb = np.full(L, ord("N"), np.uint8)
    refb[:min(ref.shape[0], L)] = ref[:L]
    rb = refb[start:end] & np.uint8(0xDF)
    q = acgt[start:end].astype(np.int64)
    dp, dl = depth[start:end].astype(np.int64), n_del[start:end].astype(np.int64)
    span = dp + dl
    m = q.max(1) if end > start else np.zeros(0, np.int64)
    base = np.frombuffer(b"ACGT", np.uint8)[q.argmax(1)] if end > start else np.zeros(0, np.uint8)      # argmax: the first among equals
    low1 = span < min_depth
    deleted = ~low1 & (dl >= min_del_count) & (10000 * dl >= per_10k * span)
    low2 = ~low1 & ~deleted & (dp < min_depth)
    called = ~low1 & ~deleted & ~low2 & (10 * m >= 7 * dp)
    cls = np.select([low1 | low2, deleted, called & (base == rb), called], [LOW_DEPTH, DELETED, REF, ALT], NO_CALL)
    cons = np.select([cls == LOW_DEPTH, cls == DELETED, cls == NO_CALL], [ord("n"), ord("-"), ord("N")], base.astype(np.int64)).astype(np.uint8)
    n = tuple(int((cls == k).sum()) for k in range(5))
    assert sum(n) == max(end - start, 0)
    return dict(cons=cons, counts=n, cls=cls)


def insertions(L, ref_len, rec, ref, min_quality, exclude_flags, min_base_quality, min_depth, min_ins_count, per_10k, start, end):
    """[(pos 1-based, depth, alleles of the position, the top one first)] for the positions ins_ref calls in [start, end)."""
    depth, ins, events = I.walk(L, ref_len, rec, min_quality, exclude_flags, min_base_quality)
    exp = I.reduce(depth, ins, ref, L, min_depth, min_ins_count, per_10k, start, end)
    by_pos = {}
    for a in I.alleles(I.observations(events, rec, exp["candidates"])):
        by_pos.setdefault(a["pos"], []).append(a)
    return [(c[0], c[3], by_pos[c[0]]) for c in exp["candidates"]]


def assemble(cons, ref, start, ins=(), min_ins_count=3, ins_per_10k=7000, fill="N"):
    """(sequence, changes) of the bytes `cons` of [start, start + len(cons)).  ref: the whole reference; ins: what
    insertions() returns.  A change: (pos, end, kind, ref, cons, count, depth, note), count and depth None unless an
    insertion, note '' unless a skipped one."""
    text = bytes(cons).decode()
    n = len(text)

    def ref_at(i):
        p = start + i
        return chr(ref[p]) if p < len(ref) else "N"

    ins_at = {pos: (depth, al) for pos, depth, al in ins}
    seq, changes = [], []
    i = 0
    while i < n:
        b = text[i]
        if b == "-" and (i == 0 or text[i - 1] != "-"):
            j = i
            while j + 1 < n and text[j + 1] == "-":
                j += 1
            gone = "".join(ref_at(k).upper() for k in range(i, j + 1))
            changes.append((start + i + 1, start + j + 1, "del", gone if len(gone) <= 64 else ".", "-", None, None, ""))
        if b == "N":
            seq.append("N")
        elif b == "n":
            r = ref_at(i).lower()
            seq.append(r if fill == "ref" and r in "acgt" else "N")
        elif b in "ACGT":
            seq.append(b)
            if ref_at(i).upper() != b:
                changes.append((start + i + 1, start + i + 1, "snv", ref_at(i).upper(), b, None, None, ""))
        else:
            assert b == "-", b
        pos = start + i + 1
        if pos in ins_at:
            depth, al = ins_at[pos]
            top = al[0]
            what = "".join(k if k in "ACGT" else "N" for k in top["seq"])
            if b == "-":
                note = "anchor_deleted"
            elif top["len"] > 32:
                note = "too_long"
            elif not (top["count"] >= min_ins_count and Fraction(top["count"], depth) >= Fraction(ins_per_10k, 10000)):
                note = "no_allele"
            else:
                note = ""
                seq.append(what)
            changes.append((pos, pos, "ins_skipped" if note else "ins", ref_at(i).upper(), what, top["count"], depth, note))
        i += 1
    return "".join(seq), changes


def expected_fasta(contig, seq, start, end, whole, width=60):
    head = f">{contig}" if whole else f">{contig}:{start + 1}-{end}"
    return "\n".join([head] + [seq[k:k + width] for k in range(0, len(seq), width)]) + "\n"


def expected_changes(contig, n, seq, changes, a, b, md, mq, mbq, exclude_flags, del_per_10k, del_count, ins_per_10k, ins_count, fill):
    """The change list's file for the class counts n, the sequence and assemble()'s changes."""
    def frac(v):
        return f"{v // 10000}.{v % 10000:04d}"
    out = [f"##contig={contig}", f"##range={a}-{b}", f"##min_depth={md}", f"##min_quality={mq}",
           f"##min_base_quality={'.' if mbq is None else mbq}", f"##exclude_flags=0x{exclude_flags:04x}",
           f"##min_del_fraction={frac(del_per_10k)}", f"##min_del_count={del_count}", f"##min_ins_fraction={frac(ins_per_10k)}",
           f"##min_ins_count={ins_count}", f"##fill={fill}", f"##positions={b - a}"]
    out += [f"##{name}={v}" for name, v in zip(NAMES, n)]
    out += [f"##length={len(seq)}", f"##deletions={sum(c[2] == 'del' for c in changes)}", f"##insertions={sum(c[2] == 'ins' for c in changes)}",
            f"##insertions_skipped={sum(c[2] == 'ins_skipped' for c in changes)}", "#contig\tpos\tend\tkind\tref\tcons\tcount\tdepth\tnote"]
    for pos, end, kind, r, c, count, depth, note in changes:
        out.append(f"{contig}\t{pos}\t{end}\t{kind}\t{r}\t{c}\t{'.' if count is None else count}\t{'.' if depth is None else depth}\t{note or '.'}")
    return "\n".join(out) + "\n"
