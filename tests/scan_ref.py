"""The independent reference of the filtered, strand-aware site scan (include/callable_loci.h, cl_site_scan_ex): plain
numpy, read by read and CIGAR operation by CIGAR operation, from a ContigRecords.  It shares no code with the library.

    a read counts   iff 0 <= pos < contig_len, mapq >= min_quality and (flag & exclude_flags) == 0
    a base counts   iff it lies in an M / = / X operation, its query index is < l_seq (the number of bases the read
                    has), its position is < ref_len, and (no base-quality filter, or the base has no quality value, or
                    that value is >= min_base_quality; 0xFF is >= every threshold)
    strand          reverse iff flag & 0x10

stranded_hist returns hist[strand][position][code] over the 16 BAM base codes; everything else is derived from it here,
with the f64 rule of the caller (largest / depth >= 0.7) as tests/test_gpu_variants.py::reduce_hist takes it."""
import numpy as np

CODE = "=ACMGRSVTWYHKDBN"
ACGT_CODES = np.array([1, 2, 4, 8])


def unpack_seq4(seq4, n_bases):
    s = np.asarray(seq4, np.uint8)
    out = np.empty(s.shape[0] * 2, np.uint8)
    out[0::2] = s >> 4
    out[1::2] = s & 15
    return out[:n_bases]


def stranded_hist(L, ref_len, rec, min_quality, exclude_flags=0, min_base_quality=None):
    """(2, L, 16) uint32: [0] forward, [1] reverse.  min_base_quality=None: no base-quality filter."""
    codes = unpack_seq4(rec.seq4, int(rec.seq_off[-1])) if rec.n else np.zeros(0, np.uint8)
    flat = [[], []]
    hi = min(L, int(ref_len))
    for r in range(rec.n):
        pos = int(rec.pos[r])
        if pos < 0 or pos >= L or int(rec.mapq[r]) < min_quality or (int(rec.flag[r]) & exclude_flags):
            continue
        strand = 1 if int(rec.flag[r]) & 0x10 else 0
        s0, s1 = int(rec.seq_off[r]), int(rec.seq_off[r + 1])
        q0, q1 = int(rec.qual_off[r]), int(rec.qual_off[r + 1])
        l_seq = s1 - s0
        x, y = pos, 0
        for w in rec.cigar[int(rec.cigar_off[r]):int(rec.cigar_off[r + 1])].tolist():
            op, l = w & 15, w >> 4
            if op in (0, 7, 8):
                n = max(0, min(l, l_seq - y, hi - x))                 # query index < l_seq, position < ref_len (and < L)
                if n > 0:
                    c = codes[s0 + y:s0 + y + n]
                    p = np.arange(x, x + n, dtype=np.int64)
                    if min_base_quality is not None:
                        ok = np.ones(n, bool)
                        nq = max(0, min(n, (q1 - q0) - y))            # the bases of this run that have a quality value
                        if nq > 0:
                            ok[:nq] = rec.qual[q0 + y:q0 + y + nq] >= min_base_quality
                        c, p = c[ok], p[ok]
                    flat[strand].append(p * 16 + c)
                x += l; y += l
            elif op in (2, 3):
                x += l
            elif op in (1, 4):
                y += l
            if x >= hi:
                break
    out = np.zeros((2, L, 16), np.uint32)
    for s in (0, 1):
        if flat[s]:
            out[s] = np.bincount(np.concatenate(flat[s]), minlength=L * 16).astype(np.uint32).reshape(L, 16)
    return out


def counts9(h2):
    """(L, 9): A+ A- C+ C- G+ G- T+ T- depth, the layout of cl_site_scan_counts_ex."""
    L = h2.shape[1]
    out = np.zeros((L, 9), np.uint32)
    for k, c in enumerate(ACGT_CODES):
        out[:, 2 * k] = h2[0, :, c]
        out[:, 2 * k + 1] = h2[1, :, c]
    out[:, 8] = h2.sum((0, 2), dtype=np.uint64).astype(np.uint32)
    return out


def reduce(h2, ref, L, min_depth, start, end):
    """Classes and candidates of [start, end).  A candidate: (pos 1-based, ref, alt, A, C, G, T, depth, alt_fwd, alt_rev,
    ref_fwd, ref_rev)."""
    both = h2[0].astype(np.uint64) + h2[1].astype(np.uint64)
    h = both[start:end]
    depth = h.sum(1)
    m = h.max(1) if end > start else np.zeros(0, np.uint64)
    cstar = h.argmax(1) if end > start else np.zeros(0, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        called = (depth >= min_depth) & (m.astype(np.float64) / depth.astype(np.float64) >= 0.7)
    refb = np.full(L, ord("N"), np.uint8)
    refb[:min(ref.shape[0], L)] = ref[:L]
    rb = refb[start:end] & np.uint8(0xDF)
    ref_ok = np.isin(rb, np.frombuffer(b"ACGT", np.uint8))
    code_ok = np.isin(cstar, ACGT_CODES)
    cbase = np.frombuffer(CODE.encode(), np.uint8)[cstar]
    low = depth < min_depth
    mixed = ~low & ~called
    unc = called & ~(code_ok & ref_ok)
    match = called & code_ok & ref_ok & (cbase == rb)
    var = called & code_ok & ref_ok & (cbase != rb)
    assert int(low.sum() + mixed.sum() + unc.sum() + match.sum() + var.sum()) == end - start
    cand = []
    for i in np.nonzero(var)[0]:
        p = start + int(i)
        ac, rc = int(cstar[i]), CODE.index(chr(rb[i]))
        cand.append((p + 1, chr(rb[i]), chr(cbase[i]), int(h[i, 1]), int(h[i, 2]), int(h[i, 4]), int(h[i, 8]), int(depth[i]),
                     int(h2[0, p, ac]), int(h2[1, p, ac]), int(h2[0, p, rc]), int(h2[1, p, rc])))
    return dict(low_depth=int(low.sum()), mixed=int(mixed.sum()), uncomparable=int(unc.sum()), match=int(match.sum()),
                variant=int(var.sum()), candidates=cand, cls=np.select([low, mixed, unc, match, var], [0, 1, 2, 3, 4]))


def expected_tsv_ex(contig, exp, a, b, md, mq, mbq, exclude_flags, k, notes=None):
    """The extended TSV of find-variants for reduce()'s result; notes: {pos: (names, alleles)} for an annotated file,
    None for one without a tree."""
    out = [f"##contig={contig}", f"##range={a}-{b}", f"##min_depth={md}", f"##min_quality={mq}",
           f"##min_base_quality={'.' if mbq is None else mbq}", f"##exclude_flags=0x{exclude_flags:04x}", f"##positions={b - a}",
           f"##low_depth={exp['low_depth']}", f"##mixed={exp['mixed']}", f"##uncomparable={exp['uncomparable']}", f"##match={exp['match']}",
           f"##variant={exp['variant']}",
           "#contig\tpos\tref\talt\tdepth\tA\tC\tG\tT\tfreq\tstatus\tnames\talleles\talt_fwd\talt_rev\tref_fwd\tref_rev\tfilter"]
    for pos, r, alt, A, C, G, T, depth, af, ar, rf, rr in exp["candidates"]:
        freq = dict(A=A, C=C, G=G, T=T)[alt] / depth
        line = f"{contig}\t{pos}\t{r}\t{alt}\t{depth}\t{A}\t{C}\t{G}\t{T}\t{freq:.4f}\t"
        if notes is None:
            line += ".\t.\t."
        elif pos not in notes:
            line += "novel\t.\t."
        else:
            line += f"known\t{notes[pos][0]}\t{notes[pos][1]}"
        line += f"\t{af}\t{ar}\t{rf}\t{rr}\t{'strand' if min(af, ar) < k else 'PASS'}"
        out.append(line)
    return "\n".join(out) + "\n"
