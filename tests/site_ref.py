"""The independent reference of the site-list pileup (include/callable_loci.h, cl_site_run / cl_site_pileup): plain numpy
on top of tests/scan_ref.py, no device and no library code.

    hist_at_sites   the 16-code row of every entry of a site list: scan_ref.stranded_hist summed over the strands and
                    indexed at site - 1; zeros for a site of 0 and for site - 1 >= min(L, ref_len)
    hits            the (read, site) pairs behind those rows, with the place of the site in the sorted list and the CIGAR
                    operation that holds it: what the tests assert about their own inputs (a case must not pass by being
                    empty) comes from here
    tile shapes     the tiles of tests/test_gpu_site_pileup.py, at any size, so that tests/test_site_ref_host.py can tie
                    this reference to the oracle on every one of them without a device"""
import numpy as np

import scan_ref
from decodingustools_amd import synth
from decodingustools_amd.records import ContigRecords, pack_seq4

BLOCK = 256                    # reads per workgroup of k_site_pileup
LDS_SITES = 64                 # sites a workgroup keeps in LDS (kSiteLds)
ACGT_CODES = np.array([1, 2, 4, 8], np.uint8)


def hist_all(L, ref_len, rec, min_quality):
    """(L, 16) uint32: the row of every position of the contig, both strands."""
    h2 = scan_ref.stranded_hist(L, ref_len, rec, min_quality)
    return h2[0] + h2[1]


def rows(both, L, ref_len, sites):
    """The rows of a site list out of hist_all's table: zeros for a site of 0 and for site - 1 >= min(L, ref_len)."""
    sites = np.asarray(sites, np.int64)
    out = np.zeros((sites.shape[0], 16), np.uint32)
    ok = (sites >= 1) & (sites - 1 < min(L, int(ref_len)))
    out[ok] = both[sites[ok] - 1]
    return out


def hist_at_sites(L, ref_len, rec, min_quality, sites):
    """(n_sites, 16) uint32.  A duplicated site has the same row at every one of its entries."""
    return rows(hist_all(L, ref_len, rec, min_quality), L, ref_len, sites)


def sorted_sites(sites):
    """The list as site_prepare leaves it: 0-based positions ascending (ties in list order), sites of 0 left out."""
    sites = np.asarray(sites, np.int64)
    order = np.argsort(sites, kind="stable")
    order = order[sites[order] >= 1]
    return sites[order] - 1, order


def ref_spans(rec):
    """Per read the reference span of its CIGAR: M D N = X."""
    adv = np.where(np.isin(rec.cigar & 15, [0, 2, 3, 7, 8]), (rec.cigar >> 4).astype(np.int64), 0)
    cs = np.concatenate([[0], np.cumsum(adv)])
    return cs[rec.cigar_off[1:].astype(np.int64)] - cs[rec.cigar_off[:-1].astype(np.int64)]


def hits(L, ref_len, rec, min_quality, sites):
    """Every (read, entry of the sorted list) pair that counts: arrays read, lo (index into sorted_sites), op (index of
    the CIGAR operation inside the read)."""
    pos0, _ = sorted_sites(sites)
    hi = min(L, int(ref_len))
    R, LO, OP = [], [], []
    for r in range(rec.n):
        pos = int(rec.pos[r])
        if pos < 0 or pos >= L or int(rec.mapq[r]) < min_quality:
            continue
        l_seq = int(rec.seq_off[r + 1]) - int(rec.seq_off[r])
        x, y = pos, 0
        for k, w in enumerate(rec.cigar[int(rec.cigar_off[r]):int(rec.cigar_off[r + 1])].tolist()):
            op, l = w & 15, w >> 4
            if op in (0, 7, 8):
                n = max(0, min(l, l_seq - y, hi - x))
                if n > 0:
                    a, b = np.searchsorted(pos0, [x, x + n], side="left")
                    if b > a:
                        R.append(np.full(b - a, r)); LO.append(np.arange(a, b)); OP.append(np.full(b - a, k))
                x += l; y += l
            elif op in (2, 3):
                x += l
            elif op in (1, 4):
                y += l
    cat = lambda v: np.concatenate(v).astype(np.int64) if v else np.zeros(0, np.int64)
    return cat(R), cat(LO), cat(OP)


def group_first(rec, sites):
    """Per read the sorted-list index at which its workgroup's LDS histogram starts: the first sorted site at or after
    the position of the first read of its group of BLOCK reads."""
    pos0, _ = sorted_sites(sites)
    lead = np.maximum(rec.pos[(np.arange(rec.n) // BLOCK) * BLOCK].astype(np.int64), 0)
    return np.searchsorted(pos0, lead, side="left")


def slot_stats(L, ref_len, rec, min_quality, sites):
    """dict: wrapped = hits whose sorted index lies below their workgroup's first one, far = hits at a slot >= LDS_SITES,
    widest = the largest number of distinct sorted sites one workgroup hits, groups = workgroups in the launch."""
    r, lo, _ = hits(L, ref_len, rec, min_quality, sites)
    first = group_first(rec, sites)[r] if r.size else np.zeros(0, np.int64)
    widest = 0
    if r.size:
        pair = np.unique((r // BLOCK) * (int(lo.max()) + 1) + lo)
        widest = int(np.bincount(pair // (int(lo.max()) + 1)).max())
    return dict(hits=int(r.size), wrapped=int((lo < first).sum()), far=int((lo >= first + LDS_SITES).sum()), widest=widest,
                groups=(rec.n + BLOCK - 1) // BLOCK)


def kept(L, rec, min_quality, sites):
    """The reads the one-call form sends (site_filter): inside the contig, mapq, a site inside [pos, pos + span)."""
    pos0, _ = sorted_sites(sites)
    p = rec.pos.astype(np.int64)
    a = np.searchsorted(pos0, p, side="left")
    b = np.searchsorted(pos0, p + ref_spans(rec), side="left")
    return (p >= 0) & (p < L) & (rec.mapq >= min_quality) & (b > a)


# ---- site lists -----------------------------------------------------------------------------------------------------
def site_lists(L, rec, seed):
    """The lists of a contig of length L, by name.  `duplicates` enters 50 covered sites two or three times each."""
    rng = np.random.default_rng(seed)
    u32 = lambda v: np.asarray(v, np.uint32)
    sparse = np.sort(rng.choice(np.arange(1, L + 50), size=max(8, min(L // 12, 5000)), replace=False))
    cover = hist_all(L, L, rec, 0).sum(1) > 0
    pick = rng.choice(np.flatnonzero(cover) + 1, size=min(50, int(cover.sum())), replace=False)
    dup = np.concatenate([sparse, pick, pick, pick[::2]])
    rng.shuffle(dup)
    edges = np.arange(0, L + 600, 256)
    last = int((rec.pos.astype(np.int64) + ref_spans(rec)).max()) if rec.n else 0
    return {"every": u32(np.arange(1, L + 51)), "sparse": u32(sparse), "shuffled": u32(rng.permutation(sparse)), "duplicates": u32(dup),
            "bucket-edges": u32(np.concatenate([edges[1:] - 1, edges, edges + 1])),
            "beyond": u32(max(last, L) + 1 + np.sort(rng.choice(100_000, 200, replace=False))),
            "ends": u32([0, L, L + 1, 2**31]), "empty": u32([])}


# ---- tiles ----------------------------------------------------------------------------------------------------------
def with_random_seq(rec, seed, all_codes=True):
    """4-bit bases for records that have none: as many as the read has quality values (l_seq), any of the 16 codes."""
    rng = np.random.default_rng(seed)
    n = int(rec.qual_off[-1])
    codes = rng.integers(0, 16, n, dtype=np.uint8) if all_codes else ACGT_CODES[rng.integers(0, 4, n)]
    rec.seq_off = rec.qual_off.copy()
    rec.seq4 = pack_seq4(codes)
    return rec


def permuted(rec, order):
    """The records in another order, bases included (offsets rebuilt; the bases keep their nibble values)."""
    order = np.asarray(order, np.int64)

    def ragged(off, data, dtype):
        off = off.astype(np.int64)
        ln = off[1:] - off[:-1]
        new = np.concatenate([[0], np.cumsum(ln[order])])
        idx = np.repeat(off[:-1][order] - new[:-1], ln[order]) + np.arange(int(new[-1]))
        return new.astype(dtype), np.ascontiguousarray(data[idx])
    coff, cig = ragged(rec.cigar_off, rec.cigar, np.uint32)
    qoff, qual = ragged(rec.qual_off, rec.qual, np.uint64)
    noff, qname = ragged(rec.qname_off, rec.qname, np.uint32)
    out = ContigRecords(pos=np.ascontiguousarray(rec.pos[order]), flag=np.ascontiguousarray(rec.flag[order]),
                        mapq=np.ascontiguousarray(rec.mapq[order]), cigar_off=coff, cigar=cig, qual_off=qoff, qual=qual,
                        qname_off=noff, qname=qname).validate()
    soff, codes = ragged(rec.seq_off, scan_ref.unpack_seq4(rec.seq4, int(rec.seq_off[-1])), np.uint64)
    out.seq_off, out.seq4 = soff, pack_seq4(codes)
    return out


ADVERSARIAL = ((1, 3000, 600, False), (2, 5000, 1500, True), (3, 2048, 900, True), (4, 700, 300, False))


def adversarial_tile(seed, L, n, overhang):
    return with_random_seq(synth.adversarial_contig(L, n, seed, overhang=overhang, deep=(seed == 2)), 100 + seed)


def edge_reads(L):
    """Ten hand-written reads: fewer bases than the CIGAR spends, every kind of operation, an overhang, the last position,
    starts at and beyond the contig end, two mapping qualities around 20."""
    seq = "ACGTN=MR" * 50
    return [(0, "50M", 60, 30, 0, "first", seq[:50]), (10, "100M", 60, 30, 0, "a", seq[:100]),
            (20, "30M", 60, 30, 0, "fewer-bases", seq[:12]),
            (25, "10S20M5I20M3D10M2N10M5H", 60, 30, 0, "ops", seq[:75]),
            (L - 40, "100M", 60, 30, 0, "overhang", seq[:100]), (L - 1, "10M", 60, 30, 0, "last", seq[:10]),
            (L, "50M", 60, 30, 0, "at-end", seq[:50]), (L + 500, "50M", 60, 30, 0, "beyond", seq[:50]),
            (1500, "40M", 19, 30, 0, "lowq", seq[:40]), (1500, "40M", 20, 30, 0, "q20", seq[:40])]


def edge_tiles(L):
    reads = edge_reads(L)
    return {"sorted": ContigRecords.from_reads(reads), "reversed": ContigRecords.from_reads(reads[::-1]),
            "rotated": ContigRecords.from_reads(reads[3:] + reads[:3])}


def shuffled_short_reads(L, depth, seed):
    """A short-read tile with its reads randomly permuted: every workgroup spans the contig."""
    rec = synth.short_read_contig(L, depth, seed, with_seq=True)
    return permuted(rec, np.random.default_rng(seed + 1).permutation(rec.n))


def ladder_tile(L, n, seed):
    """Reads of exactly 1 ... 6 operations.  The first four are S, H, I, P in varying order and hold no reference span;
    the matched bases begin at the fifth operation of the reads that have one, and the sixth is a second matched run of
    another kind.  Every other read of one operation is a single matched run instead of a clip, and so is the very last
    read of the tile: the 16-byte load of its CIGAR words ends in the padding behind the tile's last word."""
    rng = np.random.default_rng(seed)
    reads = []
    starts = np.sort(rng.integers(0, L - 200, n))
    for i in range(n):
        k = 1 if i == n - 1 else 1 + i % 6
        ops = [(str(o), int(rng.integers(1, 9))) for o in rng.permutation(list("SHIP"))[:min(k, 4)]]
        if k == 1 and (i % 12 == 0 or i == n - 1):
            ops = [(str(rng.choice(list("M=X"))), int(rng.integers(1, 150)))]
        if k >= 5:
            ops.append((str(rng.choice(list("M=X"))), int(rng.integers(1, 120))))
        if k == 6:
            ops.append((str(rng.choice(list("=X"))) if ops[-1][0] == "M" else "M", int(rng.integers(1, 60))))
        cig = "".join(f"{l}{o}" for o, l in ops)
        ql = sum(l for o, l in ops if o in "MIS=X")
        seq = "".join(rng.choice(list(scan_ref.CODE), ql))
        reads.append((int(starts[i]), cig, int(rng.choice([0, 9, 10, 60])), 30, 0, f"l{i}", seq))
    rec = ContigRecords.from_reads(reads)
    nops = np.diff(rec.cigar_off.astype(np.int64))
    assert sorted(set(nops.tolist())) == [1, 2, 3, 4, 5, 6] and nops[-1] == 1 and (rec.cigar[-1] & 15) in (0, 7, 8)
    return rec


def long_cigar(n_ops, rng):
    """n_ops operations: M runs of 5-40 bases between I / D / N / =X, starting and ending on M."""
    ops = []
    while len(ops) < n_ops - 1:
        ops.append(("M", int(rng.integers(5, 40))))
        ops.append((str(rng.choice(["I", "D", "N", "X", "="])), int(rng.integers(1, 6))))
    ops = ops[:n_ops - 1] + [("M", 20)]
    return "".join(f"{l}{o}" for o, l in ops), sum(l for o, l in ops if o in "MIS=X")


def escape_tile(scale=1):
    """The values at which a SiteRec hands over to the next record's offsets: 254, 255 and 300 operations, 65 534,
    65 535 and 70 000 bases (scale < 1 shrinks the base counts for the host-only test, which has no such edge)."""
    rng = np.random.default_rng(5)
    seq = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    c300, q300 = long_cigar(300, rng)
    c255, q255 = long_cigar(255, rng)
    c254, q254 = long_cigar(254, rng)
    b = [int(x * scale) for x in (70000, 65535, 65534, 30000)]
    reads = [(100, c300, 60, 30, 0, "ops300", seq(q300)), (900, c255, 60, 30, 0, "ops255", seq(q255)), (950, c254, 60, 30, 0, "ops254", seq(q254)),
             (2000, f"{b[0]}M", 60, 30, 0, "b70000", seq(b[0])), (2500, f"{b[1]}M", 60, 30, 0, "b65535", seq(b[1])),
             (3000, f"{b[2]}M", 60, 30, 0, "b65534", seq(b[2])), (3500, f"{b[3]}M200D{b[3]}M", 33, 30, 0, "del", seq(2 * b[3]))]
    return ContigRecords.from_reads(reads)


def no_escape(rec):
    """True when no read of the tile has 255 operations or 65 535 bases and more: the one-call form may filter it."""
    return int(np.diff(rec.cigar_off.astype(np.int64)).max()) < 255 and int(np.diff(rec.seq_off.astype(np.int64)).max()) < 0xFFFF


def pile_tile(n, start=1000):
    """n identical 50-base reads at one start."""
    rec = ContigRecords(pos=np.full(n, start, np.int32), flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8),
                        cigar_off=np.arange(n + 1, dtype=np.uint32), cigar=np.full(n, (50 << 4) | 0, np.uint32),
                        qual_off=np.arange(n + 1, dtype=np.uint64) * np.uint64(50), qual=np.full(n * 50, 30, np.uint8),
                        qname_off=np.arange(n + 1, dtype=np.uint32), qname=np.full(n, ord("p"), np.uint8)).validate()
    rec.seq_off = rec.qual_off.copy()
    rec.seq4 = np.tile(pack_seq4(np.array([1, 2, 4, 8, 15] * 10, np.uint8)), n)
    return rec


def odd_length_tile(L, n, seed):
    """Single-M reads of odd and even lengths in coordinate order, one in nine without bases (l_seq = 0): the base
    offsets of the reads that follow an odd one are odd."""
    rng = np.random.default_rng(seed)
    reads = []
    for i, p in enumerate(np.sort(rng.integers(0, L - 160, n)).tolist()):
        l = int(rng.integers(20, 151))
        seq = "" if i % 9 == 4 else "".join(rng.choice(list(scan_ref.CODE), l))
        reads.append((p, f"{l}M", int(rng.choice([0, 10, 60])), 30, 0, f"o{i}", seq))
    return ContigRecords.from_reads(reads)


def half_dropping_list(L, rec, seed):
    """A sparse list that leaves about half of the reads of odd_length_tile without a site."""
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(np.arange(1, L + 1), size=max(4, L // 120), replace=False)).astype(np.uint32)


# ---- a tile whose base offsets pass 2^32 (or any other mark, for the host-only test) ------------------------------------
def concat(recs):
    """Several tiles as one, in the order given (the bases are repacked nibble by nibble)."""
    cat = lambda name, dt: np.ascontiguousarray(np.concatenate([getattr(r, name) for r in recs]), dtype=dt)

    def offs(name, dt):
        out, base = [np.zeros(1, np.int64)], 0
        for r in recs:
            o = getattr(r, name).astype(np.int64)
            out.append(o[1:] - o[0] + base); base += int(o[-1] - o[0])
        return np.concatenate(out).astype(dt)
    out = ContigRecords(pos=cat("pos", np.int32), flag=cat("flag", np.uint16), mapq=cat("mapq", np.uint8), cigar_off=offs("cigar_off", np.uint32),
                        cigar=cat("cigar", np.uint32), qual_off=offs("qual_off", np.uint64), qual=cat("qual", np.uint8),
                        qname_off=offs("qname_off", np.uint32), qname=cat("qname", np.uint8)).validate()
    out.seq_off = offs("seq_off", np.uint64)
    out.seq4 = pack_seq4(np.concatenate([scan_ref.unpack_seq4(r.seq4, int(r.seq_off[-1]))[int(r.seq_off[0]):] for r in recs]))
    return out


def ballast_bases(interesting, cross_read, mark):
    """The even number of ballast bases in front of `interesting` that puts `mark` inside the bases of its read
    cross_read: seq_off[cross_read] < mark <= seq_off[cross_read + 1] in the whole tile."""
    s0, s1 = int(interesting.seq_off[cross_read]), int(interesting.seq_off[cross_read + 1])
    assert s1 - s0 >= 4
    B = mark - s0 - (s1 - s0) // 2
    return B - (B & 1)


def ballast_buffer(interesting, B, seed):
    """The bases of the whole tile: B random ballast bases (B even), then those of `interesting`."""
    nb = B // 2
    buf = np.empty(nb + interesting.seq4.shape[0], np.uint8)
    rng = np.random.default_rng(seed)
    step = 1 << 27
    for a in range(0, nb, step):
        n = min(step, nb - a)
        buf[a:a + n] = rng.integers(0, 1 << 63, (n + 7) // 8, dtype=np.int64).view(np.uint8)[:n]
    buf[nb:] = interesting.seq4
    return buf


def ballast_lengths(B, about, fixed=False, seed=0):
    """Read lengths that add up to B: all `about` long and a shorter last one (fixed), or about `about`, up to a tenth
    more or less."""
    if fixed:
        n = B // about
        return np.concatenate([np.full(n, about, np.int64), np.full(1 if B % about else 0, B % about, np.int64)])
    n = max(2, B // about)
    lens = np.full(n, B // n, np.int64)
    d = np.random.default_rng(seed).integers(0, max(1, B // n // 10), n // 2)
    lens[0:2 * (n // 2):2] += d; lens[1:2 * (n // 2):2] -= d
    lens[-1] += B - int(lens.sum())
    return lens


def ballast_tile(interesting, buf, lens, span, seed, mapq=5):
    """Single-M ballast reads over the first bases of buf (lengths lens, starts in [0, span), no quality values,
    flag 0), then the interesting reads.  Returns (tile, number of ballast reads)."""
    nb = lens.shape[0]
    B = int(lens.sum())
    it = interesting
    pos = np.sort(np.random.default_rng(seed).integers(0, span, nb)).astype(np.int32)
    u = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    rec = ContigRecords(pos=u(np.concatenate([pos, it.pos]), np.int32), flag=u(np.concatenate([np.zeros(nb, np.uint16), it.flag]), np.uint16),
                        mapq=u(np.concatenate([np.full(nb, mapq, np.uint8), it.mapq]), np.uint8),
                        cigar_off=u(np.concatenate([np.arange(nb), nb + it.cigar_off.astype(np.int64)]), np.uint32),
                        cigar=u(np.concatenate([(lens << 4).astype(np.uint32), it.cigar]), np.uint32),
                        qual_off=u(np.concatenate([np.zeros(nb, np.uint64), it.qual_off]), np.uint64), qual=it.qual,
                        qname_off=u(np.concatenate([np.arange(nb), nb + it.qname_off.astype(np.int64)]), np.uint32),
                        qname=u(np.concatenate([np.full(nb, ord("b"), np.uint8), it.qname]), np.uint8)).validate()
    rec.seq_off = u(np.concatenate([np.concatenate([[0], np.cumsum(lens)])[:-1], B + it.seq_off.astype(np.int64)]), np.uint64)
    rec.seq4 = buf
    assert int(it.seq_off[0]) == 0 and B % 2 == 0 and buf.shape[0] == B // 2 + it.seq4.shape[0]
    return rec, nb


def ballast_share(tile, nb, L, ref_len, positions):
    """(len(positions), 16): what the ballast reads [0, nb) of the tile count at the 0-based positions given -- the code of
    read r at position p is nibble seq_off[r] + p - pos[r], for pos[r] <= p < pos[r] + length, p < min(L, ref_len)."""
    positions = np.asarray(positions, np.int64)
    uniq, inv = np.unique(positions, return_inverse=True)
    uniq_ok = uniq[(uniq >= 0) & (uniq < min(L, int(ref_len)))]
    acc = np.zeros(uniq.shape[0] * 16, np.int64)
    base = int(np.searchsorted(uniq, 0, side="left"))                 # index of uniq_ok[0] in uniq
    pos = tile.pos[:nb].astype(np.int64)
    soff = tile.seq_off[:nb + 1].astype(np.int64)
    step = max(1, (1 << 23) // max(1, uniq_ok.shape[0]))
    for r0 in range(0, nb, step):
        r1 = min(nb, r0 + step)
        ok = (pos[r0:r1] >= 0) & (pos[r0:r1] < L)
        a = np.searchsorted(uniq_ok, pos[r0:r1], side="left")
        b = np.where(ok, np.searchsorted(uniq_ok, pos[r0:r1] + (soff[r0 + 1:r1 + 1] - soff[r0:r1]), side="left"), a)
        cnt = b - a
        tot = int(cnt.sum())
        if tot == 0:
            continue
        rr = np.repeat(np.arange(r0, r1), cnt)
        start = np.cumsum(cnt) - cnt
        si = np.repeat(a - start, cnt) + np.arange(tot)
        bi = soff[rr] + uniq_ok[si] - pos[rr]
        byte = tile.seq4[bi >> 1]
        code = np.where(bi & 1, byte & 15, byte >> 4).astype(np.int64)
        acc += np.bincount((si + base) * 16 + code, minlength=acc.shape[0])
    return acc.reshape(-1, 16)[inv].astype(np.uint32)
