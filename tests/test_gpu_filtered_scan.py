"""The filtered, strand-aware site scan on the device (-m gpu): cl_site_attach_quals / cl_site_scan_ex /
cl_site_scan_counts_ex / find-variants with the filter flags, everything compared exactly with the independent numpy
reference tests/scan_ref.py (tied to the committed oracle in tests/test_filtered_scan_host.py) -- never with the engine's
own other calls, except where the invariant between the two is what is tested."""
import random
import subprocess

import numpy as np
import pytest

import scan_ref as R
from bamio import write_bam, write_fasta
from helpers import load_kats
from decodingustools_amd import CallableOptions, Engine, EngineError, build as _b, haplogroup as H, synth, variants as V
from decodingustools_amd._lib import CL_SCAN_MAX_DENSE
from decodingustools_amd.records import ContigRecords, pack_seq4
from oracle import haplogroup_oracle as HO

pytestmark = pytest.mark.gpu
KATS = load_kats()
W = 1024                                            # the kernel's window
FILTERS = [(ex, bq) for ex in (0, 0x10, 0x704, 0xFFFF) for bq in (False, True)]
QUALS = np.array([2, 12, 19, 20, 21, 37, 255], np.uint8)


def random_flags(n, seed):
    """Every bit somewhere, 0x10 on about half, and enough reads with no excluded bit that every filter leaves some."""
    rng = np.random.default_rng(seed)
    wild = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    tame = (wild & np.uint16(0x10)) | rng.choice(np.array([0, 0, 0, 1, 2, 0x20, 0x40, 0x80, 0x63, 0x400, 0x100], np.uint16), n)
    tame[rng.random(n) < 0.15] = 0
    return np.where(rng.random(n) < 0.6, tame, wild).astype(np.uint16)


def requal(rec, seed, ragged=True):
    """New quality values around the thresholds; ragged: some reads get fewer values than bases, or none, so that the
    numbering of qual_off differs from that of seq_off."""
    rng = np.random.default_rng(seed)
    l_seq = np.diff(rec.seq_off.astype(np.int64))
    nq = l_seq.copy()
    if ragged:
        k = rng.random(rec.n)
        nq[k < 0.1] = 0
        part = (k >= 0.1) & (k < 0.25)
        nq[part] = (l_seq[part] * rng.random(int(part.sum()))).astype(np.int64)
    rec.qual_off = np.concatenate([[0], np.cumsum(nq)]).astype(np.uint64)
    rec.qual = QUALS[rng.integers(0, QUALS.shape[0], int(nq.sum()))]
    rec.flag = random_flags(rec.n, seed + 1)
    return rec.validate()


def with_random_seq(rec, seed, all_codes=True):
    rng = np.random.default_rng(seed)
    n = int(rec.qual_off[-1])
    codes = rng.integers(0, 16, n, dtype=np.uint8) if all_codes else np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, n)]
    rec.seq_off = rec.qual_off.copy()
    rec.seq4 = pack_seq4(codes)
    return rec


def ranges_for(L):
    r = [(0, L), (0, 0), (L, L), (0, 1), (L - 1, L), (3, 700), (W - 1, W + 1), (W, 2 * W), (1000, 3 * W + 17), (L // 2, L)]
    return sorted({(max(0, min(a, L)), max(0, min(b, L))) for a, b in r if min(a, L) <= min(b, L)})


def same_scan(got, exp, what):
    assert (got.low_depth, got.mixed, got.uncomparable, got.match, got.variant) == \
        (exp["low_depth"], exp["mixed"], exp["uncomparable"], exp["match"], exp["variant"]), what
    have = [(int(r["pos"]), chr(r["ref"]), chr(r["alt"]), int(r["a"]), int(r["c"]), int(r["g"]), int(r["t"]), int(r["depth"]),
             int(r["alt_fwd"]), int(r["alt_rev"]), int(r["ref_fwd"]), int(r["ref_rev"])) for r in got.candidates]
    assert have == exp["candidates"], what


def check_filters(eng, L, ref, rec, mq, mbq, filters=FILTERS, ranges=None, depths=(1, 5), what=""):
    """The resident tile of `eng` is `rec` with an attachment at mbq: counters and calls of every filter and range."""
    ref_len = ref.shape[0]
    total = {}
    for ex, bq in filters:
        h2 = R.stranded_hist(L, ref_len, rec, mq, ex, mbq if bq else None)
        want = R.counts9(h2)
        total[(ex, bq)] = int(want[:, 8].sum(dtype=np.uint64))
        for a, b in (ranges or ranges_for(L)):
            if b - a <= CL_SCAN_MAX_DENSE:
                got = eng.site_scan_counts_ex(mq, a, b, ex, bq)
                assert got.shape == (b - a, 9)
                bad = np.nonzero((got != want[a:b]).any(1))[0]
                assert bad.size == 0, (what, mq, mbq, hex(ex), bq, (a, b), int(a + bad[0]), got[bad[0]].tolist(), want[a + bad[0]].tolist())
            for md in depths:
                same_scan(eng.site_scan_ex(mq, md, ref, ex, bq, a, b), R.reduce(h2, ref, L, md, a, b), (what, mq, mbq, hex(ex), bq, (a, b), md))
    return total


@pytest.mark.parametrize("case", KATS["site_cases"], ids=[c["name"] for c in KATS["site_cases"]])
def test_filtered_scan_site_kats(case):
    rec = requal(ContigRecords.from_reads([tuple(r) for r in case["reads"]]), 5)
    ref = np.frombuffer(case["ref"].encode(), dtype=np.uint8).copy()
    L = case["contig_len"]
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, ref.shape[0], rec)
        for mbq in (0, 20, 255):
            eng.site_attach_quals(rec, mbq)
            for mq in (0, case["min_quality"]):
                check_filters(eng, L, ref, rec, mq, mbq, depths=(1, case["min_depth"]), what=case["name"])


def test_filtered_scan_adversarial_cigars_and_edges():
    """All 16 codes, every CIGAR operation, overhang, unsorted order, l_seq shorter than the CIGAR, reads with fewer
    quality values than bases; ranges inside, at and across window edges; ref_len < contig_len."""
    for seed, L, n, overhang in ((1, 3000, 600, False), (2, 5000, 1500, True), (3, 2 * W, 900, True), (4, 700, 300, False)):
        rec = requal(with_random_seq(synth.adversarial_contig(L, n, seed, overhang=overhang, deep=(seed == 2)), 100 + seed), 200 + seed)
        ref = synth.make_reference(L, 50 + seed, lowercase=True)
        with Engine(CallableOptions(), 0) as eng:
            eng.site_upload(L, L, rec)
            for mbq in (0, 20, 255):
                eng.site_attach_quals(rec, mbq)
                tot = check_filters(eng, L, ref, rec, 10, mbq, what=("adversarial", seed))
                # every filtered total is at most the unfiltered one; 0x704 with qualities removes something, not everything
                assert all(v <= tot[(0, False)] for v in tot.values())
                if mbq == 20:
                    assert 0 < tot[(0x704, True)] < tot[(0, False)] and 0 < tot[(0xFFFF, False)] < tot[(0x704, False)]
            eng.site_upload(L, L - 300, rec)
            eng.site_attach_quals(rec, 20)
            check_filters(eng, L, ref[:L - 300], rec, 10, 20, filters=[(0x704, True), (0, False)],
                          ranges=[(0, L), (L - 305, L - 295), (L - 300, L)], what=("short reference", seed))
    L = 4000
    seq = "ACGTN=MR" * 50
    reads = [(0, "50M", 60, 30, 0x10, "first", seq[:50]), (10, "100M", 60, [5] * 40, 0, "a", seq[:100]),
             (20, "30M", 60, 30, 0x400, "fewer-bases", seq[:12]),
             (25, "10S20M5I20M3D10M2N10M5H", 60, [25, 3] * 37, 0x10, "ops", seq[:75]),
             (L - 40, "100M", 60, 30, 0, "overhang", seq[:100]), (L - 1, "10M", 60, None, 0x10, "last", seq[:10]),
             (L, "50M", 60, 30, 0, "at-end", seq[:50]), (L + 500, "50M", 60, 30, 0, "beyond", seq[:50]),
             (1500, "40M", 19, 30, 0, "lowq", seq[:40]), (1500, "40M", 20, 30, 0x110, "q20", seq[:40])]
    for order in (reads, reads[::-1], reads[3:] + reads[:3]):
        rec = ContigRecords.from_reads(order)
        ref = synth.make_reference(L, 9)
        with Engine(CallableOptions(), 0) as eng:
            eng.site_upload(L, L, rec)
            eng.site_attach_quals(rec, 20)
            check_filters(eng, L, ref, rec, 20, 20, what="edges")


def long_cigar(n_ops, rng):
    ops = []
    while len(ops) < n_ops - 1:
        ops.append(("M", int(rng.integers(5, 40))))
        ops.append((str(rng.choice(["I", "D", "N", "X", "="])), int(rng.integers(1, 6))))
    ops = ops[:n_ops - 1] + [("M", 20)]
    return "".join(f"{l}{o}" for o, l in ops), sum(l for o, l in ops if o in "MIS=X")


def test_filtered_scan_long_reads_and_a_deep_strand():
    """SiteRec's escapes (255 and more operations, 65 535 and more bases) and a pile deeper than 2^16 on one strand."""
    rng = np.random.default_rng(5)
    L = 90_000
    ref = synth.make_reference(L, 21)

    def seq(n):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    c300, q300 = long_cigar(300, rng)
    c255, q255 = long_cigar(255, rng)
    c254, q254 = long_cigar(254, rng)
    reads = [(100, c300, 60, 30, 0x10, "ops300", seq(q300)), (900, c255, 60, 30, 0, "ops255", seq(q255)), (950, c254, 60, 30, 0x10, "ops254", seq(q254)),
             (2000, "70000M", 60, 30, 0, "b70000", seq(70000)), (2500, "65535M", 60, 30, 0x10, "b65535", seq(65535)),
             (3000, "65534M", 60, 30, 0x410, "b65534", seq(65534)), (3500, "30000M200D30000M", 33, 30, 0, "del", seq(60000))]
    rec = ContigRecords.from_reads(reads)
    flags = rec.flag.copy()
    rec = requal(rec, 31)
    rec.flag = flags
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        check_filters(eng, L, ref, rec, 0, 20, filters=[(0, False), (0x704, True), (0x10, True)],
                      ranges=[(0, L), (W - 3, 5 * W + 9), (70 * W, L)], depths=(1,), what="long operations")
    n = 70_000
    pile = ContigRecords(pos=np.full(n, 1000, np.int32), flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8),
                         cigar_off=np.arange(n + 1, dtype=np.uint32), cigar=np.full(n, (50 << 4) | 0, np.uint32),
                         qual_off=np.arange(n + 1, dtype=np.uint64) * np.uint64(50), qual=np.full(n * 50, 30, np.uint8),
                         qname_off=np.arange(n + 1, dtype=np.uint32), qname=np.full(n, ord("p"), np.uint8)).validate()
    pile.flag[:67_000] = 0x10                                 # 67 000 > 2^16 on the reverse strand
    pile.flag[67_000:67_500] = 0x400
    pile.qual[::7] = 10
    pile.seq_off = pile.qual_off.copy()
    pile.seq4 = np.tile(pack_seq4(np.array([1, 2, 4, 8, 15] * 10, np.uint8)), n)
    Lp = 3000
    refp = synth.make_reference(Lp, 3)
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(Lp, Lp, pile)
        eng.site_attach_quals(pile, 20)
        check_filters(eng, Lp, refp, pile, 20, 20, filters=[(0, False), (0x704, True)], ranges=[(0, Lp), (990, 1060)], depths=(10,), what="pile")
        got = eng.site_scan_counts_ex(20, 1000, 1001, 0, False)
        assert int(got[0, 1]) == 67_000 and int(got[0, 8]) == n


def planted_sample(L):
    """A 200 kb contig whose reads carry 200 substitutions, plus two kinds of artefact: positions where the alternative
    base sits only on bases below Q20, and positions where it sits only on reverse-strand reads."""
    ref = synth.make_reference(L, 7)
    rng = np.random.default_rng(23)
    sample = ref.copy()
    ok = np.nonzero(np.isin(ref & np.uint8(0xDF), np.frombuffer(b"ACGT", np.uint8)))[0]
    ok = ok[(ok > 2000) & (ok < L - 2000)]
    picks = np.sort(rng.choice(ok, 240, replace=False))
    planted, lowq_pos, rev_pos = picks[:200], picks[200:220], picks[220:240]
    code = {ord("A"): 1, ord("C"): 2, ord("G"): 4, ord("T"): 8}
    alt_of = {}
    for p in picks:
        alt_of[int(p)] = int(rng.choice([b for b in b"ACGT" if b != (ref[p] & 0xDF)]))
    for p in planted:
        sample[p] = alt_of[int(p)]
    rec = synth.short_read_contig(L, 40, 11, with_seq=True, ref=sample)
    rec.flag = rec.flag | (np.random.default_rng(3).integers(0, 2, rec.n).astype(np.uint16) << np.uint16(4))
    # the artefacts are written into the reads: plain 150M reads only (query index = position - start)
    codes = R.unpack_seq4(rec.seq4, int(rec.seq_off[-1])).copy()
    qual = rec.qual.copy()
    plain = (np.diff(rec.cigar_off.astype(np.int64)) == 1) & (rec.cigar[rec.cigar_off[:-1].astype(np.int64)] == ((150 << 4) | 0))
    pos = rec.pos.astype(np.int64)
    for p in lowq_pos.tolist() + rev_pos.tolist():
        over = np.nonzero((pos <= p) & (pos + 150 > p))[0]
        for r in over:
            if not plain[r]:
                rec.mapq[r] = 0                               # keeps the columns simple: other reads do not count there
                continue
            bi = int(rec.seq_off[r]) + (p - int(pos[r]))
            qi = int(rec.qual_off[r]) + (p - int(pos[r]))
            if p in lowq_pos:
                codes[bi] = code[alt_of[p]]; qual[qi] = 5    # every base there is the alternative, all below the threshold
            else:
                rev = bool(rec.flag[r] & 0x10)
                qual[qi] = 37
                codes[bi] = code[alt_of[p]] if rev else code[int(ref[p] & 0xDF)]
        if p in rev_pos:                                      # the alternative must hold 0.7: thin the forward reads out
            fwd = [r for r in over if plain[r] and not (rec.flag[r] & 0x10)]
            for r in fwd[2:]:
                rec.mapq[r] = 0
    rec.seq4 = pack_seq4(codes)
    rec.qual = qual
    return ref, rec.validate(), planted, lowq_pos, rev_pos


def test_filtered_scan_finds_planted_variants_and_artefacts():
    L = 200_000
    ref, rec, planted, lowq_pos, rev_pos = planted_sample(L)
    off = R.stranded_hist(L, L, rec, 20)
    on = R.stranded_hist(L, L, rec, 20, 0x704, 20)
    exp_off, exp_on = R.reduce(off, ref, L, 10, 0, L), R.reduce(on, ref, L, 10, 0, L)
    # the reference itself shows all of it before the device is asked
    found = {c[0] - 1 for c in exp_on["candidates"]}
    assert len(found & set(planted.tolist())) >= 150, len(found & set(planted.tolist()))
    var_off = {c[0] - 1 for c in exp_off["candidates"]}
    gone = [p for p in lowq_pos.tolist() if p in var_off and p not in found]
    assert len(gone) >= 10, len(gone)                                  # variant with the filter off, not with it on
    by_pos = {c[0] - 1: c for c in exp_on["candidates"]}
    one_strand = [p for p in rev_pos.tolist() if p in by_pos and by_pos[p][8] == 0 and by_pos[p][9] > 0]
    assert len(one_strand) >= 5, len(one_strand)                       # alt_fwd == 0: flagged `strand` at K = 1
    d_on, d_off = int(on.sum(dtype=np.uint64)), int(off.sum(dtype=np.uint64))
    assert 0 < d_on < d_off
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        same_scan(eng.site_scan_ex(20, 10, ref, 0x704, True), exp_on, "filtered")
        same_scan(eng.site_scan_ex(20, 10, ref, 0, False), exp_off, "filter off")
        for a, b in ((777, 778), (W - 1, 3 * W + 1), (L - 5000, L)):
            same_scan(eng.site_scan_ex(20, 10, ref, 0x704, True, a, b), R.reduce(on, ref, L, 10, a, b), (a, b))
        got = eng.site_scan_counts_ex(20, 0, L, 0x704, True)
        assert np.array_equal(got, R.counts9(on))
        ms, nbytes = eng.site_scan_stats()
        assert ms > 0 and nbytes > rec.seq4.shape[0] + int(rec.seq_off[-1]) // 8 + 2 * rec.n


def test_invariants_between_the_two_forms_and_the_attachment():
    L = 120_000
    ref = synth.make_reference(L, 31)
    sample = ref.copy()                                        # the reads carry 300 substitutions: the scans have candidates
    rng = np.random.default_rng(8)
    for p in rng.choice(L, 300, replace=False):
        sample[p] = rng.choice(list(b"ACGT"))
    rec = synth.short_read_contig(L, 30, 41, with_seq=True, ref=sample)
    rec.flag = rec.flag | (np.random.default_rng(2).integers(0, 2, rec.n).astype(np.uint16) << np.uint16(4))
    sites = np.sort(np.random.default_rng(8).choice(np.arange(1, L + 1), 4000, replace=False)).astype(np.uint32)
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        before = eng.site_run(20, sites)
        eng.site_attach_quals(rec, 20)
        # filter off equals the unfiltered form on the same tile, strands summed
        plain = eng.site_scan(20, 10, ref)
        ex = eng.site_scan_ex(20, 10, ref, 0, False)
        assert (plain.low_depth, plain.mixed, plain.uncomparable, plain.match, plain.variant) == \
            (ex.low_depth, ex.mixed, ex.uncomparable, ex.match, ex.variant)
        for f in ("pos", "ref", "alt", "a", "c", "g", "t", "depth"):
            assert np.array_equal(plain.candidates[f], ex.candidates[f]), f
        alt_total = ex.candidates["alt_fwd"].astype(np.int64) + ex.candidates["alt_rev"]
        alt_count = np.choose(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), ex.candidates["alt"]),
                              [ex.candidates["a"], ex.candidates["c"], ex.candidates["g"], ex.candidates["t"]])
        assert np.array_equal(alt_total, alt_count) and ex.variant > 0
        c5 = eng.site_scan_counts(20, 0, L)
        c9 = eng.site_scan_counts_ex(20, 0, L, 0, False)
        assert np.array_equal(c5[:, :4], c9[:, 0:8:2] + c9[:, 1:8:2]) and np.array_equal(c5[:, 4], c9[:, 8])
        # every filtered counter is <= the unfiltered one
        f9 = eng.site_scan_counts_ex(20, 0, L, 0x704, True)
        assert (f9 <= c9).all() and int(f9[:, 8].sum()) < int(c9[:, 8].sum())
        assert np.array_equal(eng.site_run(20, sites), before)                    # cl_site_run is left alone
        # two attachments at different thresholds, scans in either order, each equal the reference
        h20 = R.stranded_hist(L, L, rec, 20, 0x704, 20)
        h30 = R.stranded_hist(L, L, rec, 20, 0x704, 30)
        assert not np.array_equal(h20, h30)
        for mbq, h in ((30, h30), (20, h20), (30, h30)):
            eng.site_attach_quals(rec, mbq)
            assert np.array_equal(eng.site_scan_counts_ex(20, 0, L, 0x704, True), R.counts9(h)), mbq
            same_scan(eng.site_scan_ex(20, 10, ref, 0x704, True), R.reduce(h, ref, L, 10, 0, L), mbq)
            again = eng.site_scan(20, 10, ref)
            assert again.variant == plain.variant and np.array_equal(again.candidates, plain.candidates)
        # a new upload drops the attachment
        eng.site_upload(L, L, rec)
        with pytest.raises(EngineError) as e:
            eng.site_scan_ex(20, 10, ref, 0, False)
        assert e.value.status == -1 and "attach" in str(e.value)
        assert np.array_equal(eng.site_run(20, sites), before)


def test_other_code_columns_are_settled_under_the_filter():
    """The columns of test_scan_settles_positions_ruled_by_other_codes with reads excluded by flag and bases below the
    threshold: the settlement must use the filtered 16-code counts, not cl_site_run's."""
    L = 300
    ref = synth.make_reference(L, 2)
    col = ["M" * 10, "M" * 8 + "RR", "MMMMRRRRAA", "=" * 7 + "ACG", "RRRYYYKKKA", "NNNNNNNNMM", "NNNNMMMMRR"]
    flags = [0, 0x10, 0, 0x10, 0x400, 0x410, 0, 0x10, 0x100, 0]
    quals = [[30] * 7 for _ in range(10)]
    quals[0][4] = 3; quals[1][4] = 3; quals[2][4] = 3            # column 4: RRR YYY KKK A -> the three R leave: Y and K share it
    quals[6][2] = 3; quals[7][2] = 3                             # column 2: MMMM RRRR AA -> two R leave
    reads = [(100, f"{len(col)}M", 60, quals[i], flags[i], f"r{i}", "".join(c[i] for c in col)) for i in range(10)]
    rec = ContigRecords.from_reads(reads)
    off = R.reduce(R.stranded_hist(L, L, rec, 20), ref, L, 3, 0, L)
    assert off["cls"][100:107].tolist() == [2, 2, 1, 2, 1, 2, 1]
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        differs = 0
        for ex, bq in ((0, False), (0x704, False), (0, True), (0x704, True), (0x10, True), (0xFFFF, True)):
            exp = R.reduce(R.stranded_hist(L, L, rec, 20, ex, 20 if bq else None), ref, L, 3, 0, L)
            differs += exp["cls"][100:107].tolist() != off["cls"][100:107].tolist()
            same_scan(eng.site_scan_ex(20, 3, ref, ex, bq), exp, (hex(ex), bq))
            same_scan(eng.site_scan_ex(20, 3, ref, ex, bq, 101, 105), R.reduce(R.stranded_hist(L, L, rec, 20, ex, 20 if bq else None), ref, L, 3, 101, 105),
                      (hex(ex), bq, "range"))
        assert differs >= 1                                      # the filtered class differs from the unfiltered one somewhere


def test_refusals_leave_the_context_usable():
    L = 50_000
    ref = synth.make_reference(L, 3)
    rec = synth.short_read_contig(L, 20, 4, with_seq=True, ref=ref)
    sites = np.arange(1, 2000, 7, dtype=np.uint32)

    def refused(fn, *a):
        with pytest.raises(EngineError) as e:
            fn(*a)
        assert e.value.status == -1 and len(str(e.value)) > len(" (cl_status -1)") + 10, str(e.value)

    with Engine(CallableOptions(), 0) as eng:
        refused(eng.site_attach_quals, rec, 20)                                    # nothing resident
        refused(eng.site_scan_ex, 20, 10, ref)
        eng.site_pileup(20, L, L, rec, sites)                                      # a tile filtered for its own list
        refused(eng.site_attach_quals, rec, 20)
        refused(eng.site_scan_counts_ex, 20, 0, 10)
        eng.site_upload(L, L, rec)
        refused(eng.site_scan_ex, 20, 10, ref)                                     # nothing attached
        refused(eng.site_scan_counts_ex, 20, 0, 10)
        refused(eng.site_attach_quals, rec.slice(0, rec.n - 1), 20)               # another n_reads
        eng.site_attach_quals(rec, 20)
        refused(eng.site_attach_quals, rec.slice(0, 10), 20)                      # a refused attachment keeps the earlier one
        refused(eng.site_scan_ex, 20, 10, ref, 0, False, 0, L + 1)                 # end > contig_len
        refused(eng.site_scan_ex, 20, 10, ref, 0, False, 10, 9)                    # start > end
        refused(eng.site_scan_ex, 20, 0, ref)                                      # min_depth == 0
        refused(eng.site_scan_ex, 20, 10, ref[:L - 1], 0, False, 0, L)             # another ref_len
        refused(eng.site_scan_counts_ex, 20, 0, L + 1)
        h = R.stranded_hist(L, L, rec, 20, 0x704, 20)
        same_scan(eng.site_scan_ex(20, 10, ref, 0x704, True), R.reduce(h, ref, L, 10, 0, L), "after the refusals")
        assert np.array_equal(eng.site_scan_counts_ex(20, 0, L, 0x704, True), R.counts9(h))
        empty = eng.site_scan_ex(20, 10, ref, 0x704, True, 5, 5)
        assert (empty.low_depth, empty.mixed, empty.uncomparable, empty.match, empty.variant) == (0, 0, 0, 0, 0)


def test_find_variants_with_filters_on_files_and_cli(tmp_path):
    import test_haplogroup as TH
    L = 60_000
    ref = synth.make_reference(L, 31)
    rng = random.Random(21)
    ok_pos = [p for p in rng.sample(range(5_000, L - 5_000), 300) if chr(ref[p - 1]).upper() in "ACGT"]

    def fix(nodes):
        for n in nodes.values():
            for v in n["variants"]:
                if v.get("position"):
                    anc = chr(ref[abs(v["position"]) - 1]).upper()
                    v["ancestral"] = anc; v["derived"] = rng.choice([b for b in "ACGT" if b != anc])
    text = TH.ftdna_tree(rng, 80, ok_pos, extra=fix)
    tree_path = str(tmp_path / "ytree.json"); open(tree_path, "w").write(text)
    _, ot = HO.load_tree(text, "ftdna")
    sample = ref.copy()
    positions = {}
    HO.collect_snps(ot, positions, "GRCh38")
    for k, p in enumerate(sorted(positions)):
        if k % 2 == 0:
            sample[p - 1] = ord(positions[p][0][1]["coordinates"]["GRCh38"]["derived"][0])
    for p in rng.sample(range(5_000, L - 5_000), 60):
        if p not in positions and chr(ref[p - 1]).upper() in "ACGT":
            sample[p - 1] = ord(rng.choice([b for b in "ACGT" if b != chr(ref[p - 1]).upper()]))
    rec = synth.short_read_contig(L, 30, 77, with_seq=True, ref=sample)
    rec.flag = rec.flag | (np.random.default_rng(4).integers(0, 2, rec.n).astype(np.uint16) << np.uint16(4))
    names = ["chr1", "chrY", "chrM"]; lens = [248956422, L, 16569]
    bam = str(tmp_path / "y.bam"); fa = str(tmp_path / "y.fa")
    write_bam(bam, list(zip(names, lens)), {1: rec}, block_every=5000)
    write_fasta(fa, [("chrY", ref), ("chrM", synth.make_reference(16569, 32))])
    notes = {}
    for p, entries in positions.items():
        loci = sorted({(l["name"], l["coordinates"]["GRCh38"]["ancestral"], l["coordinates"]["GRCh38"]["derived"]) for _, l in entries
                       if l["coordinates"]["GRCh38"]["chromosome"] == "chrY"}, key=lambda x: tuple(s.encode() for s in x))
        if loci:
            notes[p] = loci

    def want(mq, md, mbq, ex, k, a=0, b=L, tree=True):
        exp = R.reduce(R.stranded_hist(L, L, rec, mq, ex, mbq), ref, L, md, a, b)
        nt = None
        if tree:
            nt = {}
            for c in exp["candidates"]:
                if c[0] in notes:
                    alt = c[2]
                    nt[c[0]] = (",".join(n for n, _, _ in notes[c[0]]),
                                ",".join("derived" if d[:1] == alt else "ancestral" if an[:1] == alt else "other" for _, an, d in notes[c[0]]))
        return R.expected_tsv_ex("chrY", exp, a, b, md, mq, mbq, ex, k, nt), exp

    out = str(tmp_path / "v.tsv")
    yb0 = str(tmp_path / "yb0.tsv"); yb1 = str(tmp_path / "yb1.tsv")
    H.analyze_haplogroup(bam, fa, tree_path, yb0, show_snps=True)
    w1, e1 = want(20, 10, 20, 0x704, 7)                # K = 7: some candidates have fewer on a strand, most have more
    assert e1["variant"] > 50 and "\tknown\t" in w1 and "\tnovel\t" in w1 and "\tstrand\n" in w1 and "\tPASS\n" in w1
    V.find_variants(bam, fa, "chrY", out, tree_json=tree_path, min_base_quality=20, exclude_flags=0x704, min_alt_per_strand=7)
    assert open(out).read() == w1
    V.find_variants(bam, fa, "chrY", out, exclude_flags=0x10)
    assert open(out).read() == want(20, 10, None, 0x10, 0, tree=False)[0]
    r = subprocess.run([_b.CLI, "find-variants", bam, "-r", fa, "-o", out, "-L", "chrY", "--tree", tree_path, "--min-base-quality", "20",
                        "--exclude-flags", "0x704", "--min-alt-per-strand=7"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w1
    a, b = 20_000 + 7, 41_000
    r = subprocess.run([_b.CLI, "find-variants", bam, "-r", fa, "-o", out, "-L", "chrY", f"--region={a}-{b}", "--min-depth", "12",
                        "--min-quality=30", "--exclude-flags", "1796"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == want(30, 12, None, 0x704, 0, a, b, tree=False)[0]
    r = subprocess.run([_b.CLI, "find-variants", bam, "-r", fa, "-o", out, "-L", "chrY", "--min-alt-per-strand", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == want(20, 10, None, 0, 0, tree=False)[0]
    # without the flags: the old columns, and the counts of the filter-off reference
    V.find_variants(bam, fa, "chrY", out, tree_json=tree_path)
    old = open(out).read()
    plain = R.reduce(R.stranded_hist(L, L, rec, 20), ref, L, 10, 0, L)
    assert "alt_fwd" not in old and "exclude_flags" not in old and f"##variant={plain['variant']}\n" in old
    body = [l.split("\t") for l in old.splitlines() if not l.startswith("#")]
    assert [(int(l[1]), l[2], l[3], int(l[5]), int(l[6]), int(l[7]), int(l[8]), int(l[4])) for l in body] == [c[:8] for c in plain["candidates"]]
    assert all(len(l) == 13 for l in body)
    r = subprocess.run([_b.CLI, "find-variants", bam, "-r", fa, "-o", str(tmp_path / "v2.tsv"), "-L", "chrY", "--tree", tree_path], capture_output=True, text=True)
    assert r.returncode == 0 and open(str(tmp_path / "v2.tsv")).read() == old
    H.analyze_haplogroup(bam, fa, tree_path, yb1, show_snps=True)
    assert open(yb0).read() == open(yb1).read()
