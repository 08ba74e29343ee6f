"""The dense site scan on the device (-m gpu): cl_site_scan_counts / cl_site_scan / find-variants against the CPU
oracle's site pileup with a site at every position (oracle.site_pileup), reduced with numpy here -- never against the
engine's own cl_site_run, except where the invariant between the two is what is tested.  Counts: everything is exact."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import oracle
from bamio import write_bam, write_fasta
from helpers import load_kats
from decodingustools_amd import CallableOptions, Engine, EngineError, build as _b, haplogroup as H, synth, variants as V
from decodingustools_amd._lib import CL_SCAN_MAX_DENSE
from decodingustools_amd.records import ContigRecords, pack_seq4
from oracle import haplogroup_oracle as HO

pytestmark = pytest.mark.gpu
KATS = load_kats()
W = 1024                                            # the kernel's window: ranges below start and end inside, at and across its edges
CODE = "=ACMGRSVTWYHKDBN"
ACGT_CODES = np.array([1, 2, 4, 8])


def oracle_hist(L, ref, rec, min_quality):
    return oracle.site_pileup(1, min_quality, L, ref, rec, np.arange(1, L + 1, dtype=np.uint32))["hist"]


def counts_of(hist):
    """(L, 5): A, C, G, T, depth from the oracle's 16-code histogram."""
    return np.concatenate([hist[:, [1, 2, 4, 8]], hist.sum(1, dtype=np.uint64)[:, None].astype(np.uint32)], axis=1)


def reduce_hist(hist, ref, L, min_depth, start, end):
    """Classes and candidates of [start, end) from the oracle's histogram, by the definitions of include/callable_loci.h
    with the f64 rule of caller.rs:132-149."""
    h = hist[start:end].astype(np.uint64)
    depth = h.sum(1)
    m = h.max(1)
    cstar = h.argmax(1)
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
    idx = np.nonzero(var)[0]
    cand = [(int(start + i + 1), chr(rb[i]), chr(cbase[i]), int(h[i, 1]), int(h[i, 2]), int(h[i, 4]), int(h[i, 8]), int(depth[i])) for i in idx]
    return dict(low_depth=int(low.sum()), mixed=int(mixed.sum()), uncomparable=int(unc.sum()), match=int(match.sum()),
                variant=int(var.sum()), candidates=cand, cls=np.select([low, mixed, unc, match, var], [0, 1, 2, 3, 4]))


def same_scan(got, exp, what):
    assert (got.low_depth, got.mixed, got.uncomparable, got.match, got.variant) == \
        (exp["low_depth"], exp["mixed"], exp["uncomparable"], exp["match"], exp["variant"]), what
    c = got.candidates
    have = [(int(r["pos"]), chr(r["ref"]), chr(r["alt"]), int(r["a"]), int(r["c"]), int(r["g"]), int(r["t"]), int(r["depth"])) for r in c]
    assert have == exp["candidates"], what


def ranges_for(L):
    r = [(0, L), (0, 0), (L, L), (5, 5), (0, 1), (L - 1, L), (3, 700), (W - 1, W + 1), (W, 2 * W), (W, W + 1), (1000, 3 * W + 17),
         (2 * W - 1, 2 * W), (L // 2, L)]
    return sorted({(max(0, min(a, L)), max(0, min(b, L))) for a, b in r if min(a, L) <= min(b, L)})


def check_dense(eng, L, ref_len, ref, rec, qualities=(20,), ranges=None, what=""):
    eng.site_upload(L, ref_len, rec)
    for mq in qualities:
        want = counts_of(oracle_hist(L, ref, rec, mq))
        for a, b in (ranges or ranges_for(L)):
            if b - a > CL_SCAN_MAX_DENSE:
                continue
            got = eng.site_scan_counts(mq, a, b)
            assert got.shape == (b - a, 5)
            bad = np.nonzero((got != want[a:b]).any(1))[0]
            assert bad.size == 0, (what, mq, (a, b), int(a + bad[0]), got[bad[0]].tolist(), want[a + bad[0]].tolist())
    return want


def with_random_seq(rec, seed, all_codes=True):
    """4-bit bases for records that have none: as many as the read has quality values (l_seq), any of the 16 codes."""
    rng = np.random.default_rng(seed)
    n = int(rec.qual_off[-1])
    codes = rng.integers(0, 16, n, dtype=np.uint8) if all_codes else ACGT_CODES.astype(np.uint8)[rng.integers(0, 4, n)]
    rec.seq_off = rec.qual_off.copy()
    rec.seq4 = pack_seq4(codes)
    return rec


@pytest.mark.parametrize("case", KATS["site_cases"], ids=[c["name"] for c in KATS["site_cases"]])
def test_dense_counts_site_kats(case):
    rec = ContigRecords.from_reads([tuple(r) for r in case["reads"]])
    ref = np.frombuffer(case["ref"].encode(), dtype=np.uint8).copy()
    L = case["contig_len"]
    with Engine(CallableOptions(), 0) as eng:
        check_dense(eng, L, ref.shape[0], ref, rec, qualities=(0, case["min_quality"], 61), what=case["name"])
        for md in (1, case["min_depth"]):
            for mq in (0, case["min_quality"]):
                same_scan(eng.site_scan(mq, md, ref), reduce_hist(oracle_hist(L, ref, rec, mq), ref, L, md, 0, L), (case["name"], md, mq))


@pytest.mark.parametrize("follow_ref", [True, False], ids=["reference-following", "random-bases"])
def test_dense_counts_short_reads(follow_ref):
    L = 200_000
    ref = synth.make_reference(L, 7)
    rec = synth.short_read_contig(L, 40, 11 if follow_ref else 12, with_seq=True, ref=ref if follow_ref else None)
    with Engine(CallableOptions(), 0) as eng:
        want = check_dense(eng, L, L, ref, rec, qualities=(0, 20, 61))
        # ref_len < contig_len: positions at and beyond ref_len count nothing (caller.rs:110-113)
        short = L - 3 * W - 100
        check_dense(eng, L, short, ref[:short], rec, ranges=[(0, L), (short - 5, short + 5), (short, L), (L - 2 * W, L)], what="short reference")


def test_dense_counts_adversarial_cigars_and_edges():
    """Insertions, deletions, soft and hard clips, reference skips, pads, reads without a reference span, reads with no
    bases at all (more query bases in the CIGAR than l_seq), all 16 base codes, reads that overhang the contig end, that
    start at or beyond it, and a tile that is not coordinate sorted."""
    for seed, L, n, overhang in ((1, 3000, 600, False), (2, 5000, 1500, True), (3, 2 * W, 900, True), (4, 700, 300, False)):
        rec = with_random_seq(synth.adversarial_contig(L, n, seed, overhang=overhang, deep=(seed == 2)), 100 + seed)
        ref = synth.make_reference(L, 50 + seed, lowercase=True)
        with Engine(CallableOptions(), 0) as eng:
            check_dense(eng, L, L, ref, rec, qualities=(0, 10, 61), what=("adversarial", seed))
            check_dense(eng, L, L - 300, ref[:L - 300], rec, qualities=(10,), what=("adversarial, short reference", seed))
    L = 4000
    seq = "ACGTN=MR" * 50
    reads = [(0, "50M", 60, 30, 0, "first", seq[:50]), (10, "100M", 60, 30, 0, "a", seq[:100]),
             (20, "30M", 60, 30, 0, "fewer-bases", seq[:12]),                        # l_seq 12 < 30 query bases
             (25, "10S20M5I20M3D10M2N10M5H", 60, 30, 0, "ops", seq[:75]),
             (L - 40, "100M", 60, 30, 0, "overhang", seq[:100]), (L - 1, "10M", 60, 30, 0, "last", seq[:10]),
             (L, "50M", 60, 30, 0, "at-end", seq[:50]), (L + 500, "50M", 60, 30, 0, "beyond", seq[:50]),
             (1500, "40M", 19, 30, 0, "lowq", seq[:40]), (1500, "40M", 20, 30, 0, "q20", seq[:40])]
    for order in (reads, reads[::-1], reads[3:] + reads[:3]):                        # sorted, reversed, rotated
        rec = ContigRecords.from_reads(order)
        ref = synth.make_reference(L, 9)
        with Engine(CallableOptions(), 0) as eng:
            check_dense(eng, L, L, ref, rec, qualities=(0, 20, 61), what="edges")
            check_dense(eng, L, L - 100, ref[:L - 100], rec, what="edges, short reference")


def long_cigar(n_ops, rng):
    """n_ops operations: M runs of 5-40 bases between I / D / N / =X, starting and ending on M."""
    ops = []
    while len(ops) < n_ops - 1:
        ops.append(("M", int(rng.integers(5, 40))))
        ops.append((str(rng.choice(["I", "D", "N", "X", "="])), int(rng.integers(1, 6))))
    ops = ops[:n_ops - 1] + [("M", 20)]
    fixed = []
    for o, l in ops:                                   # no two M-like neighbours merge: keep as written, BAM allows it
        fixed.append((o, l))
    return "".join(f"{l}{o}" for o, l in fixed), sum(l for o, l in fixed if o in "MIS=X")


def test_dense_counts_long_reads_and_deep_piles():
    """SiteRec's escape to the next record's offsets (255 and more CIGAR operations, 65 535 and more bases), long reads
    walked over many windows, and counters beyond 16 bits."""
    rng = np.random.default_rng(5)
    L = 90_000
    ref = synth.make_reference(L, 21)
    codes = "ACGT"
    def seq(n):
        return "".join(codes[i] for i in rng.integers(0, 4, n))
    c300, q300 = long_cigar(300, rng)
    c255, q255 = long_cigar(255, rng)
    c254, q254 = long_cigar(254, rng)
    reads = [(100, c300, 60, 30, 0, "ops300", seq(q300)), (900, c255, 60, 30, 0, "ops255", seq(q255)), (950, c254, 60, 30, 0, "ops254", seq(q254)),
             (2000, "70000M", 60, 30, 0, "b70000", seq(70000)), (2500, "65535M", 60, 30, 0, "b65535", seq(65535)),
             (3000, "65534M", 60, 30, 0, "b65534", seq(65534)), (3500, "30000M200D30000M", 33, 30, 0, "del", seq(60000))]
    # long_read_contig-shaped records (thousands of operations each) with bases added
    lr = with_random_seq(synth.long_read_contig(L, 6, 77), 78, all_codes=False)
    rec = ContigRecords.from_reads(reads)
    with Engine(CallableOptions(), 0) as eng:
        check_dense(eng, L, L, ref, rec, qualities=(0, 40), ranges=[(0, L), (W - 3, 5 * W + 9), (70 * W, L)], what="long operations")
        check_dense(eng, L, L, ref, lr, qualities=(20,), ranges=[(0, L), (10 * W + 1, 30 * W)], what="long reads")
    # 70 000 identical 50-bp reads at one start: every counter there is beyond 16 bits
    n = 70_000
    pile = ContigRecords(pos=np.full(n, 1000, np.int32), flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8),
                         cigar_off=np.arange(n + 1, dtype=np.uint32), cigar=np.full(n, (50 << 4) | 0, np.uint32),
                         qual_off=np.arange(n + 1, dtype=np.uint64) * np.uint64(50), qual=np.full(n * 50, 30, np.uint8),
                         qname_off=np.arange(n + 1, dtype=np.uint32), qname=np.full(n, ord("p"), np.uint8)).validate()
    one = np.array([1, 2, 4, 8, 15] * 10, np.uint8)
    pile.seq_off = pile.qual_off.copy()
    pile.seq4 = np.tile(pack_seq4(one), n)
    Lp = 3000
    refp = synth.make_reference(Lp, 3)
    with Engine(CallableOptions(), 0) as eng:
        want = check_dense(eng, Lp, Lp, refp, pile, qualities=(20,), ranges=[(0, Lp), (990, 1060)], what="pile")
        assert int(want[1000, 4]) == n and int(want[1000:1050, 4].min()) == n
        res = eng.site_scan(20, 10, refp)
        same_scan(res, reduce_hist(oracle_hist(Lp, refp, pile, 20), refp, Lp, 10, 0, Lp), "pile")
        assert res.uncomparable >= 10                                              # the N columns: called, not comparable


def changed_reference(ref, seed):
    """200 substitutions at random A/C/G/T positions, 20 positions set to N, a lower-case stretch, one IUPAC code."""
    rng = np.random.default_rng(seed)
    out = ref.copy()
    ok = np.nonzero(np.isin(out & np.uint8(0xDF), np.frombuffer(b"ACGT", np.uint8)))[0]
    planted = np.sort(rng.choice(ok, 200, replace=False))
    for p in planted:
        out[p] = rng.choice([b for b in b"ACGT" if b != (out[p] & 0xDF)])
    rest = np.setdiff1d(ok, planted)
    out[rng.choice(rest, 20, replace=False)] = ord("N")
    out[50_000:50_400] |= np.uint8(0x20)
    out[int(rng.choice(rest))] = ord("R")
    return out, planted


def test_scan_calls_and_candidates_against_a_changed_reference():
    L = 200_000
    ref = synth.make_reference(L, 7)
    rec = synth.short_read_contig(L, 40, 11, with_seq=True, ref=ref)
    changed, planted = changed_reference(ref, 23)
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        for mq in (20, 0):
            hist = oracle_hist(L, ref, rec, mq)
            for md in (1, 10, 30):
                exp = reduce_hist(hist, changed, L, md, 0, L)
                if (md, mq) == (10, 20):
                    # the oracle itself finds the planted differences: the comparison below cannot pass on an empty list
                    found = {c[0] - 1 for c in exp["candidates"]}
                    assert len(found & set(planted.tolist())) >= 150, len(found & set(planted.tolist()))
                same_scan(eng.site_scan(mq, md, changed), exp, (md, mq))
                for a, b in ((0, 0), (777, 778), (W - 1, 3 * W + 1), (50_000 - 10, 50_410), (L - 5000, L)):
                    same_scan(eng.site_scan(mq, md, changed, a, b), reduce_hist(hist, changed, L, md, a, b), (md, mq, a, b))
    # the random-base contig: almost nothing is called, nearly every deep position is mixed
    rnd = synth.short_read_contig(L, 40, 12, with_seq=True, ref=None)
    hist = oracle_hist(L, ref, rnd, 20)
    exp = reduce_hist(hist, ref, L, 10, 0, L)
    deep = L - exp["low_depth"]
    assert deep > L // 2 and exp["mixed"] >= 0.9 * deep
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rnd)
        same_scan(eng.site_scan(20, 10, ref), exp, "random bases")


def test_scan_settles_positions_ruled_by_other_codes():
    """Positions where the codes outside A/C/G/T/N hold 0.7 of the depth -- alone (a call of nothing comparable) or
    between them (no call): the six counter planes of the kernel cannot tell, the engine settles them exactly."""
    L = 300
    ref = synth.make_reference(L, 2)
    col = ["M" * 10, "M" * 8 + "RR", "MMMMRRRRAA", "=" * 7 + "ACG", "RRRYYYKKKA", "NNNNNNNNMM", "NNNNMMMMRR"]
    reads = [(100, f"{len(col)}M", 60, 30, 0, f"r{i}", "".join(c[i] for c in col)) for i in range(10)]
    rec = ContigRecords.from_reads(reads)
    hist = oracle_hist(L, ref, rec, 20)
    exp = reduce_hist(hist, ref, L, 5, 0, L)
    assert exp["cls"][100:107].tolist() == [2, 2, 1, 2, 1, 2, 1]
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        same_scan(eng.site_scan(20, 5, ref), exp, "other codes")
        same_scan(eng.site_scan(20, 5, ref, 101, 105), reduce_hist(hist, ref, L, 5, 101, 105), "other codes, range")


def test_scan_agrees_with_site_run_and_leaves_it_alone():
    L = 120_000
    ref = synth.make_reference(L, 31)
    sample = ref.copy()
    rng = np.random.default_rng(8)
    for p in rng.choice(L, 300, replace=False):
        sample[p] = rng.choice(list(b"ACGT"))
    rec = synth.short_read_contig(L, 30, 41, with_seq=True, ref=sample)
    sites = np.sort(rng.choice(np.arange(1, L + 1), 4000, replace=False)).astype(np.uint32)
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        before = eng.site_run(20, sites)
        res = eng.site_scan(20, 10, ref)
        counts = eng.site_scan_counts(20, 0, L)
        after = eng.site_run(20, sites)
        assert np.array_equal(before, after) and np.array_equal(before, oracle.site_pileup(10, 20, L, ref, rec, sites)["hist"])
        # the invariant: the scan's call at a site is the call dut_call_sites makes of cl_site_run's histogram there
        calls = {c.position: c for c in H.call_sites(sites, before, 10)}
        cand = {int(c["pos"]): chr(c["alt"]) for c in res.candidates}
        def scan_class(s):
            r = eng.site_scan(20, 10, ref, s - 1, s)
            k = [r.low_depth, r.mixed, r.uncomparable, r.match, r.variant]
            assert sum(k) == 1
            return k.index(1)

        n_var = 0
        for i, s in enumerate(sites.tolist()):
            cls, base = V.scan_classify_counts(counts[s - 1], ref[s - 1], 10)
            if cls == V.UNDETERMINED or i < 300:                 # (five counters do not name a majority of N: ask the scan itself)
                one = scan_class(s)
                assert cls in (one, V.UNDETERMINED), s
                cls = one
            assert (cls in (V.MATCH, V.VARIANT, V.UNCOMPARABLE)) == (s in calls), s
            if s in calls:
                assert calls[s].depth == int(counts[s - 1, 4]) and (not base or calls[s].base == base)
            assert (cls == V.VARIANT) == (s in cand)
            if cls == V.VARIANT:
                assert cand[s] == calls[s].base
            n_var += cls == V.VARIANT
        assert n_var >= 3 and len(calls) > 2000
        # two scans with different gates on one resident tile each equal the oracle, in either order
        for mq, md in ((0, 1), (30, 25), (20, 10), (0, 1)):
            same_scan(eng.site_scan(mq, md, ref), reduce_hist(oracle_hist(L, ref, rec, mq), ref, L, md, 0, L), (mq, md))
        ms, nbytes = eng.site_scan_stats()
        assert ms > 0 and nbytes > rec.seq4.shape[0]


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
        refused(eng.site_scan, 20, 10, ref)                                         # nothing resident
        refused(eng.site_scan_counts, 20, 0, 10)
        eng.site_pileup(20, L, L, rec, sites)                                       # a tile filtered for its own list
        refused(eng.site_scan, 20, 10, ref)
        refused(eng.site_scan_counts, 20, 0, 10)
        eng.site_upload(L, L, rec)
        refused(eng.site_scan, 20, 10, ref, 0, L + 1)                               # end > contig_len
        refused(eng.site_scan, 20, 10, ref, 10, 9)                                  # start > end
        refused(eng.site_scan, 20, 0, ref)                                          # min_depth == 0
        refused(eng.site_scan, 20, 10, ref[:L - 1], 0, L)                           # another ref_len
        refused(eng.site_scan_counts, 20, 0, L + 1)
        big = 3 * (1 << 20)
        same_scan(eng.site_scan(20, 10, ref), reduce_hist(oracle_hist(L, ref, rec, 20), ref, L, 10, 0, L), "after the refusals")
        assert np.array_equal(eng.site_scan_counts(20, 0, L), counts_of(oracle_hist(L, ref, rec, 20)))
        # a dense range above the limit: a longer contig with a handful of reads
        few = rec.slice(0, 50)
        eng.site_upload(big, L, few)
        refused(eng.site_scan_counts, 20, 0, CL_SCAN_MAX_DENSE + 1)
        got = eng.site_scan_counts(20, 0, CL_SCAN_MAX_DENSE)
        want = counts_of(oracle_hist(L, ref, few, 20))
        assert np.array_equal(got[:L], want) and not got[L:].any()
        res = eng.site_scan(20, 1, ref, 0, big)
        exp = reduce_hist(oracle_hist(L, ref, few, 20), ref, L, 1, 0, L)
        assert res.low_depth == exp["low_depth"] + big - L and res.variant == exp["variant"] and res.match == exp["match"]


def expected_tsv(contig, hist, ref, L, a, b, md, mq, tree=None, build=None):
    exp = reduce_hist(hist, ref, L, md, a, b)
    out = [f"##contig={contig}", f"##range={a}-{b}", f"##min_depth={md}", f"##min_quality={mq}", f"##positions={b - a}",
           f"##low_depth={exp['low_depth']}", f"##mixed={exp['mixed']}", f"##uncomparable={exp['uncomparable']}", f"##match={exp['match']}",
           f"##variant={exp['variant']}", "#contig\tpos\tref\talt\tdepth\tA\tC\tG\tT\tfreq\tstatus\tnames\talleles"]
    by_pos = {}
    if tree is not None:
        positions = {}
        HO.collect_snps(tree, positions, build)
        for p, entries in positions.items():
            loci = {(l["name"], l["coordinates"][build]["ancestral"], l["coordinates"][build]["derived"]) for _, l in entries
                    if l["coordinates"][build]["chromosome"] == contig}
            if loci:
                by_pos[p] = sorted(loci, key=lambda x: tuple(s.encode() for s in x))
    for pos, r, alt, A, C, G, T, depth in exp["candidates"]:
        freq = dict(A=A, C=C, G=G, T=T)[alt] / depth
        line = f"{contig}\t{pos}\t{r}\t{alt}\t{depth}\t{A}\t{C}\t{G}\t{T}\t{freq:.4f}\t"
        if tree is None:
            line += ".\t.\t."
        elif pos not in by_pos:
            line += "novel\t.\t."
        else:
            names = ",".join(n for n, _, _ in by_pos[pos])
            alleles = ",".join("derived" if d[:1] == alt else "ancestral" if an[:1] == alt else "other" for _, an, d in by_pos[pos])
            line += f"known\t{names}\t{alleles}"
        out.append(line)
    return "\n".join(out) + "\n", exp


def test_find_variants_on_files_and_cli(tmp_path):
    import test_haplogroup as TH
    L = 150_000
    ref = synth.make_reference(L, 31)
    rng = random.Random(21)
    ok_pos = [p for p in rng.sample(range(10_000, L - 10_000), 500) if chr(ref[p - 1]).upper() in "ACGT"]

    def fix(nodes):
        for n in nodes.values():
            for v in n["variants"]:
                if v.get("position"):
                    anc = chr(ref[abs(v["position"]) - 1]).upper()
                    v["ancestral"] = anc; v["derived"] = rng.choice([b for b in "ACGT" if b != anc])
    text = TH.ftdna_tree(rng, 120, ok_pos, extra=fix)
    tree_path = str(tmp_path / "ytree.json"); open(tree_path, "w").write(text)
    _, ot = HO.load_tree(text, "ftdna")
    # the sample: the derived allele at every second tree site, and 80 differences the tree does not know
    sample = ref.copy()
    positions = {}
    HO.collect_snps(ot, positions, "GRCh38")
    for k, p in enumerate(sorted(positions)):
        if k % 2 == 0:
            sample[p - 1] = ord(positions[p][0][1]["coordinates"]["GRCh38"]["derived"][0])
    for p in rng.sample(range(10_000, L - 10_000), 80):
        if p not in positions and chr(ref[p - 1]).upper() in "ACGT":
            sample[p - 1] = ord(rng.choice([b for b in "ACGT" if b != chr(ref[p - 1]).upper()]))
    rec = synth.short_read_contig(L, 30, 77, with_seq=True, ref=sample)
    names = ["chr1", "chrY", "chrM"]; lens = [248956422, L, 16569]        # the chr1 length marks the header as GRCh38
    bam = str(tmp_path / "y.bam"); fa = str(tmp_path / "y.fa")
    write_bam(bam, list(zip(names, lens)), {1: rec}, block_every=5000)
    write_fasta(fa, [("chrY", ref), ("chrM", synth.make_reference(16569, 32))])
    hist = oracle_hist(L, ref, rec, 20)
    want, exp = expected_tsv("chrY", hist, ref, L, 0, L, 10, 20, ot, "GRCh38")
    assert exp["variant"] > 100 and "\tknown\t" in want and "\tnovel\t" in want and "derived" in want
    out = str(tmp_path / "v.tsv")
    # find-y-branch on these files, before and after: the scan changes nothing for it
    yb0 = str(tmp_path / "yb0.tsv"); yb1 = str(tmp_path / "yb1.tsv")
    H.analyze_haplogroup(bam, fa, tree_path, yb0, show_snps=True)
    V.find_variants(bam, fa, "chrY", out, tree_json=tree_path)
    assert open(out).read() == want
    V.find_variants(bam, fa, "chrY", out)
    assert open(out).read() == expected_tsv("chrY", hist, ref, L, 0, L, 10, 20)[0]
    r = subprocess.run([_b.CLI, "find-variants", bam, "-r", fa, "-o", out, "-L", "chrY", "--tree", tree_path, "--provider", "ftdna",
                        "--tree-type", "y"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == want
    a, b = 20_000 + 7, 61_000
    r = subprocess.run([_b.CLI, "find-variants", bam, "-r", fa, "-o", out, "-L", "chrY", f"--region={a}-{b}", "--min-depth", "12",
                        "--min-quality=30", "--tree", tree_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want_r, exp_r = expected_tsv("chrY", oracle_hist(L, ref, rec, 30), ref, L, a, b, 12, 30, ot, "GRCh38")
    assert open(out).read() == want_r
    assert exp_r["low_depth"] + exp_r["mixed"] + exp_r["uncomparable"] + exp_r["match"] + exp_r["variant"] == b - a
    assert all(a < int(l.split("\t")[1]) <= b for l in want_r.splitlines() if not l.startswith("#"))
    H.analyze_haplogroup(bam, fa, tree_path, yb1, show_snps=True)
    sites, rel = HO.sites_and_relevance(ot, "GRCh38", "chrY")
    calls = HO.call_sites(sites, rel, oracle.site_pileup(10, 20, L, ref, rec, np.asarray(sites, np.uint32))["hist"], 10)
    assert open(yb0).read() == open(yb1).read() == HO.report_text(ot, calls, "GRCh38", True)[0]
    # errors with a message, exit 1: an unknown contig, a region beyond the contig
    r = subprocess.run([_b.CLI, "find-variants", bam, "-r", fa, "-o", out, "-L", "chrZ"], capture_output=True, text=True)
    assert r.returncode == 1 and "chrZ" in r.stderr
    r = subprocess.run([_b.CLI, "find-variants", bam, "-r", fa, "-o", out, "-L", "chrY", "--region", f"10-{L + 1}"], capture_output=True, text=True)
    assert r.returncode == 1 and "beyond" in r.stderr
