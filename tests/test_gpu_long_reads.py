"""error-profile, phase-sites, find-strs and the scan modes dels, ins, minor and consensus on long reads, on the device
(-m gpu): the tile of tests/long_cases.py -- reads past the base-count escape of a SiteRec, past its operation-count escape
and past 65 535 operations, reads over many windows of the scan's index, a contig of more windows than
k_site_error_profile has workgroups, pairs of sites further apart than a short read -- compared exactly with the independent
references tests/ep_ref.py, tests/link_ref.py, tests/str_ref.py and the scan modes' own; never with the engine's other calls,
except where the invariant between two calls is what is tested."""
import ctypes as C
import itertools
import random
import subprocess

import numpy as np
import pytest

import ep_ref
import link_ref
import long_cases as S
import str_ref
from bamio import write_bam, write_fasta
from decodingustools_amd import CallableOptions, Engine, _lib, build as _b, variants as V

pytestmark = pytest.mark.gpu
LC, W, REF = S.LC, S.W, S.REF


def resident(eng, case):
    eng.site_upload(LC, LC, case.rec)
    eng.site_attach_quals(case.rec, S.MBQ)


def test_long_tile_is_what_it_was_built_for():
    case = S.whole()
    bases, ops = S.check_shape(case)
    assert {254, 255, 256, 300, 66_001} <= set(ops.tolist()) and int((bases >= 65_535).sum()) >= 12
    lo, hi = case.ep_events["lo"], case.ep_events["hi"]
    assert int(((hi - 1) // W - lo // W + 1).max()) >= 64                           # a read over 64 windows of the index and more
    assert int((hi - lo).max()) > 100_000                                           # the read over the 50 000N
    assert sum(1 for r in case.reads if r[5].startswith("stack-")) == 300


# ---- error-profile -----------------------------------------------------------------------------------------------------------
def ep_run(eng, C_, mq, flt, start=0, end=LC):
    return eng.site_error_profile(C_, mq, REF, start, end, filter=flt)


@pytest.mark.parametrize("rng", S.EP_RANGES, ids=lambda r: f"{r[0]}-{r[1]}")
def test_long_ep_every_table_and_scalar_equals_the_reference(rng):
    case = S.whole()
    a, b = rng
    # the whole product over the ranges of a window or less, S.EP_COMBOS over the two of many windows
    combos = S.EP_COMBOS if b - a > 2 * W else itertools.product(S.EP_CYCLES, S.QUALS, S.EP_FILTERS)
    wants = {k: case.ep_expected(*k, a, b) for k in combos}
    assert all(w["reads"] > 0 and w["bases"] > 0 for w in wants.values())
    assert {k[0] for k in wants} == set(S.EP_CYCLES) and {k[1] for k in wants} == set(S.QUALS) and {k[2] for k in wants} == set(S.EP_FILTERS)
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        for (C_, mq, flt), want in wants.items():
            assert ep_ref.differences(ep_run(eng, C_, mq, flt, a, b), want) == [], (a, b, C_, mq, flt)


def test_long_ep_reads_that_start_before_the_range_and_cycles_of_reads_past_the_escape():
    case = S.whole()
    lo = case.ep_events["lo"]
    a, b = 66 * W, 67 * W
    mid = case.ep_expected(256, 0, None, a, b)
    assert mid["reads"] > int(((lo >= a) & (lo < b)).sum()) == 0                    # every read of that window starts before it
    # the last 256 positions of the forward read of 70 000 bases and the first 256 of the reverse one: no other read has a
    # base there within 256 of its 3' end, so these cells come from L = 70 000, on either strand
    tails = ((S.M70 + 70_000 - 256, S.M70 + 70_000), (S.R70, S.R70 + 256))
    wants = [case.ep_expected(256, 20, (0, False), x, y) for x, y in tails]
    for want in wants:
        assert int(want["from3"][0].sum()) == 1 == int(want["from3"][255].sum()) and int(want["from3"].sum()) == 256
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        assert ep_ref.differences(ep_run(eng, 256, 0, None, a, b), mid) == []
        for (x, y), want in zip(tails, wants):
            assert ep_ref.differences(ep_run(eng, 256, 20, (0, False), x, y), want) == [], (x, y)
        # additivity of every table over a split at a window border inside a read of 70 000 bases
        x, cut, y = S.EP_SPLIT
        assert cut % W == 0 and S.M70 < cut < S.M70 + 70_000
        for C_, flt in ((256, (0x704, True)), (1, None)):
            left, right, both = ep_run(eng, C_, 20, flt, x, cut), ep_run(eng, C_, 20, flt, cut, y), ep_run(eng, C_, 20, flt, x, y)
            for k in ep_ref.SCALARS[4:] + ep_ref.TABLES:
                assert np.array_equal(np.asarray(getattr(left, k)) + np.asarray(getattr(right, k)), np.asarray(getattr(both, k))), (C_, flt, k)
            assert left.reads + right.reads > both.reads > 0 and both.bases > 100_000
            assert ep_ref.differences(both, case.ep_expected(C_, 20, flt, x, y)) == []


def test_long_ep_windows_dealt_to_any_number_of_workgroups_give_identical_bytes(monkeypatch):
    case = S.whole()
    combos = [(256, 20, (0x704, True)), (1, 0, None)]
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)

        def raw(C_, mq, flt):
            """The bytes of the result record's scalars and of its context-owned arrays."""
            r = _lib.cl_ep_result()
            f = None if flt is None else C.byref(_lib.cl_scan_filter(flt[0], 1 if flt[1] else 0, 0))
            assert eng._lib.cl_site_error_profile(eng._h, mq, f, C_, REF.ctypes.data, LC, 0, LC, C.byref(r)) == 0
            return C.string_at(C.addressof(r), 16 + 7 * 8 + 16 * 8) + C.string_at(r.from5, 36 * C_ * 8)

        # the default: 256 workgroups take 264 windows
        base = {c: raw(*c) for c in combos}
        for c in combos:
            assert ep_ref.differences(ep_run(eng, *c), case.ep_expected(*c)) == [], c
            assert raw(*c) == base[c]
        # one workgroup and three take many windows each; 1000 gives 264, one window each; a small flush bound flushes between
        # windows and inside a window's read range
        for name, value in (("DUT_EP_GROUPS", "1"), ("DUT_EP_GROUPS", "3"), ("DUT_EP_GROUPS", "1000"), ("DUT_EP_FLUSH", "1024"), ("DUT_EP_FLUSH", "5000")):
            monkeypatch.setenv(name, value)
            for c in combos[:1] if value == "1" else combos:
                assert raw(*c) == base[c], (name, value, c)
            monkeypatch.delenv(name)


# ---- phase-sites -------------------------------------------------------------------------------------------------------------
def link_run(eng, D, K, mq, flt, sites=None):
    return eng.site_link_counts(np.array(S.SITES if sites is None else sites, np.uint32), D, K, mq, filter=flt)


def test_long_link_reference_shows_what_the_sites_were_planted_for():
    case = S.whole()
    sites = np.array(S.SITES, np.int64)
    assert (np.diff(sites) > 0).all()
    z = case.link_expected(2 ** 32 - 1, 15, 20, (0x704, False))
    first, t = z["first"].astype(np.int64), z["tables"].astype(np.int64)
    anchor = np.repeat(np.arange(len(sites)), np.diff(first))
    partner = anchor + 1 + np.arange(int(first[-1])) - first[anchor]
    far = (sites[partner] - sites[anchor] > 65_535) & (t.sum((1, 2)) > 0)
    assert int(far.sum()) >= 20                                                     # pairs further apart than the escape, seen by one read
    for a in (S.ANCHOR_1, S.ANCHOR_2):
        i = S.SITES.index(a)
        assert int(first[i + 1]) - int(first[i]) == 15 and (t[int(first[i]):int(first[i + 1])].sum((1, 2)) > 0).sum() >= 10
    z7 = case.link_expected(70_000, 15, 20, (0x704, False))                         # ... and the first keeps them within 70 000
    i = S.SITES.index(S.ANCHOR_1)
    assert int(z7["first"][i + 1]) - int(z7["first"][i]) == 15 and S.SITES[i + 15] - S.ANCHOR_1 == 60_000
    i = S.SITES.index(S.STACK0 + 500 + 9 * 100)
    assert int(t[int(first[i]):int(first[i + 1])].max()) > 255                      # a cell above 255 under the stack
    i = S.SITES.index(S.STACK_SITE)
    assert (t[int(first[i])].sum(1) > 20).sum() >= 2                                # ... and two alleles at the planted site
    assert t[:, link_ref.DEL, :].any() and t[:, :, link_ref.DEL].any() and (t[:, link_ref.OTHER, :].any() or t[:, :, link_ref.OTHER].any())
    # sites beyond the stored bases of the truncated read are seen by other reads, never by it
    r = case.index("m70000-with-65535-stored")
    assert S.TRUNCATED + 65_534 in case.link_events["maps"][r] and S.TRUNCATED + 65_535 not in case.link_events["maps"][r]


@pytest.mark.parametrize("pairs", S.LINK_SETS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_long_link_every_table_and_site_count_equals_the_reference(pairs):
    case = S.whole()
    D, K = pairs
    wants = {k: case.link_expected(D, K, *k) for k in S.LINK_COMBOS[pairs]}
    assert all(int(w["tables"].sum()) > 500 for w in wants.values())
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        for (mq, flt), want in wants.items():
            got = link_run(eng, D, K, mq, flt)
            assert link_ref.differences(got, want) == [], (D, K, mq, flt)


def test_long_link_tile_orders_and_the_columns_of_the_dense_scans():
    case = S.whole()
    combos = ((70_000, 15, 0, (0x704, True)), (2 ** 32 - 1, 15, 0, None))                       # (both in S.LINK_COMBOS)
    # a tile in descending coordinate order, and a shuffled one: the escape read is no longer the last record
    for order in (sorted(case.reads, key=lambda r: -r[0]), random.Random(5).sample(case.reads, len(case.reads))):
        other = S.Case(order, sort=False)
        assert other.reads[-1][5] != case.reads[-1][5]
        with Engine(CallableOptions(), 0) as eng:
            resident(eng, other)
            for D, K, mq, flt in combos:
                assert link_ref.differences(link_run(eng, D, K, mq, flt), case.link_expected(D, K, mq, flt)) == [], (D, K, mq, flt)
    sites = np.array(S.SITES, np.int64)
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        for mq in (20,):
            got = link_run(eng, 1000, 4, mq, None).site_counts.astype(np.int64)
            col = eng.site_scan_counts(mq, 0, LC).astype(np.int64)[sites]
            assert np.array_equal(got[:, :4], col[:, :4]) and np.array_equal(got[:, link_ref.OTHER], col[:, 4] - col[:, :4].sum(1)), mq
            dels = eng.site_scan_dels(mq, 1, 1, 1, REF).candidates
            listed = dict(zip((dels["pos"].astype(np.int64) - 1).tolist(), dels["del"].tolist()))
            assert got[:, link_ref.DEL].tolist() == [listed.get(int(p), 0) for p in sites] and got[:, link_ref.DEL].sum() > 0, mq
            got = link_run(eng, 1000, 4, mq, (0x704, True)).site_counts.astype(np.int64)
            col = eng.site_scan_counts_ex(mq, 0, LC, exclude_flags=0x704, use_base_quality=True).astype(np.int64)[sites]
            acgt = col[:, 0:8:2] + col[:, 1:8:2]
            assert np.array_equal(got[:, :4], acgt) and np.array_equal(got[:, link_ref.OTHER], col[:, 8] - acgt.sum(1)), mq


# ---- find-strs ---------------------------------------------------------------------------------------------------------------
def test_long_str_every_histogram_and_partial_count_equals_the_reference():
    case = S.whole()
    names = [r[5] for r in case.reads]
    # what the loci were planted for, by the reference alone: +7 and -12 in their bins, the larger gaps in `other`, the
    # skipped loci partial, a locus deep inside a read of 70 000 bases spanned
    hist, partial = case.str_expected(5, 20, None)
    for k, (s, e) in enumerate(S.LOCI):
        for name in ("ont-forward", "ont-reverse"):
            pos, marks = S.ONT[name][0], S.ONT[name][4]
            ev = case.str_events[names.index(name)]
            if (s, e) == (pos + marks["7I"] - 6, pos + marks["7I"] + 6):
                assert str_ref.measure_read(ev, s, e, 5) == (True, 7)
            if (s, e) == (pos + marks["12D"] - 4, pos + marks["12D"] + 16):
                assert str_ref.measure_read(ev, s, e, 5) == (True, -12)
            if (s, e) in ((pos + marks["70I"] - 6, pos + marks["70I"] + 6), (pos + marks["80D"] - 10, pos + marks["80D"] + 90)):
                assert str_ref.measure_read(ev, s, e, 5)[0] and int(hist[k, 0, 127]) >= 1
    skipped = case.str_events[names.index("ont-over-50000n-reverse")]
    assert not str_ref.measure_read(skipped, S.SKIP[0] + 100, S.SKIP[0] + 400, 1)[0] and int(partial[S.LOCI.index((S.SKIP[0] + 100, S.SKIP[0] + 400))]) >= 1
    assert str_ref.measure_read(case.str_events[names.index("m70000-forward")], S.M70 + 67_000, S.M70 + 68_024, 64) == (True, 0)
    assert str_ref.measure_read(case.str_events[names.index("m70000-forward")], S.M70 + 69_940, S.M70 + 69_952, 64)[0] is False
    assert int(hist[S.LOCI.index((S.STACK0 + 1100, S.STACK0 + 1112))].max()) > 200
    seen = 0
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        for flank, mq, ex in S.STR_COMBOS:
            hist, partial = case.str_expected(flank, mq, ex)
            got = eng.site_str_lengths(S.LOCI, flank, mq, filter=None if ex is None else (ex, False))
            assert got.hist.shape == hist.shape and np.array_equal(got.hist, hist), (flank, mq, ex, np.argwhere(got.hist != hist)[:3])
            assert np.array_equal(got.partial, partial), (flank, mq, ex, np.argwhere(got.partial != partial)[:3])
            seen += int(hist.sum())
    assert seen > 10_000


# ---- the scan modes dels, ins, minor and consensus ---------------------------------------------------------------------------
def test_long_scan_modes_over_reads_past_the_escape():
    from test_gpu_consensus import check_cons
    from test_gpu_del_scan import check_dels
    from test_gpu_ins_scan import check_ins
    from test_gpu_minor_scan import check_minor
    case = S.whole()
    # the gaps of the two reads of 70 000 bases with an insertion and a deletion at query index 69 800, inside two ONT-like
    # reads.  The references walk the reads that share a position with the range, in the tile's order: no other read
    # counts there, and the read of 66 001 operations costs them a second each.
    a, b = S.GAPPED[0] + S.GAP_AT - 800, S.GAPPED[1] + S.GAP_AT + 400
    lo, hi = case.ep_events["lo"], case.ep_events["hi"]
    over = [case.reads[i] for i in np.nonzero((lo < b) & (hi > a))[0]]
    assert {"m70000-gaps-past-the-escape", "m70000-gaps-past-the-escape-reverse", "ont-over-50000n-reverse", "ont-leading-3h-5000s-reverse"} <= {r[5] for r in over}
    rec = S.Case(over, sort=False).rec
    flt = [(0x704, True)]
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        assert check_dels(eng, LC, REF, rec, 20, S.MBQ, filters=flt, params=[(1, 1, 1)], ranges=[(a, b)], what="long") > 100
        assert check_ins(eng, LC, REF, rec, 20, S.MBQ, filters=flt, params=[(1, 1, 1)], ranges=[(a, b)], what="long") > 100
        assert check_minor(eng, LC, REF, rec, 20, S.MBQ, filters=flt, params=[(2, 1, 500)], ranges=[(a, b)], what="long") > 0
        seen = check_cons(eng, LC, REF, rec, 20, S.MBQ, [None] + flt, params=[(2, 1, 2000)], ranges=[(a, b)], what="long")
        assert seen.get("-", 0) > 50 and sum(seen.get(c, 0) for c in "ACGT") > 1000
        # the carriers themselves: the deletion and the insertion of the forward read at query index 69 799
        p = S.GAPPED[0] + S.GAP_AT
        dels = eng.site_scan_dels(0, 1, 1, 1, REF, p - 1, p + 4).candidates
        assert {p, p + 1, p + 2} <= set((dels["pos"].astype(np.int64) - 1).tolist())


# ---- files -------------------------------------------------------------------------------------------------------------------
def test_long_reads_on_files_and_cli(tmp_path):
    case = S.reduced()
    bases, ops = S.check_shape(case, ends=False)
    assert 500_000 < int(bases.sum()) < 900_000
    names = ["chr1", "chrL", "chrY"]; lens = [248956422, LC, 57227415]
    bam = str(tmp_path / "s.bam"); fa = str(tmp_path / "s.fa")
    write_bam(bam, list(zip(names, lens)), {1: case.rec}, block_every=5, long_cigar_tag=True)      # more than 65 535 operations go to CG
    write_fasta(fa, [("chrL", REF)])
    out = str(tmp_path / "o.tsv")

    def cli(sub, *args):
        r = subprocess.run([_b.CLI, sub, bam, "-r", fa, "-o", out, "-L", "chrL"] + list(args), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return open(out).read()

    # error-profile
    z = case.ep_expected(256, 20, (0x704, True))
    want = ep_ref.expected_tsv("chrL", z, 20, S.MBQ, 0x704)
    assert z["bases"] > 500_000 and z["ins"] > 10_000 and z["dels"] > 10_000
    assert cli("error-profile", "--cycles=256", "--min-base-quality", str(S.MBQ), "--exclude-flags", "0x704") == want
    V.error_profile(bam, fa, "chrL", out, cycles=256, min_base_quality=S.MBQ, exclude_flags=0x704)
    assert open(out).read() == want
    # phase-sites
    sf = str(tmp_path / "sites.tsv")
    open(sf, "w").write("#contig\tpos\n" + "".join(f"chrL\t{s + 1}\n" for s in S.SITES))
    z = case.link_expected(70_000, 15, 20, (0, False))
    want = link_ref.expected_tsv("chrL", S.SITES, z, 0, 70_000, 15, 2, 20, 1, 500, None, 0)
    assert int(z["tables"].sum()) > 500
    assert cli("phase-sites", "--sites", sf, "--max-dist", "70000", "--max-partners", "15", "--min-depth", "2", "--min-link-count", "1") == want
    V.phase_sites(bam, fa, "chrL", sf, out, max_dist=70_000, max_partners=15, min_depth=2, min_link_count=1)
    assert open(out).read() == want
    # find-strs
    lf = str(tmp_path / "loci.tsv")
    loci = [dict(start=s, end=e, period=4, name=f"locus-{k}") for k, (s, e) in enumerate(S.LOCI)]
    open(lf, "w").write("".join(f"chrL\t{l['start']}\t{l['end']}\t{l['period']}\t{l['name']}\n" for l in loci))
    hist, partial = case.str_expected(5, 20, 0x704)
    want = str_ref.expected_tsv("chrL", loci, 0, hist, partial, 5, 1, 20, 0x704, 7000)
    assert int(hist.sum()) > 20
    assert cli("find-strs", "--loci", lf, "--min-depth", "1", "--exclude-flags", "0x704") == want
    V.find_strs(bam, fa, "chrL", lf, out, min_depth=1, exclude_flags=0x704)
    assert open(out).read() == want
