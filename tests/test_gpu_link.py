"""Linked sites on the device (-m gpu): cl_site_link_counts in both forms and phase-sites; first, every table and every
site count compared exactly with the independent reference tests/link_ref.py (reads expanded into position -> observation
maps, counted from those) on the planted and random inputs of tests/link_cases.py -- never with the engine's own host
route or other calls, except where the invariant between two calls is what is tested."""
import ctypes as C
import itertools
import random
import subprocess

import numpy as np
import pytest

import link_cases as S
import link_ref as R
from bamio import write_bam, write_fasta
from decodingustools_amd import CallableOptions, Engine, EngineError, _lib, build as _b, synth, variants as V
from decodingustools_amd.callable_loci import HostStage
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu
L = S.L
REF = np.frombuffer((b"ACGT" * (L // 4)), np.uint8).copy()                          # the scans the identities are held against want one


def resident(eng, case, mbq=S.MBQ):
    eng.site_upload(L, L, case.rec)
    eng.site_attach_quals(case.rec, mbq)


def run(eng, case, D, K, mq, flt, sites=None):
    return eng.site_link_counts(case.sites if sites is None else sites, D, K, mq, filter=flt)


@pytest.mark.parametrize("which", ["planted", "random-1", "random-2", "random-3"])
def test_link_every_table_and_site_count_equals_the_reference(which):
    case, (D, K) = {name: (c, dk) for name, c, dk in S.all_cases()}[which]
    if which != "planted":
        assert S.hollow(case, D, K) is None                                        # on the reference's output alone, before the device is asked
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        for mq, flt in itertools.product(S.QUALS, S.FILTERS):
            got = run(eng, case, D, K, mq, flt)
            assert R.differences(got, case.expected(D, K, mq, flt)) == [], (which, mq, flt)
        assert got.kernel_ms > 0
        # other pair sets over the same sites
        for d, k in ((1, 1), (7, 2), (1000, 4)):
            assert R.differences(run(eng, case, d, k, 20, (0x704, True)), case.expected(d, k, 20, (0x704, True))) == [], (which, d, k)


def test_link_single_reads_alone_on_a_tile_give_their_hand_derived_counts():
    import test_link_host as H
    with Engine(CallableOptions(), 0) as eng:
        for name, read, sites, flt, mq, seen in S.PINS:
            rec = ContigRecords.from_reads([read])
            eng.site_upload(L, L, rec)
            eng.site_attach_quals(rec, S.MBQ)
            got = eng.site_link_counts(sites, S.PIN_D, S.PIN_K, mq, filter=flt)
            assert R.differences(got, S.pin_expected(sites, seen)) == [], name
        # the reads of the golden file together
        kat = H.KAT
        rec = H.kat_records()
        eng.site_upload(kat["contig_len"], kat["contig_len"], rec)
        eng.site_attach_quals(rec, 0)
        got = eng.site_link_counts(kat["sites"], kat["max_dist"], kat["max_partners"], kat["min_quality"], filter=(kat["exclude_flags"], False))
        assert R.differences(got, H.kat_counts()) == []


def test_link_shapes_of_the_pair_set_and_of_the_tile():
    case = S.planted()
    sites = [int(s) for s in case.sites]
    flt = (0x704, False)                                                            # (no base-quality threshold: the deep pair keeps its reads)
    whole = case.expected(S.PIN_D, S.PIN_K, 20, flt)
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        got = run(eng, case, S.PIN_D, S.PIN_K, 20, flt)
        assert R.differences(got, whole) == []
        # an anchor with exactly 15 partners and a 16th site within max_dist; anchors without partners, with and without reads
        k = sites.index(S.CLUSTER[0])
        assert int(got.first[k + 1]) - int(got.first[k]) == 15 and sites[k + 16] - sites[k] <= S.PIN_D and got.tables[int(got.first[k]) + 14].sum() > 0
        for lonely, reads in ((S.LONELY, True), (S.EMPTY, False)):
            j = sites.index(lonely)
            assert int(got.first[j + 1]) == int(got.first[j]) and (int(got.site_counts[j].sum()) > 10) == reads
        # 700 reads over one pair: a cell past 255, most reads on one cell
        i = sites.index(S.DEEP[0])
        deep = got.tables[int(got.first[i])].astype(np.int64)
        assert deep[0, 1] > 255 and deep.sum() > 512 and deep[0, 1] > deep.sum() // 2
        # anchors at 1023 and 1024 with partners across the window border
        for a in (1023, 1024):
            j = sites.index(a)
            assert sites[j + 1] // S.W == 1 and got.tables[int(got.first[j])].sum() > 10
        # no sites: an empty result without a launch; one site: its counts alone
        none = run(eng, case, S.PIN_D, S.PIN_K, 20, flt, sites=[])
        assert none.first.tolist() == [0] and none.tables.shape == (0, 6, 6) and none.site_counts.shape == (0, 6) and eng.site_scan_stats()[0] == 0.0
        one = run(eng, case, S.PIN_D, S.PIN_K, 20, flt, sites=[S.DEEP[0]])
        assert one.first.tolist() == [0, 0] and one.tables.shape == (0, 6, 6) and np.array_equal(one.site_counts[0], whole["site_counts"][i])
    # a tile in descending coordinate order, and a shuffled one: wider read ranges, the same counts
    for order in (sorted(case.reads, key=lambda r: -r[0]), random.Random(5).sample(case.reads, len(case.reads))):
        other = S.Case(order, case.sites, sort=False)
        with Engine(CallableOptions(), 0) as eng:
            resident(eng, other)
            for mq, f in ((20, (0x704, True)), (0, None)):
                assert R.differences(run(eng, other, S.PIN_D, S.PIN_K, mq, f), case.expected(S.PIN_D, S.PIN_K, mq, f)) == [], (mq, f)


def test_link_site_counts_are_the_columns_of_the_dense_scans():
    for case, (D, K) in ((S.planted(), (S.PIN_D, S.PIN_K)), (S.randomised(2), S.RANDOM_SETS[2])):
        sites = case.sites.astype(np.int64)
        with Engine(CallableOptions(), 0) as eng:
            resident(eng, case)
            for mq in S.QUALS:
                got = run(eng, case, D, K, mq, None).site_counts.astype(np.int64)
                col = eng.site_scan_counts(mq, 0, L).astype(np.int64)[sites]
                assert np.array_equal(got[:, :4], col[:, :4]) and np.array_equal(got[:, R.OTHER], col[:, 4] - col[:, :4].sum(1)), mq
                dels = eng.site_scan_dels(mq, 1, 1, 1, REF).candidates
                listed = dict(zip((dels["pos"].astype(np.int64) - 1).tolist(), dels["del"].tolist()))
                assert got[:, R.DEL].tolist() == [listed.get(int(p), 0) for p in sites] and got[:, R.DEL].sum() > 0, mq
                for ex, bq in ((0, False), (0x704, False), (0x704, True)):
                    got = run(eng, case, D, K, mq, (ex, bq)).site_counts.astype(np.int64)
                    col = eng.site_scan_counts_ex(mq, 0, L, exclude_flags=ex, use_base_quality=bq).astype(np.int64)[sites]
                    acgt = col[:, 0:8:2] + col[:, 1:8:2]
                    assert np.array_equal(got[:, :4], acgt) and np.array_equal(got[:, R.OTHER], col[:, 8] - acgt.sum(1)), (mq, ex, bq)
                    dels = eng.site_scan_dels(mq, 1, 1, 1, REF, filter=(ex, bq)).candidates
                    listed = dict(zip((dels["pos"].astype(np.int64) - 1).tolist(), dels["del"].tolist()))
                    assert got[:, R.DEL].tolist() == [listed.get(int(p), 0) for p in sites], (mq, ex, bq)


def test_link_a_pairs_table_does_not_depend_on_the_rest_of_the_call():
    case = S.randomised(1)
    D, K = S.RANDOM_SETS[1]
    sites = [int(s) for s in case.sites]
    flt = (0x704, True)
    rng = random.Random(12)
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        whole = run(eng, case, D, K, 20, flt)
        by_pair = {(sites[i], sites[i + 1 + p - int(whole.first[i])]): whole.tables[p] for i in range(len(sites)) for p in range(int(whole.first[i]), int(whole.first[i + 1]))}
        by_site = {s: whole.site_counts[i] for i, s in enumerate(sites)}
        seen = 0
        for d, k in ((D, K), (60, 3), (9, 15), (1000, 1)):
            some = sorted(rng.sample(sites, len(sites) // 2))
            got = run(eng, case, d, k, 20, flt, sites=some)
            assert np.array_equal(got.first, R.pair_set(some, d, k))
            for i in range(len(some)):
                assert np.array_equal(got.site_counts[i], by_site[some[i]])
                for p in range(int(got.first[i]), int(got.first[i + 1])):
                    pair = (some[i], some[i + 1 + p - int(got.first[i])])
                    if pair in by_pair:
                        assert np.array_equal(got.tables[p], by_pair[pair]), (d, k, pair)
                        seen += int(got.tables[p].sum() > 0)
        assert seen > 20


def test_link_interleaves_with_the_scans_builds_the_index_itself_and_repeats_its_bytes():
    case = S.planted()
    D, K, flt = S.PIN_D, S.PIN_K, (0x704, True)
    loci = [(5990, 6005), (2990, 3030)]
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        first = run(eng, case, D, K, 20, flt)                                       # the first call on a fresh tile builds the index itself
        assert R.differences(first, case.expected(D, K, 20, flt)) == [] and first.kernel_ms > 0
        ms, nbytes = eng.site_scan_stats()
        assert ms == first.kernel_ms and nbytes >= 4 * (first.tables.size + first.site_counts.size)
        scan0 = eng.site_scan(20, 10, REF)
        str0 = eng.site_str_lengths(loci, 5, 20, filter=(0x704, False))
        ep0 = eng.site_error_profile(7, 20, REF, filter=flt)

        def raw(mq, f):
            """The result record's counts and the bytes of its three context-owned arrays."""
            r = _lib.cl_link_result()
            ff = None if f is None else C.byref(_lib.cl_scan_filter(f[0], 1 if f[1] else 0, 0))
            assert eng._lib.cl_site_link_counts(eng._h, mq, ff, case.sites.ctypes.data, len(case.sites), D, K, C.byref(r)) == 0
            return r, (int(r.n_sites), int(r.n_pairs), C.string_at(r.first, 4 * (int(r.n_sites) + 1)), C.string_at(r.tables, 144 * int(r.n_pairs)),
                       C.string_at(r.site_counts, 24 * int(r.n_sites)))

        r, keep = raw(20, flt)
        assert keep[2] == first.first.tobytes() and keep[3] == first.tables.tobytes() and keep[4] == first.site_counts.tobytes()
        # the other calls leave this call's arrays alone, and it leaves their results alone
        scan1 = eng.site_scan(20, 10, REF)
        dels = eng.site_scan_dels(20, 1, 1, 1, REF, filter=flt)
        str1 = eng.site_str_lengths(loci, 5, 20, filter=(0x704, False))
        ep1 = eng.site_error_profile(7, 20, REF, filter=flt)
        hist = eng.site_run(20, case.sites + 1)
        assert keep[3] == C.string_at(r.tables, 144 * int(r.n_pairs)) and keep[4] == C.string_at(r.site_counts, 24 * int(r.n_sites))
        assert raw(20, flt)[1] == keep and raw(20, flt)[1] == keep                  # two calls return equal bytes
        assert raw(0, None)[1] != keep
        assert (scan0.low_depth, scan0.mixed, scan0.match, scan0.variant) == (scan1.low_depth, scan1.mixed, scan1.match, scan1.variant)
        assert np.array_equal(scan0.candidates, scan1.candidates) and dels.deleted >= 3 and int(hist.sum()) > 1000
        assert np.array_equal(str0.hist, str1.hist) and np.array_equal(str0.partial, str1.partial) and int(str0.hist.sum()) > 100
        assert ep0.tables_equal(ep1) and ep0.bases > 10_000
        assert R.differences(run(eng, case, D, K, 0, None), case.expected(D, K, 0, None)) == []
        assert np.array_equal(eng.site_scan(20, 10, REF).candidates, scan0.candidates)


def test_link_refusals_leave_the_context_usable():
    case = S.planted()
    D, K = S.PIN_D, S.PIN_K

    def refused(*a, **k):
        with pytest.raises(EngineError) as e:
            eng.site_link_counts(*a, **k)
        assert e.value.status == -1 and len(str(e.value)) > len(" (cl_status -1)") + 10, str(e.value)
        return str(e.value)

    with Engine(CallableOptions(), 0) as eng:
        refused(case.sites, D, K, 20)                                               # nothing resident
        eng.site_pileup(20, L, L, S.randomised(1).rec, np.arange(1, 2000, 7, dtype=np.uint32))
        assert "cl_site_pileup" in refused(case.sites, D, K, 20)                    # a tile filtered for its own list
        eng.site_upload(L, L - 100, case.rec)                                       # a reference shorter than the contig
        assert "attach" in refused(case.sites, D, K, 20, filter=(0, False))         # a filter with nothing attached
        assert str(L - 100) in refused([5, L - 100], D, K, 20) and "site 1" in refused([5, L - 100], D, K, 20)
        ok = eng.site_link_counts([5, L - 101], D, K, 20)                           # the unfiltered form needs no attachment
        assert ok.first.tolist() == [0, 0, 0]
        eng.site_upload(L, L, case.rec)
        eng.site_attach_quals(case.rec, S.MBQ)
        for form in (None, (0x704, True)):
            assert "max_dist" in refused(case.sites, 0, K, 20, filter=form)
            assert "max_partners" in refused(case.sites, D, 0, 20, filter=form)
            assert "max_partners" in refused(case.sites, D, 16, 20, filter=form)
            assert "site 2" in refused([10, 20, 20, 30], D, K, 20, filter=form)     # not strictly ascending: the index is named
            assert "site 1" in refused([10, 9], D, K, 20, filter=form)
            assert "site 1" in refused([10, L], D, K, 20, filter=form)              # beyond the contig
        out = _lib.cl_link_result()
        one = np.array([5], np.uint32)
        assert eng._lib.cl_site_link_counts(eng._h, 20, None, None, 1, D, K, C.byref(out)) == -1 and b"null sites" in eng._lib.cl_last_error(eng._h)
        assert eng._lib.cl_site_link_counts(eng._h, 20, None, one.ctypes.data, 1, D, K, None) == -1 and eng._lib.cl_last_error(eng._h)
        assert eng._lib.cl_site_link_counts(eng._h, 20, None, one.ctypes.data, _lib.CL_LINK_MAX_SITES + 1, D, K, C.byref(out)) == -1
        assert b"CL_LINK_MAX_SITES" in eng._lib.cl_last_error(eng._h)
        # a pair set above the limit: 70 000 sites with 15 partners each; the message gives the count
        many = np.arange(70_000, dtype=np.uint32)
        with Engine(CallableOptions(), 0) as big:
            big.site_upload(70_000, 70_000, case.rec)
            with pytest.raises(EngineError) as e:
                big.site_link_counts(many, 1000, 15, 20)
            n_pairs = (70_000 - 15) * 15 + sum(range(15))                           # every site but the last fifteen has fifteen partners
            assert e.value.status == -1 and n_pairs > _lib.CL_LINK_MAX_PAIRS and str(n_pairs) in str(e.value)
            assert big.site_link_counts(many, 1000, 14, 20).tables.shape[0] == (70_000 - 14) * 14 + sum(range(14))
        # the next good calls succeed and equal the reference
        for mq, flt in ((20, None), (0, (0x704, True)), (20, (0, False))):
            assert R.differences(run(eng, case, D, K, mq, flt), case.expected(D, K, mq, flt)) == [], (mq, flt)
    with HostStage(CallableOptions()) as hs:
        with pytest.raises(EngineError) as e:
            hs.site_link_counts(case.sites, D, K, 20)
        assert e.value.status == -2


# ---- phase-sites on files ---------------------------------------------------------------------------------------------------
def phased_sample(seed=81, Lc=20_000, rl=100, n=2400):
    """Reads of rl matched bases over a reference of their own, half of them reverse, a few duplicates, 600 of them over each
    of three pairs of sites.  Planted (0-based): at 5000 and 5040 the same reads, one in five, carry T and G where the others
    have the reference's A (cis); at 9000 and 9030 one read in five carries C at the first and another read in five G at the
    second (trans); at 12000 one read in five carries C and at 12050 a single read T, far below min_link_count (unresolved);
    16000 and 16010 lie under four reads (low_depth)."""
    ref = synth.make_reference(Lc, seed)
    text = bytearray(bytes(ref & 0xDF))
    for p in (5000, 5040, 9000, 9030, 12000, 12050, 16000, 16010):
        text[p] = ord("A")
    text = text.decode()
    rng = random.Random(seed)
    reads = []
    starts = [rng.randint(lo, lo + 80) for lo in (4920, 8930, 11_920) for _ in range(600)] + [rng.randint(0, 15_000 - rl) for _ in range(n - 1804)]
    starts += [15_950, 15_955, 15_960, 15_965]
    for i, p in enumerate(starts):
        seq = list(text[p:p + rl])

        def plant(site, base):
            if p <= site < p + rl:
                seq[site - p] = base
        if i % 5 == 0:
            plant(5000, "T"); plant(5040, "G"); plant(9000, "C"); plant(12000, "C")
        if i % 5 == 1:
            plant(9030, "G")
        reads.append((p, f"{rl}M", 60, 30, (0x10 if i & 1 else 0) | (0x400 if rng.random() < 0.03 else 0), f"p{i}", "".join(seq)))
    s = list(text[11_990:11_990 + rl]); s[60] = "T"
    reads.append((11_990, f"{rl}M", 60, 30, 0, "lone", "".join(s)))
    reads.sort(key=lambda r: r[0])
    return np.frombuffer(text.encode(), np.uint8).copy(), ContigRecords.from_reads(reads)


def test_phase_sites_on_files_and_cli(tmp_path):
    Lc = 20_000
    ref, rec = phased_sample()
    names = ["chr1", "chrM", "chrY"]; lens = [248956422, Lc, 57227415]
    bam = str(tmp_path / "s.bam"); fa = str(tmp_path / "s.fa")
    write_bam(bam, list(zip(names, lens)), {1: rec}, block_every=500)
    write_fasta(fa, [("chrM", ref)])
    sites = [5000, 5040, 9000, 9030, 12000, 12050, 16000, 16010]
    sf = str(tmp_path / "sites.tsv")
    open(sf, "w").write("#contig\tpos\tnote\n" + "".join(f"chrM\t{s + 1}\tx\n" for s in reversed(sites)) + "chrY\t77\n" + f"chrM\t{sites[0] + 1}\n")
    ev = R.expand(rec)

    def want(D=1000, K=4, depth=10, mq=20, links=3, disc=500, bq=None, ex=0):
        z = R.counts(ev, rec, Lc, sites, D, K, mq, ex, bq)
        return z, R.expected_tsv("chrM", sites, z, 1, D, K, depth, mq, links, disc, bq, ex)

    out = str(tmp_path / "o.tsv"); fi = str(tmp_path / "fi.tsv"); lib_out = str(tmp_path / "w.tsv")

    def cli(sub, *args, o=out):
        return subprocess.run([_b.CLI, sub, bam, "-r", fa, "-o", o, "-L", "chrM"] + list(args), capture_output=True, text=True)

    def other():
        r = cli("find-variants", o=fi)
        assert r.returncode == 0, r.stderr
        return open(fi).read()

    before = other()
    z, w0 = want(D=60, K=1)
    # the sample shows what was planted, by the reference's own summary
    status = {(int(l.split("\t")[1]) - 1, int(l.split("\t")[2]) - 1): l.rstrip("\n").split("\t")[-1] for l in w0.splitlines() if not l.startswith("#")}
    assert status == {(5000, 5040): "cis", (9000, 9030): "trans", (12000, 12050): "unresolved", (16000, 16010): "low_depth"}
    r = cli("phase-sites", "--sites", sf, "--max-dist", "60", "--max-partners", "1")
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w0
    V.phase_sites(bam, fa, "chrM", sf, out, max_dist=60, max_partners=1)
    assert open(out).read() == w0
    got = V.link_measure(rec, Lc, sites, 60, 1, 20, exclude_flags=0)
    V.write_links(lib_out, "chrM", sites, got, sites_skipped=1, max_dist=60, max_partners=1)
    assert open(lib_out).read() == w0
    # the defaults (every pair within 1000 positions, four partners), and every flag
    r = cli("phase-sites", "--sites", sf)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == want()[1]
    z1, w1 = want(D=50, K=15, depth=25, mq=0, links=2, disc=1250, bq=13, ex=0x704)
    assert w1 != w0 and "##exclude_flags=0x0704" in w1 and "##min_base_quality=13" in w1 and "##max_discordance=0.1250" in w1
    r = cli("phase-sites", "--sites", sf, "--max-dist=50", "--max-partners", "15", "--min-depth", "25", "--min-quality", "0", "--min-link-count", "2",
            "--max-discordance", "0.125", "--min-base-quality", "13", "--exclude-flags", "0x704")
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w1
    V.phase_sites(bam, fa, "chrM", sf, out, max_dist=50, max_partners=15, min_depth=25, min_quality=0, min_link_count=2, max_discordance="0.125",
                  min_base_quality=13, exclude_flags=0x704)
    assert open(out).read() == w1
    # the other subcommands write the bytes they wrote before
    assert other() == before
    # exit 1 with a message: an unknown contig, a site beyond the contig, a pair set above the limit
    r = subprocess.run([_b.CLI, "phase-sites", bam, "-r", fa, "-o", out, "-L", "chrZ", "--sites", sf], capture_output=True, text=True)
    assert r.returncode == 1 and "chrZ" in r.stderr
    far = str(tmp_path / "far.tsv")
    open(far, "w").write(f"chrM\t{Lc}\nchrM\t{Lc + 1}\n")
    r = cli("phase-sites", "--sites", far)
    assert r.returncode == 1 and "beyond" in r.stderr
    with pytest.raises(EngineError):
        V.phase_sites(bam, fa, "chrM", far, out)
    many = str(tmp_path / "many.tsv")
    open(many, "w").write("".join(f"chr1\t{p}\n" for p in range(1, 70_002)))
    r = subprocess.run([_b.CLI, "phase-sites", bam, "-r", fa, "-o", out, "-L", "chr1", "--sites", many, "--max-partners", "15"], capture_output=True, text=True)
    assert r.returncode == 1 and "pairs" in r.stderr
