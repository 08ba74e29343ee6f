"""The error profile on the device (-m gpu): cl_site_error_profile in both forms and error-profile; every table and scalar
compared exactly with the independent reference tests/ep_ref.py (reads expanded into per-base and per-event records, counted
from those) on the planted and random inputs of tests/ep_cases.py -- never with the engine's own other calls, except where
the invariant between two calls is what is tested."""
import ctypes as C
import itertools
import json
import os
import random
import subprocess

import numpy as np
import pytest

import ep_cases as S
import ep_ref as R
from bamio import write_bam, write_fasta
from decodingustools_amd import CallableOptions, Engine, EngineError, ErrorProfile, _lib, build as _b, synth, variants as V
from decodingustools_amd.callable_loci import HostStage
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu
L = S.L
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resident(eng, case, mbq=S.MBQ):
    eng.site_upload(L, case.ref_len, case.rec)
    eng.site_attach_quals(case.rec, mbq)


def run(eng, case, C_, mq, flt, start=0, end=L):
    return eng.site_error_profile(C_, mq, case.ref, start, end, filter=flt)


@pytest.mark.parametrize("which", ["planted", "planted-short-reference", "random-1", "random-2"])
def test_ep_every_table_and_scalar_equals_the_reference(which):
    case = dict(S.all_cases())[which]
    seen = 0
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        for C_, mq, flt in itertools.product(S.CYCLES, S.QUALS, S.FILTERS):
            want = case.expected(C_, mq, flt)
            got = run(eng, case, C_, mq, flt)
            assert R.differences(got, want) == [], (which, C_, mq, flt)
            seen += want["bases"]
        # ranges that start and end mid-window, one window exactly, two positions over a border, an empty one
        for (a, b), (C_, flt) in itertools.product(S.RANGES, ((7, None), (256, (0x704, True)))):
            assert R.differences(run(eng, case, C_, 20, flt, a, b), case.expected(C_, 20, flt, a, b)) == [], (which, a, b, C_, flt)
    assert seen > 100_000


def test_ep_single_reads_alone_on_a_tile_give_their_hand_derived_tables():
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "ep_kat.json")))
    with Engine(CallableOptions(), 0) as eng:
        for name, read, flt, want in S.PINS:
            rec = ContigRecords.from_reads([read])
            eng.site_upload(S.PIN_L, S.PIN_L, rec)
            eng.site_attach_quals(rec, S.MBQ)
            got = eng.site_error_profile(S.PIN_C, 20, S.PIN_REF, filter=flt)
            assert R.differences(got, S.pin_expected(want)) == [], name
        # the two reads of the golden file together, and the bytes of its TSV from the device's tables
        import test_ep_host as H
        rec = H.kat_records()
        eng.site_upload(kat["contig_len"], kat["contig_len"], rec)
        eng.site_attach_quals(rec, 0)
        got = eng.site_error_profile(kat["n_cycles"], kat["min_quality"], np.frombuffer(kat["ref"].encode(), np.uint8), filter=(kat["exclude_flags"], False))
        assert R.differences(got, H.kat_profile()) == []


def test_ep_tile_order_hooks_and_repeatability(monkeypatch, tmp_path):
    case = S.planted()
    combos = [(7, 20, None), (256, 20, (0x704, True)), (201, 0, (0, False))]
    # a tile in descending coordinate order, and a shuffled one: wider read ranges, the same counts
    for order in (sorted(case.reads, key=lambda r: -r[0]), random.Random(5).sample(case.reads, len(case.reads))):
        other = S.Case(order, case.ref_len, sort=False)
        with Engine(CallableOptions(), 0) as eng:
            resident(eng, other)
            for C_, mq, flt in combos:
                assert R.differences(run(eng, other, C_, mq, flt), case.expected(C_, mq, flt)) == [], (C_, mq, flt)
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)

        def raw(C_, mq, flt, start=0, end=L):
            """The bytes of the result record's scalars and of its context-owned arrays."""
            r = _lib.cl_ep_result()
            f = None if flt is None else C.byref(_lib.cl_scan_filter(flt[0], 1 if flt[1] else 0, 0))
            assert eng._lib.cl_site_error_profile(eng._h, mq, f, C_, case.ref.ctypes.data, case.ref_len, start, end, C.byref(r)) == 0
            return C.string_at(C.addressof(r), 16 + 7 * 8 + 16 * 8) + C.string_at(r.from5, 36 * C_ * 8)

        base = {c: raw(*c) for c in combos}
        # two calls return identical bytes, and the six arrays are one block in the order of the record
        for c in combos:
            assert raw(*c) == base[c]
        # one workgroup and three take many windows each; a small flush bound flushes between windows and inside a window's
        # read range (2048: one piece of two reads at a time; 5000: four)
        for name, value in (("DUT_EP_GROUPS", "1"), ("DUT_EP_GROUPS", "3"), ("DUT_EP_FLUSH", "2048"), ("DUT_EP_FLUSH", "5000")):
            monkeypatch.setenv(name, value)
            for c in combos:
                assert raw(*c) == base[c], (name, value, c)
            assert raw(7, 20, (0x704, True), 500, 3100) == raw(7, 20, (0x704, True), 500, 3100)
            monkeypatch.delenv(name)
        monkeypatch.setenv("DUT_EP_GROUPS", "2")
        monkeypatch.setenv("DUT_EP_FLUSH", "1024")
        for c in combos:
            assert raw(*c) == base[c], c


def test_ep_invariants_between_calls():
    for case in (S.planted(), S.randomised(2)):
        with Engine(CallableOptions(), 0) as eng:
            resident(eng, case)
            for (a, b), mq in itertools.product(((0, L), (500, 3100), (4090, L)), S.QUALS):
                # every aligned base is a unit of the scan's depth under the same gates
                got = run(eng, case, 7, mq, None, a, b)
                assert got.bases + got.uncomparable == int(eng.site_scan_counts(mq, a, b)[:, 4].astype(np.uint64).sum()), (a, b, mq)
                for ex, bq in ((0, False), (0x704, False), (0x704, True)):
                    got = run(eng, case, 7, mq, (ex, bq), a, b)
                    depth = eng.site_scan_counts_ex(mq, a, b, exclude_flags=ex, use_base_quality=bq)[:, 8]
                    assert got.bases + got.uncomparable == int(depth.astype(np.uint64).sum()), (a, b, mq, ex, bq)
            # C at and above the longest read: the cycle tables each add up to total, cell by cell, and the events to their counts
            for C_, flt in ((201, (0x704, True)), (256, None)):
                got = run(eng, case, C_, 20, flt)
                assert np.array_equal(got.from5.sum(0), got.total) and np.array_equal(got.from3.sum(0), got.total) and got.bases == int(got.total.sum())
                assert int(got.ins5.sum()) == got.ins == int(got.ins3.sum()) and int(got.del5.sum()) == got.dels == int(got.del3.sum())
            # additivity over a split range, for everything but the reads
            for cut in (S.W, 1500, 2 * S.W + 1):
                x, y, whole = run(eng, case, 7, 20, (0, False), 300, cut), run(eng, case, 7, 20, (0, False), cut, 4950), run(eng, case, 7, 20, (0, False), 300, 4950)
                for k in R.SCALARS[4:] + R.TABLES:
                    assert np.array_equal(np.asarray(getattr(x, k)) + np.asarray(getattr(y, k)), np.asarray(getattr(whole, k))), (cut, k)
                assert x.reads + y.reads >= whole.reads > 0


def test_ep_interleaves_with_the_scans_and_builds_the_index_itself():
    case = S.planted()
    loci = [(1135, 1145), (2000, 2060), (3000, 3080)]                               # the first: spanned by the deep reads of 50 matched bases
    with Engine(CallableOptions(), 0) as eng:
        resident(eng, case)
        first = run(eng, case, 50, 20, (0x704, True))                               # the first call on a fresh tile builds the index itself
        assert R.differences(first, case.expected(50, 20, (0x704, True))) == [] and first.kernel_ms > 0
        ms, nbytes = eng.site_scan_stats()
        table_ms, sum_ms = eng.site_error_profile_stats()
        assert ms == first.kernel_ms and table_ms > 0 and sum_ms > 0 and abs(table_ms + sum_ms - ms) < 1e-6 and nbytes > 8 * (36 * 50 + 22)
        scan0 = eng.site_scan(20, 10, case.ref)
        dels0 = eng.site_scan_dels(20, 1, 1, 1, case.ref, filter=(0x704, True))
        str0 = eng.site_str_lengths(loci, 5, 20, filter=(0x704, False))
        # the context-owned arrays of this call and of the scans: each in storage of its own
        r = _lib.cl_ep_result()
        f = _lib.cl_scan_filter(0x704, 1, 0)
        assert eng._lib.cl_site_error_profile(eng._h, 20, C.byref(f), 50, case.ref.ctypes.data, case.ref_len, 0, L, C.byref(r)) == 0
        keep = C.string_at(r.from5, 36 * 50 * 8)
        d5, dprm = _lib.cl_del_result(), _lib.cl_del_params(1, 1, 1)
        assert eng._lib.cl_site_scan_dels(eng._h, 20, C.byref(f), C.byref(dprm), case.ref.ctypes.data, case.ref_len, 0, L, C.byref(d5)) == 0
        keep_dels = C.string_at(d5.candidates, int(d5.n_deleted) * 32)
        scan1 = eng.site_scan(20, 10, case.ref)
        dels1 = eng.site_scan_dels(20, 1, 1, 1, case.ref, filter=(0x704, True))
        str1 = eng.site_str_lengths(loci, 5, 20, filter=(0x704, False))
        assert keep == C.string_at(r.from5, 36 * 50 * 8)                            # the scans leave the tables alone ...
        again = run(eng, case, 7, 0, None)
        assert R.differences(again, case.expected(7, 0, None)) == []
        assert keep_dels == C.string_at(d5.candidates, int(d5.n_deleted) * 32) and dels0.deleted >= 3      # ... and this call their candidates
        assert (scan0.low_depth, scan0.mixed, scan0.match, scan0.variant) == (scan1.low_depth, scan1.mixed, scan1.match, scan1.variant)
        assert np.array_equal(scan0.candidates, scan1.candidates) and np.array_equal(dels0.candidates, dels1.candidates)
        assert np.array_equal(str0.hist, str1.hist) and np.array_equal(str0.partial, str1.partial) and int(str0.hist.sum()) > 100
        # start == end: zeros without a launch
        none = run(eng, case, 7, 20, (0, False), 1500, 1500)
        assert (none.reads, none.bases, none.ins, none.dels) == (0, 0, 0, 0) and not none.from5.any() and eng.site_scan_stats()[0] == 0.0


def test_ep_refusals_leave_the_context_usable():
    case = S.planted()
    sites = np.arange(1, 2000, 7, dtype=np.uint32)

    def refused(*a, **k):
        with pytest.raises(EngineError) as e:
            eng.site_error_profile(*a, **k)
        assert e.value.status == -1 and len(str(e.value)) > len(" (cl_status -1)") + 10, str(e.value)
        return str(e.value)

    with Engine(CallableOptions(), 0) as eng:
        refused(7, 20, case.ref)                                                    # nothing resident
        # a tile filtered for its own list (the random reads: a read of 255 operations, as planted, makes a pileup send its tile whole)
        eng.site_pileup(20, L, L, S.randomised(1).rec, sites)
        assert "cl_site_pileup" in refused(7, 20, case.ref)
        eng.site_upload(L, L, case.rec)
        assert "attach" in refused(7, 20, case.ref, filter=(0, False))              # a filter with nothing attached
        ok = eng.site_error_profile(7, 20, case.ref)                                # the unfiltered form needs no attachment
        eng.site_attach_quals(case.rec, S.MBQ)
        for form in (None, (0x704, True)):
            assert "n_cycles" in refused(0, 20, case.ref, filter=form)
            assert "n_cycles" in refused(257, 20, case.ref, filter=form)
            refused(7, 20, case.ref, 10, 5, filter=form)                            # start > end
            refused(7, 20, case.ref, 0, L + 1, filter=form)                         # end > contig_len
            assert "ref_len" in refused(7, 20, case.ref[:4000], filter=form)        # another ref_len
        out = _lib.cl_ep_result()
        assert eng._lib.cl_site_error_profile(eng._h, 20, None, 7, None, L, 0, L, C.byref(out)) == -1 and b"reference" in eng._lib.cl_last_error(eng._h)
        assert eng._lib.cl_site_error_profile(eng._h, 20, None, 7, case.ref.ctypes.data, L, 0, L, None) == -1          # null out
        # the next good calls succeed, equal the reference, and equal the library's host route on the same arrays
        for C_, mq, flt in ((7, 20, None), (256, 0, (0x704, True)), (1, 20, (0, False))):
            got = run(eng, case, C_, mq, flt)
            assert R.differences(got, case.expected(C_, mq, flt)) == [], (C_, mq, flt)
            ex, bq = (None, None) if flt is None else (flt[0], S.MBQ if flt[1] else None)
            assert got.tables_equal(V.error_profile_measure(case.rec, L, case.ref, C_, mq, exclude_flags=ex, min_base_quality=bq))
        assert ok.tables_equal(eng.site_error_profile(7, 20, case.ref))
    with HostStage(CallableOptions()) as hs:
        with pytest.raises(EngineError) as e:
            hs.site_error_profile(7, 20, case.ref)
        assert e.value.status == -2


def damaged_sample(seed=80, Lc=20_000, rl=100, n=3000):
    """Reads of rl matched bases at random places, half of them reverse.  Three reads in ten carry deamination at the
    first three cycles of the molecule's 5' end: a forward read shows T where the reference has C at query index 0..2, a
    reverse read shows A where the reference has G at query index rl - 3 .. rl - 1.  A few reads are duplicates."""
    ref = synth.make_reference(Lc, seed)
    text = bytes(ref & 0xDF).decode()
    rng = random.Random(seed)
    reads = []
    for i in range(n):
        p = rng.randint(0, Lc - rl)
        seq = list(text[p:p + rl])
        rev = i & 1
        if i % 10 < 3:
            for q in (range(rl - 3, rl) if rev else range(3)):
                if seq[q] == ("G" if rev else "C"):
                    seq[q] = "A" if rev else "T"
        reads.append((p, f"{rl}M", 60, 30, (0x10 if rev else 0) | (0x400 if rng.random() < 0.03 else 0), f"d{i}", "".join(seq)))
    reads.sort(key=lambda r: r[0])
    return ref, ContigRecords.from_reads(reads)


def test_error_profile_on_files_and_cli(tmp_path):
    Lc = 20_000
    ref, rec = damaged_sample()
    names = ["chr1", "chrM", "chrY"]; lens = [248956422, Lc, 57227415]
    bam = str(tmp_path / "s.bam"); fa = str(tmp_path / "s.fa")
    write_bam(bam, list(zip(names, lens)), {1: rec}, block_every=500)
    write_fasta(fa, [("chrM", ref)])
    events = R.expand(rec)

    def want(cycles=50, mq=20, bq=None, ex=0, region=None):
        a, b = region or (0, Lc)
        z = R.profile(events, rec, Lc, ref, Lc, a, b, cycles, mq, ex, bq)
        return z, R.expected_tsv("chrM", z, mq, bq, ex)

    out = str(tmp_path / "o.tsv"); fi = str(tmp_path / "fi.tsv"); lib_out = str(tmp_path / "w.tsv")

    def cli(sub, *args, o=out):
        return subprocess.run([_b.CLI, sub, bam, "-r", fa, "-o", o, "-L", "chrM"] + list(args), capture_output=True, text=True)

    def other():
        r = cli("find-variants", o=fi)
        assert r.returncode == 0, r.stderr
        return open(fi).read()

    before = other()
    z, w0 = want()
    # the sample shows its damage where it was planted: C>T at the first three 5' cycles at three reads in ten, and no G>A there
    for d in range(3):
        c_to = z["from5"][d, 1].astype(np.int64)
        assert 0.2 < c_to[3] / c_to.sum() < 0.4 and int(z["from5"][d, 2, 0]) == 0, (d, c_to)
        assert int(z["from3"][d, 1, 3]) == 0
    assert int(z["from5"][3:, 1, 3].sum()) == 0 and z["reads"] > 2500
    r = cli("error-profile")
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w0
    V.error_profile(bam, fa, "chrM", out)
    assert open(out).read() == w0
    V.write_error_profile(lib_out, "chrM", ErrorProfile(**z), min_quality=20)
    assert open(lib_out).read() == w0
    z1, w1 = want(cycles=256, mq=0, bq=13, ex=0x704, region=(1000, 15_000))
    assert w1 != w0 and "##exclude_flags=0x0704" in w1 and "##min_base_quality=13" in w1 and "##range=1000-15000" in w1
    r = cli("error-profile", "--cycles=256", "--min-quality", "0", "--min-base-quality", "13", "--exclude-flags", "0x704", "--region", "1000-15000")
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w1
    V.error_profile(bam, fa, "chrM", out, region=(1000, 15_000), cycles=256, min_quality=0, min_base_quality=13, exclude_flags=0x704)
    assert open(out).read() == w1
    V.write_error_profile(lib_out, "chrM", ErrorProfile(**z1), min_quality=0, min_base_quality=13, exclude_flags=0x704)
    assert open(lib_out).read() == w1
    # the other subcommands write the bytes they wrote before
    assert other() == before
    # exit 1 with a message: an unknown contig, a region beyond the contig
    r = subprocess.run([_b.CLI, "error-profile", bam, "-r", fa, "-o", out, "-L", "chrZ"], capture_output=True, text=True)
    assert r.returncode == 1 and "chrZ" in r.stderr
    r = cli("error-profile", "--region", f"10-{Lc + 1}")
    assert r.returncode == 1 and "beyond" in r.stderr
    with pytest.raises(EngineError):
        V.error_profile(bam, fa, "chrM", out, region=(10, Lc + 1))
