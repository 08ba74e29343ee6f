"""Repeat lengths on the device (-m gpu): cl_site_str_lengths in both forms and find-strs; every histogram and partial count
compared exactly with the independent reference tests/str_ref.py (reads expanded into per-position events, counted from
those) on the planted and random inputs of tests/str_cases.py -- never with the engine's own other calls, except where the
invariant between two calls is what is tested."""
import ctypes as C
import itertools
import random
import subprocess

import numpy as np
import pytest

import str_cases as S
import str_ref as R
from bamio import write_bam, write_fasta
from decodingustools_amd import CallableOptions, Engine, EngineError, _lib, build as _b, synth, variants as V
from decodingustools_amd.callable_loci import HostStage
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu
L = S.L


def flt(ex):
    return None if ex is None else (ex, False)


def check_case(eng, case, flanks=S.FLANKS, quals=(0, 20), filters=S.FILTERS, what=""):
    """The resident tile of `eng` is case.rec (flags attached): every flank, mapping quality and form against the reference.
    Returns the spanning reads seen."""
    seen = 0
    for flank, mq, ex in itertools.product(flanks, quals, filters):
        hist, partial = case.expected(flank, mq, ex)
        got = eng.site_str_lengths(case.loci, flank, mq, filter=flt(ex))
        assert got.hist.shape == hist.shape, (what, flank, mq, ex)
        assert np.array_equal(got.hist, hist), (what, flank, mq, ex, np.argwhere(got.hist != hist)[:3])
        assert np.array_equal(got.partial, partial), (what, flank, mq, ex, np.argwhere(got.partial != partial)[:3])
        seen += int(hist.sum())
    return seen


def test_str_planted_reads_and_loci_at_every_corner_of_the_rule():
    case = S.planted()
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, case.rec)
        eng.site_attach_quals(case.rec, 0)
        assert check_case(eng, case, what="planted") > 5000
        # what the planted reads say by themselves (tests/str_cases.py PINS, derived by hand): each alone on a tile
        for read, locus, flank, spanning, delta in S.PINS:
            one = S.Case([case.reads[case.index(read)]], [S.PLANTED_LOCI[locus]])
            eng.site_upload(L, L, one.rec)
            got = eng.site_str_lengths(one.loci, flank, 20)
            want = np.zeros(128, np.uint32)
            if spanning:
                want[delta + 63 if -63 <= delta <= 63 else 127] = 1
            assert np.array_equal(got.hist[0, 0], want) and int(got.partial[0]) == (0 if spanning else 1), (read, locus, flank)
        # 700 reads over one locus: more than two strides of the workgroup, bins past 255
        eng.site_upload(L, L, case.rec)
        eng.site_attach_quals(case.rec, 0)
        deep = eng.site_str_lengths([S.PLANTED_LOCI["deep"]], 5, 20).hist[0, 0]
        assert (int(deep[63]), int(deep[67]), int(deep.sum())) == (400, 300, 700)
        gates = eng.site_str_lengths([S.PLANTED_LOCI["gates"]], 5, 20, filter=(0x704, False))
        assert (int(gates.hist[0, 0, 63]), int(gates.hist[0, 1, 63]), int(gates.hist.sum()), int(gates.partial[0])) == (1, 2, 3, 0)
    # a tile in descending coordinate order, and a shuffled one: wider read ranges, the same counts
    for order in (sorted(case.reads, key=lambda r: -r[0]), random.Random(5).sample(case.reads, len(case.reads))):
        other = S.Case(order, case.loci, sort=False)
        with Engine(CallableOptions(), 0) as eng:
            eng.site_upload(L, L, other.rec)
            eng.site_attach_quals(other.rec, 0)
            for flank, ex in ((5, None), (5, 0x704), (64, 0)):
                got = eng.site_str_lengths(case.loci, flank, 20, filter=flt(ex))
                assert np.array_equal(got.hist, case.expected(flank, 20, ex)[0]) and np.array_equal(got.partial, case.expected(flank, 20, ex)[1])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_str_random_reads_and_loci(seed):
    case = S.randomised(seed)
    assert len(case.loci) == 155 and case.rec.n == 300 and sum(1 for s, e in case.loci if e - s >= 1000) == 5
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, case.rec)
        eng.site_attach_quals(case.rec, 0)
        assert check_case(eng, case, what=f"random {seed}") > 5000


def sample(seed=70, Lc=20_000, rl=100):
    """A planted sample over a random reference: four loci of period 4, ten units each.
      expanded   60 reads, 54 with two more units -- 27 placed at x == s, 27 one unit further right -- and 6 without
      contracted 60 reads, all with one unit deleted, the deletion at three different places inside the repeat
      mixed      60 reads, 30 with one more unit
      shallow    5 reads
    and reads at random places, a few of them flagged."""
    ref = synth.make_reference(Lc, seed)
    text = bytes(ref & 0xDF).decode()
    rng = random.Random(seed)
    loci = [dict(start=3000, end=3040, period=4, name="DYS-expanded"), dict(start=7001, end=7041, period=4, name="DYS-contracted"),
            dict(start=11_003, end=11_043, period=4, name="DYS-mixed"), dict(start=15_000, end=15_040, period=4, name="DYS-shallow")]
    reads = []

    def add(p, cigar, name, i):
        seq, x = "", p
        for l, op in ((int(t[:-1]), t[-1]) for t in __import__("re").findall(r"\d+[MID]", cigar)):
            if op == "M":
                seq += text[x:x + l]; x += l
            elif op == "I":
                seq += ("ACGT" * 8)[:l]
            else:
                x += l
        k = rng.random()
        reads.append((p, cigar, 60, 30, (0x10 if i & 1 else 0) | (0x400 if k < 0.05 else 0), name, seq))

    for i in range(60):
        s = loci[0]["start"]
        p = s - 26 - i % 20
        a = s - p + (4 if i % 2 else 0)                                 # half of the aligners put the gap one unit further right
        add(p, f"{a}M8I{rl - 8 - a}M" if i < 54 else f"{rl}M", f"e{i}", i)
        s = loci[1]["start"]
        p = s - 26 - i % 20
        a = s - p + 4 * (i % 3)
        add(p, f"{a}M4D{rl - a}M", f"c{i}", i)
        s = loci[2]["start"]
        p = s - 26 - i % 20
        add(p, f"{s - p + 8}M4I{rl - 4 - (s - p + 8)}M" if i < 30 else f"{rl}M", f"m{i}", i)
    for i in range(5):
        add(loci[3]["start"] - 30 - i, f"{rl}M", f"s{i}", i)
    for i in range(400):
        p = rng.randint(0, Lc - rl - 10)
        a = rng.randint(5, rl - 10)
        k = rng.random()
        add(p, f"{rl}M" if k < 0.9 else f"{a}M2I{rl - 2 - a}M" if k < 0.95 else f"{a}M3D{rl - a}M", f"b{i}", i)
    reads.sort(key=lambda r: r[0])
    return ref, ContigRecords.from_reads(reads), loci


def test_str_call_shape_and_interleaving_with_the_scans():
    Lc = 20_000
    ref, rec, loci = sample()
    pairs = [(l["start"], l["end"]) for l in loci]
    events = R.expand(rec)
    want, want_p = R.measure(events, rec, Lc, pairs, 5, 20, 0x704)
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(Lc, Lc, rec)
        eng.site_attach_quals(rec, 20)
        first = eng.site_str_lengths(pairs, 5, 20, filter=(0x704, False))           # the first call on a fresh tile builds the index itself
        assert np.array_equal(first.hist, want) and np.array_equal(first.partial, want_p) and first.kernel_ms > 0
        assert int(first.hist[0].sum()) > 40 and int(first.hist[0, :, 63 + 8].sum()) * 10 >= int(first.hist[0].sum()) * 8
        ms, nbytes = eng.site_scan_stats()
        assert ms == first.kernel_ms and nbytes >= 4 * (2 * 512 + 12)
        scan0 = eng.site_scan(20, 10, ref)
        ins0 = eng.site_scan_ins(20, 10, 3, 2500, ref, filter=(0x704, True))
        cons0 = eng.site_scan_consensus(20, 10, 3, 7000, ref, filter=(0x704, True))
        # context-owned arrays of the other scans and of this call: each in storage of its own
        r5, iprm, f704 = _lib.cl_ins_result(), _lib.cl_ins_params(10, 3, 2500), _lib.cl_scan_filter(0x704, 1, 0)
        assert eng._lib.cl_site_scan_ins(eng._h, 20, C.byref(f704), C.byref(iprm), ref.ctypes.data, Lc, 0, Lc, C.byref(r5)) == 0
        keep_ins = C.string_at(r5.candidates, int(r5.n_inserted) * 32)
        sr = _lib.cl_str_result()
        arr = np.ascontiguousarray(pairs, np.uint32)
        f0 = _lib.cl_scan_filter(0x704, 0, 0)
        assert eng._lib.cl_site_str_lengths(eng._h, 20, C.byref(f0), 5, arr.ctypes.data, len(pairs), C.byref(sr)) == 0
        assert (int(sr.n_loci), int(sr.strands)) == (4, 2)
        keep_str = (C.string_at(sr.hist, 4 * 2 * 128 * 4), C.string_at(sr.partial, 16))
        assert keep_str == (want.tobytes(), want_p.tobytes())
        again = eng.site_str_lengths(pairs, 5, 20, filter=(0x704, False))            # two calls return equal arrays
        assert np.array_equal(again.hist, first.hist) and np.array_equal(again.partial, first.partial)
        assert keep_ins == C.string_at(r5.candidates, int(r5.n_inserted) * 32)
        scan1 = eng.site_scan(20, 10, ref)
        ins1 = eng.site_scan_ins(20, 10, 3, 2500, ref, filter=(0x704, True))
        cons1 = eng.site_scan_consensus(20, 10, 3, 7000, ref, filter=(0x704, True))
        assert keep_str == (C.string_at(sr.hist, 4 * 2 * 128 * 4), C.string_at(sr.partial, 16))       # ... and the scans leave them alone
        assert (scan0.low_depth, scan0.mixed, scan0.match, scan0.variant) == (scan1.low_depth, scan1.mixed, scan1.match, scan1.variant)
        assert np.array_equal(scan0.candidates, scan1.candidates)
        assert np.array_equal(ins0.candidates, ins1.candidates) and np.array_equal(ins0.observations, ins1.observations) and ins0.inserted >= 3
        assert np.array_equal(cons0.cons, cons1.cons) and (cons0.low_depth, cons0.deleted, cons0.ref) == (cons1.low_depth, cons1.deleted, cons1.ref)
        # n_loci 0, 1 and 65536; duplicate and overlapping loci in any order
        none = eng.site_str_lengths([], 5, 20, filter=(0, False))
        assert none.hist.shape == (0, 2, 128) and none.partial.shape == (0,) and eng.site_scan_stats()[0] == 0.0
        assert eng.site_str_lengths(np.zeros((0, 2), np.uint32), 5, 20).hist.shape == (0, 1, 128)
        one = eng.site_str_lengths(pairs[:1], 5, 20, filter=(0x704, False))
        assert np.array_equal(one.hist, want[:1]) and np.array_equal(one.partial, want_p[:1])
        for form in (None, (0x704, False)):
            many = eng.site_str_lengths([pairs[0]] * 65536, 5, 20, filter=form)
            assert many.hist.shape[0] == 65536 and (many.hist == many.hist[0]).all() and (many.partial == many.partial[0]).all()
            assert np.array_equal(many.hist[0], R.measure(events, rec, Lc, pairs[:1], 5, 20, 0x704 if form else None)[0][0]), form
        mixed = [pairs[2], (2990, 3050), pairs[0], pairs[0], (3010, 3030), (0, 1), pairs[3], (Lc - 1024, Lc), pairs[1], pairs[2]]
        got = eng.site_str_lengths(mixed, 5, 20, filter=(0x704, False))
        exp, exp_p = R.measure(events, rec, Lc, mixed, 5, 20, 0x704)
        assert np.array_equal(got.hist, exp) and np.array_equal(got.partial, exp_p)
        assert np.array_equal(got.hist[2], got.hist[3]) and np.array_equal(got.hist[0], got.hist[9])


def test_str_refusals_leave_the_context_usable_and_the_host_route_agrees():
    Lc = 20_000
    ref, rec, loci = sample(71)
    pairs = [(l["start"], l["end"]) for l in loci]
    sites = np.arange(1, 2000, 7, dtype=np.uint32)

    def refused(*a, **k):
        with pytest.raises(EngineError) as e:
            eng.site_str_lengths(*a, **k)
        assert e.value.status == -1 and len(str(e.value)) > len(" (cl_status -1)") + 10, str(e.value)
        return str(e.value)

    with Engine(CallableOptions(), 0) as eng:
        refused(pairs, 5, 20)                                                       # nothing resident
        eng.site_pileup(20, Lc, Lc, rec, sites)                                     # a tile filtered for its own list
        refused(pairs, 5, 20)
        eng.site_upload(Lc, Lc, rec)
        assert "attach" in refused(pairs, 5, 20, filter=(0, False))                 # a filter with nothing attached
        ok = eng.site_str_lengths(pairs, 5, 20)                                     # one strand needs no attachment
        eng.site_attach_quals(rec, 20)
        for form in (None, (0x704, False)):
            assert "flank" in refused(pairs, 0, 20, filter=form)
            assert "flank" in refused(pairs, 65, 20, filter=form)
            assert "CL_STR_MAX_LOCI" in refused([pairs[0]] * 65537, 5, 20, filter=form)
            refused([(10, 10)], 5, 20, filter=form)                                 # start >= end
            refused([pairs[0], (30, 20)], 5, 20, filter=form)
            refused([(Lc - 10, Lc + 1)], 5, 20, filter=form)                        # end > contig_len
            refused([(100, 1125)], 5, 20, filter=form)                              # longer than CL_STR_MAX_SPAN
        assert "use_base_quality" in refused(pairs, 5, 20, filter=(0x704, True))
        out = _lib.cl_str_result()
        assert eng._lib.cl_site_str_lengths(eng._h, 20, None, 5, None, 3, C.byref(out)) == -1 and b"loci" in eng._lib.cl_last_error(eng._h)
        arr = np.ascontiguousarray(pairs, np.uint32)
        assert eng._lib.cl_site_str_lengths(eng._h, 20, None, 5, arr.ctypes.data, 4, None) == -1             # null out
        # the next good calls succeed, equal the reference, and equal the library's host route on the same arrays
        events = R.expand(rec)
        for flank, mq, ex in ((5, 20, None), (5, 20, 0x704), (1, 0, 0), (64, 20, 0xFFFF)):
            got = eng.site_str_lengths(pairs, flank, mq, filter=flt(ex))
            exp, exp_p = R.measure(events, rec, Lc, pairs, flank, mq, ex)
            assert np.array_equal(got.hist, exp) and np.array_equal(got.partial, exp_p), (flank, mq, ex)
            host = V.str_measure(rec, Lc, pairs, flank, mq, ex)
            assert np.array_equal(got.hist, host.hist) and np.array_equal(got.partial, host.partial), (flank, mq, ex)
        assert np.array_equal(eng.site_str_lengths(pairs, 5, 20).hist, ok.hist)
    with HostStage(CallableOptions()) as hs:
        with pytest.raises(EngineError) as e:
            hs.site_str_lengths(pairs, 5, 20)
        assert e.value.status == -2


def test_find_strs_on_files_and_cli(tmp_path):
    Lc = 20_000
    ref, rec, loci = sample()
    names = ["chr1", "chrY", "chrM"]; lens = [248956422, Lc, 16569]
    bam = str(tmp_path / "s.bam"); fa = str(tmp_path / "s.fa"); lf = str(tmp_path / "loci.tsv")
    write_bam(bam, list(zip(names, lens)), {1: rec}, block_every=500)
    write_fasta(fa, [("chrY", ref)])
    open(lf, "w").write("# a catalogue of four\n" + "".join(f"chrY\t{l['start']}\t{l['end']}\t{l['period']}\t{l['name']}\tmore\n" for l in loci[:2]) +
                        "chr1\t5\t25\t4\telsewhere\n\n" + "".join(f"chrY\t{l['start']}\t{l['end']}\t{l['period']}\t{l['name']}\n" for l in loci[2:]))
    events = R.expand(rec)
    pairs = [(l["start"], l["end"]) for l in loci]

    def want(flank=5, md=10, mq=20, ex=0, per=7000):
        hist, partial = R.measure(events, rec, Lc, pairs, flank, mq, ex)
        return R.expected_tsv("chrY", loci, 1, hist, partial, flank, md, mq, ex, per)

    out = str(tmp_path / "o.tsv"); fi = str(tmp_path / "fi.tsv"); cs = str(tmp_path / "c.fa"); ch = str(tmp_path / "c.tsv")

    def cli(sub, *args, o=out):
        return subprocess.run([_b.CLI, sub, bam, "-r", fa, "-o", o, "-L", "chrY"] + list(args), capture_output=True, text=True)

    def others():
        r = cli("find-insertions", o=fi)
        assert r.returncode == 0, r.stderr
        r = cli("consensus", "--changes", ch, o=cs)
        assert r.returncode == 0, r.stderr
        return open(fi).read(), open(cs).read(), open(ch).read()

    before = others()
    w0 = want()
    rows = [ln.split("\t") for ln in w0.splitlines() if not ln.startswith("#")]
    assert [r[9] for r in rows] == ["called", "called", "mixed", "low_depth"]
    assert rows[0][10:12] == ["12", "+8"] and float(rows[0][13]) >= 0.85 and rows[1][10:12] == ["9", "-4"] and int(rows[3][6]) < 10
    # the expansion is spread over two anchors: find-insertions at 0.7 lists neither, find-strs calls two more units
    s = loci[0]["start"]
    anchors = {int(ln.split("\t")[1]) for ln in before[0].splitlines() if not ln.startswith("#")}
    assert not anchors & set(range(s - 2, s + 12))
    r = cli("find-strs", "--loci", lf)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w0
    V.find_strs(bam, fa, "chrY", lf, out)
    assert open(out).read() == w0
    w1 = want(flank=10, md=3, mq=0, ex=0x704, per=4000)
    assert w1 != w0 and "##exclude_flags=0x0704" in w1 and "low_depth=0" in w1
    r = cli("find-strs", "--loci", lf, "--flank=10", "--min-depth", "3", "--min-quality=0", "--exclude-flags", "0x704", "--min-allele-fraction", "0.4")
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w1
    V.find_strs(bam, fa, "chrY", lf, out, flank=10, min_depth=3, min_quality=0, exclude_flags=0x704, min_allele_fraction="0.4")
    assert open(out).read() == w1
    # the other subcommands write the bytes they wrote before
    assert others() == before
    # exit 1 with a message: an unknown contig, a malformed loci file, a locus beyond the contig, one longer than 1024
    r = subprocess.run([_b.CLI, "find-strs", bam, "-r", fa, "-o", out, "-L", "chrZ", "--loci", lf], capture_output=True, text=True)
    assert r.returncode == 1 and "chrZ" in r.stderr
    for text, word in (("chrY\t10\t20\tfour\tbad\n", "line 1"), (f"chrY\t{Lc - 10}\t{Lc + 1}\t4\tbeyond\n", "beyond"), ("chrY\t100\t1125\t4\tlong\n", "1024")):
        bad = str(tmp_path / "bad.tsv")
        open(bad, "w").write(text)
        r = cli("find-strs", "--loci", bad)
        assert r.returncode == 1 and word in r.stderr, (text, r.stderr)
        with pytest.raises(EngineError):
            V.find_strs(bam, fa, "chrY", bad, out)
