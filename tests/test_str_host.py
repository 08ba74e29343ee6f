"""The host side of find-strs, without a device: dut_str_measure against the independent reference tests/str_ref.py on the
planted and random inputs of tests/str_cases.py, the calling rule against exact fractions, the unit notation, the loci
file's parser, the TSV against a hand-written golden (tests/golden/str_kat.json), the CLI's argument checks, and the read
walk itself (csrc/str_walk.h) with dut_str_measure as a program of their own under AddressSanitizer + UBSan."""
import itertools
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import long_cases as LS
import str_cases as S
import str_ref as R
from decodingustools_amd import EngineError, build as _b, variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "str_kat.json")))


def test_the_reference_gives_what_the_planted_reads_say_by_themselves():
    c = S.planted()
    seen = set()
    for read, locus, flank, spanning, delta in S.PINS:
        s, e = S.PLANTED_LOCI[locus]
        got = R.measure_read(c.events[c.index(read)], s, e, flank)
        assert got[0] == spanning and (not spanning or got[1] == delta), (read, locus, flank, got)
        # ... and the library's host route over that read alone
        one = S.Case([c.reads[c.index(read)]], [(s, e)])
        lib = V.str_measure(one.rec, S.L, one.loci, flank, 20)
        want = np.zeros(128, np.uint32)
        if spanning:
            want[delta + 63 if -63 <= delta <= 63 else 127] = 1
        assert np.array_equal(lib.hist[0, 0], want) and int(lib.partial[0]) == (0 if spanning else 1), (read, locus, flank)
        seen.add(read)
    assert len(seen) >= 40
    names = list(S.PLANTED_LOCI)
    hist, partial = c.expected(5, 20, 0)
    gates = hist[names.index("gates")]
    # plain, mapq 20 and the reverse read, the duplicate and the secondary one span it; mapq 19 does not take part
    assert (int(gates[0, 63]), int(gates[1, 63]), int(partial[names.index("gates")])) == (3, 2, 0)
    assert c.expected(5, 20, 0x704)[0][names.index("gates")].sum() == 3 and c.expected(5, 0, None)[0][names.index("gates")].sum() == 6
    deep = hist[names.index("deep")]
    assert deep.sum() == 700 and int(deep[:, 63].sum()) == 400 and int(deep[:, 67].sum()) == 300 and deep.max() > 128
    deltas = hist[names.index("deltas")].sum(0)
    assert [int(deltas[b]) for b in (0, 126, 127)] == [1, 1, 3]            # -63 and +63 in their bins; -64, +64 and +500 in "other"
    assert not hist[names.index("s-below-the-flank")].any() and partial[names.index("s-below-the-flank")] == 2


@pytest.mark.parametrize("which", ["planted", "random-1", "random-2", "random-3"])
def test_host_route_equals_the_reference(which):
    case = S.planted() if which == "planted" else S.randomised(int(which[-1]))
    some = 0
    for flank, mq, ex in itertools.product(S.FLANKS, (0, 20), S.FILTERS):
        hist, partial = case.expected(flank, mq, ex)
        got = V.str_measure(case.rec, S.L, case.loci, flank, mq, ex)
        assert got.hist.shape == hist.shape and np.array_equal(got.hist, hist), (which, flank, mq, ex, np.argwhere(got.hist != hist)[:3])
        assert np.array_equal(got.partial, partial), (which, flank, mq, ex)
        some += int(hist.sum())
    assert some > 5000
    # a tile in descending coordinate order and a shuffled one: the same counts
    for order in (sorted(case.reads, key=lambda r: -r[0]), S.random.Random(3).sample(case.reads, len(case.reads))):
        other = S.Case(order, case.loci, sort=False)
        got = V.str_measure(other.rec, S.L, case.loci, 5, 20, 0x704)
        assert np.array_equal(got.hist, case.expected(5, 20, 0x704)[0]) and np.array_equal(got.partial, case.expected(5, 20, 0x704)[1])


def test_host_route_equals_the_reference_on_long_reads():
    """The tile of tests/long_cases.py: loci at least 65 536 positions past a read's start, inside reads of some 6 000 and of
    66 001 operations, over a 50 000N."""
    case = LS.whole()
    LS.check_shape(case)
    some = 0
    for flank, mq, ex in LS.STR_COMBOS:
        hist, partial = case.str_expected(flank, mq, ex)
        got = V.str_measure(case.rec, LS.LC, LS.LOCI, flank, mq, ex)
        assert got.hist.shape == hist.shape and np.array_equal(got.hist, hist), (flank, mq, ex, np.argwhere(got.hist != hist)[:3])
        assert np.array_equal(got.partial, partial), (flank, mq, ex)
        some += int(hist.sum())
    assert some > 10_000
    hist, partial = case.str_expected(5, 20, None)
    assert int(hist[:, 0, 127].sum()) >= 4 and int(hist[:, 0, 63 + 7].sum()) >= 2 and int(hist[:, 0, 63 - 12].sum()) >= 2 and int(partial.sum()) > 20


def test_host_route_refusals_and_the_empty_call():
    c = S.planted()
    empty = V.str_measure(c.rec, S.L, [], 5, 20, 0)
    assert empty.hist.shape == (0, 2, 128) and empty.partial.shape == (0,)
    for loci, flank in (([(10, 10)], 5), ([(12, 10)], 5), ([(S.L - 5, S.L + 1)], 5), ([(0, 1025)], 5), ([(10, 20)], 0), ([(10, 20)], 65)):
        with pytest.raises(EngineError):
            V.str_measure(c.rec, S.L, loci, flank, 20, 0)
    assert V.str_measure(c.rec, S.L, [(0, 1024), (S.L - 1, S.L)], 64, 20, None).hist.shape == (2, 1, 128)


def frac_call(both, min_depth, per_10k):
    n = sum(both)
    top = max(range(127), key=lambda b: (both[b], -b))
    rest = [b for b in range(127) if b != top]
    second = max(rest, key=lambda b: (both[b], -b))
    status = R.LOW_DEPTH if n < min_depth else R.CALLED if Fraction(both[top], n) >= Fraction(per_10k, 10000) else R.MIXED
    return status, n, top - 63, both[top], second - 63, both[second]


def test_call_equals_exact_fractions_over_every_small_count():
    seen = {R.LOW_DEPTH: 0, R.MIXED: 0, R.CALLED: 0}
    for n in range(0, 41):
        for top in range(0, n + 1):
            for md, per in ((1, 7000), (10, 7000), (5, 5000), (1, 10000), (3, 3333), (1, 1)):
                fwd, rev = np.zeros(128, np.uint32), np.zeros(128, np.uint32)
                fwd[70], rev[70] = top // 2, top - top // 2
                rest = n - top
                fwd[20], rev[127] = rest // 2, rest - rest // 2               # the rest: another length and "other"
                got = V.str_call(fwd, rev, md, per)
                want = frac_call([int(a) + int(b) for a, b in zip(fwd, rev)], md, per)
                assert (got["status"], got["n"], got["delta"], got["count"], got["delta2"], got["count2"]) == want, (n, top, md, per, got, want)
                assert got["fwd"] + got["rev"] == got["count"] and R.call(fwd, rev, md, per) == got
                seen[got["status"]] += 1
    assert min(seen.values()) > 50, seen


def test_call_ties_other_and_empty_histograms():
    h = np.zeros(128, np.uint32)
    got = V.str_call(h, None, 1, 7000)                                      # every count 0: low_depth, the smallest delta stands for both
    assert (got["status"], got["n"], got["delta"], got["count"], got["delta2"], got["count2"]) == (V.STR_LOW_DEPTH, 0, -63, 0, -62, 0)
    h[[60, 66]] = 5
    got = V.str_call(h, None, 1, 5000)                                      # a tie: the smaller delta wins, the other is second
    assert (got["status"], got["delta"], got["count"], got["delta2"], got["count2"], got["fwd"], got["rev"]) == (V.STR_CALLED, -3, 5, 3, 5, 5, 0)
    assert V.str_call(h, None, 1, 5001)["status"] == V.STR_MIXED and V.str_call(h, None, 11, 5000)["status"] == V.STR_LOW_DEPTH
    h[127] = 90                                                             # "other" is fullest: it never wins, and it counts in n
    got = V.str_call(h, None, 10, 500)
    assert (got["status"], got["n"], got["other"], got["delta"], got["count"]) == (V.STR_CALLED, 100, 90, -3, 5)
    assert V.str_call(h, None, 10, 501)["status"] == V.STR_MIXED
    only = np.zeros(128, np.uint32); only[127] = 50
    got = V.str_call(only, only, 10, 1)
    assert (got["status"], got["n"], got["other"], got["count"], got["count2"]) == (V.STR_MIXED, 100, 100, 0, 0)
    big = np.zeros(128, np.uint32); big[63] = 3_000_000_000; big[64] = 1_285_714_285      # 10000 * count is past 2^32: 64 bits
    assert V.str_call(big, None, 10, 7000) == R.call(big, None, 10, 7000) and V.str_call(big, None, 10, 7000)["status"] == V.STR_CALLED
    big[64] += 1
    assert V.str_call(big, None, 10, 7000)["status"] == V.STR_MIXED == R.call(big, None, 10, 7000)["status"]
    for md, per in ((0, 7000), (10, 0), (10, 10001)):
        with pytest.raises(EngineError):
            V.str_call(h, None, md, per)
    with pytest.raises(ValueError):
        V.str_call(h[:100])


def test_units_notation():
    assert V.str_units(13, 0, 1) == "13" and V.str_units(52, 0, 4) == "13" and V.str_units(40, -1, 4) == "9.3" and V.str_units(36, 2, 6) == "6.2"
    assert V.str_units(36, -36, 6) == "0" and V.str_units(3, 0, 4) == "0.3" and V.str_units(1024, 63, 255) == "4.67"
    for span, delta, period in itertools.product((1, 7, 40, 1024), (-63, -1, 0, 5, 63), (1, 4, 6, 255)):
        if span + delta >= 0:
            assert V.str_units(span, delta, period) == R.units(span, delta, period)
    for span, delta, period in ((10, 0, 0), (10, 0, 256), (10, -11, 4)):
        with pytest.raises(EngineError):
            V.str_units(span, delta, period)


def test_loci_file_parser(tmp_path):
    p = str(tmp_path / "loci.tsv")
    open(p, "w").write("# a catalogue\n\nchrY\t1000\t1048\t4\tDYS-A\n#chrY\t1\t2\t3\tcommented\nchrX\t5\t9\t2\tother-contig\nchrY\t2000\t2040\t4\tDYS-B\textra\tcolumns 1 2\n"
                       "chr1\t0\t4\t1\tanother\r\nchrY\t7\t8\t255\tDYS-last")
    loci, skipped = V.str_loci_parse(p, "chrY")
    assert skipped == 2 and loci == [dict(start=1000, end=1048, period=4, name="DYS-A"), dict(start=2000, end=2040, period=4, name="DYS-B"),
                                     dict(start=7, end=8, period=255, name="DYS-last")]
    assert V.str_loci_parse(p, "chrM") == ([], 5)
    good = "chrY\t1\t9\t4\tok\n"
    for bad in ("chrY\t10\t20\t4", "chrY\tten\t20\t4\tn", "chrY\t10\t-20\t4\tn", "chrY\t20\t20\t4\tn", "chrY\t10\t20\t0\tn", "chrY\t10\t20\t256\tn",
                "chrY\t10\t20\t4\t", "chrY 10 20 4 n", "chrY\t10\t4294967296\t4\tn", "chrY\t10\t20\t4\t" + "n" * 64, "chrX\t10\t5\t4\tother-contig-too"):
        open(p, "w").write("# head\n" + good + "\n" + bad + "\n" + good)
        with pytest.raises(EngineError) as e:
            V.str_loci_parse(p, "chrY")
        assert "line 4" in str(e.value), (bad, str(e.value))
    with pytest.raises(EngineError) as e:
        V.str_loci_parse(str(tmp_path / "absent.tsv"), "chrY")
    assert "absent.tsv" in str(e.value)


def kat_result():
    hist = np.zeros((len(KAT["loci"]), 2, 128), np.uint32)
    for i, l in enumerate(KAT["loci"]):
        for strand, bins in l["hist"].items():
            for delta, n in bins.items():
                hist[i, int(strand), 127 if delta == "other" else int(delta) + 63] = n
    return V.StrResult(hist=hist, partial=np.array([l["partial"] for l in KAT["loci"]], np.uint32))


def test_tsv_bytes_equal_the_hand_written_golden(tmp_path):
    out = str(tmp_path / "o.tsv")
    res = kat_result()
    want = "\n".join(KAT["tsv"]) + "\n"
    V.write_strs(out, KAT["contig"], KAT["loci"], res, loci_skipped=KAT["skipped"], flank=KAT["flank"], min_depth=KAT["min_depth"], min_quality=KAT["min_quality"],
                 min_allele_fraction=KAT["min_allele_fraction"], exclude_flags=KAT["exclude_flags"])
    assert open(out).read() == want
    # the reference writes the same bytes, so the device tests may hold the tool against it
    assert R.expected_tsv(KAT["contig"], KAT["loci"], KAT["skipped"], res.hist, res.partial, KAT["flank"], KAT["min_depth"], KAT["min_quality"],
                          KAT["exclude_flags"], 7000) == want
    assert {want.splitlines()[12 + i].split("\t")[9] for i in range(4)} == {"called", "mixed", "low_depth"} and "\t9.3\t-1\t" in want
    # one strand, no locus at all, refused options
    one = V.StrResult(hist=res.hist.sum(1, keepdims=True).astype(np.uint32), partial=res.partial)
    V.write_strs(out, "chrY", KAT["loci"], one)
    assert open(out).read() == R.expected_tsv("chrY", KAT["loci"], 0, one.hist, one.partial, 5, 10, 20, 0, 7000) and "\t18\t0.9000\t18\t0\t" in open(out).read()
    V.write_strs(out, "chrY", [], V.StrResult(hist=np.zeros((0, 2, 128), np.uint32), partial=np.zeros(0, np.uint32)), loci_skipped=9)
    assert open(out).read() == R.expected_tsv("chrY", [], 9, np.zeros((0, 2, 128), np.uint32), [], 5, 10, 20, 0, 7000)
    for kw in (dict(flank=0), dict(flank=65), dict(min_depth=0)):
        with pytest.raises(EngineError):
            V.write_strs(out, "chrY", KAT["loci"], res, **kw)
    with pytest.raises(ValueError):
        V.write_strs(out, "chrY", KAT["loci"], res, min_allele_fraction="1.5")
    with pytest.raises(ValueError):
        V.write_strs(out, "chrY", KAT["loci"][:2], res)


def test_cli_argument_errors_exit_2_without_a_device(tmp_path):
    out = str(tmp_path / "o.tsv")
    base = [_b.CLI, "find-strs", "absent.bam", "-r", "absent.fa", "-o", out]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")

    def run(*args):
        return subprocess.run(base + list(args), capture_output=True, text=True, env=env)

    for args in (["--loci", "l.tsv"],                                                   # no -L
                 ["-L", "chrY"],                                                        # no --loci
                 ["-L", "chrY", "--loci", "l.tsv", "--flank", "0"], ["-L", "chrY", "--loci", "l.tsv", "--flank=65"],
                 ["-L", "chrY", "--loci", "l.tsv", "--flank", "five"],
                 ["-L", "chrY", "--loci", "l.tsv", "--min-depth", "0"],
                 ["-L", "chrY", "--loci", "l.tsv", "--min-allele-fraction", "0"], ["-L", "chrY", "--loci", "l.tsv", "--min-allele-fraction", "1.01"],
                 ["-L", "chrY", "--loci", "l.tsv", "--min-allele-fraction=often"],
                 ["-L", "chrY", "--loci", "l.tsv", "--exclude-flags", "0x"], ["-L", "chrY", "--loci", "l.tsv", "--exclude-flags", "70000"],
                 ["-L", "chrY", "--loci", "l.tsv", "--region", "1-5"], ["-L", "chrY", "--loci", "l.tsv", "--no-such-flag"]):
        r = run(*args)
        assert r.returncode == 2 and r.stderr and not os.path.exists(out), (args, r.returncode, r.stderr[-300:])
    r = subprocess.run([_b.CLI, "find-strs", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "find-strs" in r.stderr and "--loci" in r.stderr
    # the files are looked at only behind the arguments: an unreadable loci file is exit 1 and names it
    r = run("-L", "chrY", "--loci", str(tmp_path / "absent.tsv"))
    assert r.returncode == 1 and "absent.tsv" in r.stderr


def fnv(words, h=14695981039346656037):
    for w in words:
        for k in range(4):
            h = ((h ^ ((int(w) >> (8 * k)) & 255)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_walk_and_host_route_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "str_walk_host")
    # (variants.cpp alone: what its file-level functions call of the engine and the readers stays unresolved -- this program
    # calls none of them)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "str_walk_host.cpp"), os.path.join(ROOT, "decodingustools_amd", "csrc", "variants.cpp"),
           "-Wl,--unresolved-symbols=ignore-all", "-lpthread", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if any(m in r.stderr for m in ("cannot find -lasan", "cannot find -lubsan", "unrecognized command-line option", "unrecognized argument")):
            pytest.skip("sanitizer runtimes not installed here: " + r.stderr[-300:])
        pytest.fail("the sanitizer build failed:\n" + r.stderr[-3000:])
    configs = [(5, 20, 2, 0x704), (1, 0, 1, 0), (64, 20, 2, 0), (5, 0, 2, 0xFFFF), (1, 20, 2, 0x704), (64, 0, 1, 0)]
    for name, case, L in (("planted", S.planted(), S.L), ("random", S.randomised(1), S.L), ("long", LS.whole().as_str, LS.LC)):
        rec = case.rec
        lines = [f"{L} {rec.n} {len(case.loci)} {len(configs)}"] + LS.read_lines(rec, bases=False)
        lines += [f"{s} {e}" for s, e in case.loci] + [" ".join(str(x) for x in c) for c in configs]
        path = str(tmp_path / f"{name}.txt")
        open(path, "w").write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0", DUT_THREADS="3"))
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
        walk = []
        for s, e in case.loci:
            for i in range(rec.n):
                ev = case.events[i]
                # (a read that overlaps no position of the locus matches neither flank on both sides: never spanning)
                spanning, delta = R.measure_read(ev, s, e, configs[0][0]) if ev["lo"] < e + 70 and ev["hi"] > s - 70 else (False, 0)
                walk += [1, delta & 0xFFFFFFFF] if spanning else [0, 0]
        want = [f"walk {fnv(walk):016x}"]
        for k, (flank, mq, strands, ex) in enumerate(configs):
            hist, partial = case.expected(flank, mq, ex if strands == 2 else None)
            want.append(f"measure {k} {fnv(list(hist.reshape(-1)) + list(partial)):016x}")
        assert r.stdout.splitlines() == want, (name, r.stdout, want)
