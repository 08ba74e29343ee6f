"""The host side of error-profile, without a device: dut_error_profile_measure against the independent reference
tests/ep_ref.py on the planted and random inputs of tests/ep_cases.py, with one thread and with four; single reads against
tables derived by hand (PINS, tests/golden/ep_kat.json); the TSV against the hand-written golden; the CLI's argument checks;
and the read walk itself (csrc/ep_walk.h) with dut_error_profile_measure as a program of their own under AddressSanitizer
+ UBSan."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ep_cases as S
import ep_ref as R
import long_cases as LS
from decodingustools_amd import EngineError, ErrorProfile, build as _b, variants as V
from decodingustools_amd.records import ContigRecords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "ep_kat.json")))


def measure(case, C, mq, flt, start=0, end=S.L):
    ex, bq = (None, None) if flt is None else (flt[0], S.MBQ if flt[1] else None)
    return V.error_profile_measure(case.rec, S.L, case.ref, C, mq, start, end, exclude_flags=ex, min_base_quality=bq)


def check_case(name, case):
    """Every C, mapping quality and form over the whole contig, and every range at two of them.  Returns the bases seen."""
    seen = 0
    for C, mq, flt in itertools.product(S.CYCLES, S.QUALS, S.FILTERS):
        want = case.expected(C, mq, flt)
        assert R.differences(measure(case, C, mq, flt), want) == [], (name, C, mq, flt)
        seen += want["bases"]
    for (a, b), (C, flt) in itertools.product(S.RANGES, ((7, None), (256, (0x704, True)))):
        assert R.differences(measure(case, C, 20, flt, a, b), case.expected(C, 20, flt, a, b)) == [], (name, a, b, C, flt)
    return seen


def test_the_reference_and_the_host_route_give_what_the_pinned_reads_say_by_themselves():
    for name, read, flt, want in S.PINS:
        rec = ContigRecords.from_reads([read])
        exp = S.pin_expected(want)
        ex, bq = (None, None) if flt is None else (flt[0], S.MBQ if flt[1] else None)
        ref = R.profile(R.expand(rec), rec, S.PIN_L, S.PIN_REF, S.PIN_L, 0, S.PIN_L, S.PIN_C, 20, ex, bq)
        assert R.differences(ref, exp) == [], name
        got = V.error_profile_measure(rec, S.PIN_L, S.PIN_REF, S.PIN_C, 20, exclude_flags=ex, min_base_quality=bq)
        assert R.differences(got, exp) == [], name
    assert len(S.PINS) >= 6
    # what the planted reads were planted for shows in the reference's own tables
    c = S.planted()
    whole = c.expected(256, 20, (0x704, False))
    assert whole["reads"] > 600 and whole["bases"] > 30_000 and whole["uncomparable"] > 5 and whole["ins"] > 50 and whole["dels"] > 100
    assert whole["bases"] > int(whole["total"].trace()) > 0
    # the mismatches planted at query index 0 of every tenth deep read, all of them forward: the first 5' cycle
    assert int(whole["from5"][0].sum()) - int(whole["from5"][0].trace()) >= 40 > int(whole["from3"][0].sum()) - int(whole["from3"][0].trace())
    assert c.expected(256, 0, None)["reads"] > c.expected(256, 20, None)["reads"] > whole["reads"]
    assert c.expected(256, 20, (0x704, True))["bases"] < whole["bases"]
    assert S.planted(4900).expected(7, 20, None)["bases"] < c.expected(7, 20, None)["bases"]


@pytest.mark.parametrize("which", ["planted", "planted-short-reference", "random-1", "random-2"])
def test_host_route_equals_the_reference(which):
    case = dict(S.all_cases())[which]
    assert check_case(which, case) > 100_000
    # C at and above the longest read: the cycle tables each add up to total, cell by cell
    got = measure(case, 201, 20, (0x704, True))
    assert np.array_equal(got.from5.sum(0), got.total) and np.array_equal(got.from3.sum(0), got.total)
    assert int(got.ins5.sum()) == got.ins == int(got.ins3.sum()) and int(got.del5.sum()) == got.dels == int(got.del3.sum())
    # additivity over a split range, for everything but the reads
    for cut in (S.W, 1500, 4000):
        a, b, whole = measure(case, 7, 20, (0, False), 300, cut), measure(case, 7, 20, (0, False), cut, 4950), measure(case, 7, 20, (0, False), 300, 4950)
        for k in R.SCALARS[4:] + R.TABLES:
            assert np.array_equal(np.asarray(getattr(a, k)) + np.asarray(getattr(b, k)), np.asarray(getattr(whole, k))), (which, cut, k)
        assert a.reads + b.reads >= whole.reads
    # a tile in descending coordinate order and a shuffled one: the same counts
    for order in (sorted(case.reads, key=lambda r: -r[0]), S.random.Random(3).sample(case.reads, len(case.reads))):
        other = S.Case(order, case.ref_len, sort=False)
        assert R.differences(measure(other, 7, 20, (0x704, True)), case.expected(7, 20, (0x704, True))) == []


def test_host_route_equals_the_reference_on_long_reads():
    """The tile of tests/long_cases.py: reads past 65 535 stored bases, past 255 and past 65 535 operations, over many windows."""
    case = LS.whole()
    LS.check_shape(case)
    seen = 0
    for (a, b), (C, mq, flt) in itertools.product(LS.EP_RANGES, LS.EP_COMBOS):
        ex, bq = (None, None) if flt is None else (flt[0], LS.MBQ if flt[1] else None)
        got = V.error_profile_measure(case.rec, LS.LC, LS.REF, C, mq, a, b, exclude_flags=ex, min_base_quality=bq)
        want = case.ep_expected(C, mq, flt, a, b)
        assert R.differences(got, want) == [], (a, b, C, mq, flt)
        seen += want["bases"]
    assert seen > 5_000_000
    # from3 of a read past the escape needs its exact length: the last 256 positions of the forward read of 70 000 bases
    tail = case.ep_expected(256, 20, (0, False), LS.M70 + 70_000 - 256, LS.M70 + 70_000)
    assert int(tail["from3"][0].sum()) == 1 == int(tail["from3"][255].sum())
    assert R.differences(V.error_profile_measure(case.rec, LS.LC, LS.REF, 256, 20, LS.M70 + 70_000 - 256, LS.M70 + 70_000, exclude_flags=0), tail) == []


def test_host_route_with_one_thread_and_with_four():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import ep_cases as S, ep_ref as R, test_ep_host as T\n"
            "for name, case in S.all_cases():\n"
            "    for C, flt in ((7, None), (256, (0x704, True))):\n"
            "        assert R.differences(T.measure(case, C, 20, flt), case.expected(C, 20, flt)) == [], (name, C, flt)\n"
            "print('same')\n") % (ROOT, os.path.join(ROOT, "tests"))
    for threads in ("1", "4"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, DUT_THREADS=threads))
        assert r.returncode == 0 and r.stdout.strip() == "same", (threads, r.stderr[-2000:])


def test_host_route_refusals_and_the_empty_range():
    c = S.planted()
    empty = measure(c, 7, 20, None, 1500, 1500)
    assert (empty.reads, empty.bases, empty.ins, empty.dels) == (0, 0, 0, 0) and empty.from5.shape == (7, 4, 4) and not empty.from5.any()
    beyond = V.error_profile_measure(c.rec, S.L, S.REF[:1000], 7, 20, 2000, 3000)            # the range lies beyond the reference
    assert (beyond.reads, beyond.bases, beyond.uncomparable) == (0, 0, 0)
    for kw in (dict(n_cycles=0), dict(n_cycles=257), dict(start=10, end=5), dict(end=S.L + 1)):
        args = dict(n_cycles=7, start=0, end=S.L)
        args.update(kw)
        with pytest.raises(EngineError):
            V.error_profile_measure(c.rec, S.L, S.REF, args["n_cycles"], 20, args["start"], args["end"])


def kat_profile():
    z = S.pin_expected({})
    for k in ("ins5", "ins3", "del5", "del3"):
        z[k] = np.array(KAT[k], np.uint64)
    for k in ("from5", "from3"):
        for d, cells in enumerate(KAT[k]):
            for cell, n in cells.items():
                z[k][(d,) + divmod(R.CELLS.index(cell), 4)] = n
    for cell, n in KAT["total"].items():
        z["total"][divmod(R.CELLS.index(cell), 4)] = n
    z.update(KAT["scalars"])
    return z


def kat_records():
    return ContigRecords.from_reads([(r["pos"], r["cigar"], r["mapq"], 30, r["flag"], f"kat{i}", r["seq"]) for i, r in enumerate(KAT["reads"])])


def test_tsv_bytes_equal_the_hand_written_golden(tmp_path):
    out = str(tmp_path / "o.tsv")
    want = "\n".join(KAT["tsv"]) + "\n"
    z = kat_profile()
    ref = np.frombuffer(KAT["ref"].encode(), np.uint8)
    # the golden's tables are what its two reads give, by the reference and by the host route
    rec = kat_records()
    assert R.differences(R.profile(R.expand(rec), rec, KAT["contig_len"], ref, len(ref), 0, KAT["contig_len"], KAT["n_cycles"], KAT["min_quality"], KAT["exclude_flags"]), z) == []
    got = V.error_profile_measure(rec, KAT["contig_len"], ref, KAT["n_cycles"], KAT["min_quality"], exclude_flags=KAT["exclude_flags"])
    assert R.differences(got, z) == []
    V.write_error_profile(out, KAT["contig"], got, min_quality=KAT["min_quality"], exclude_flags=KAT["exclude_flags"])
    assert open(out).read() == want
    # the reference writes the same bytes, so the device tests may hold the tool against it
    assert R.expected_tsv(KAT["contig"], z, KAT["min_quality"], None, KAT["exclude_flags"]) == want
    assert "\t0.500000\n" in want and "##mismatch_rate=0.076923\n" in want
    # a base-quality threshold, a mask and an empty table: NA, and the reference agrees
    none = ErrorProfile(**{k: (v if not isinstance(v, np.ndarray) else np.zeros_like(v)) for k, v in z.items()})
    V.write_error_profile(out, "chrM", none, min_quality=0, min_base_quality=13, exclude_flags=0x704)
    text = open(out).read()
    zero = dict(z, **{k: np.zeros_like(z[k]) for k in R.TABLES})
    assert text == R.expected_tsv("chrM", zero, 0, 13, 0x704) and "##min_base_quality=13\n##exclude_flags=0x0704\n" in text
    assert text.count("\tNA\n") == 1 + 2 * KAT["n_cycles"]
    with pytest.raises(ValueError):
        V.write_error_profile(out, "chrM", ErrorProfile(**dict(z, n_cycles=5)))
    with pytest.raises(EngineError):
        V.write_error_profile(str(tmp_path / "no" / "such" / "dir.tsv"), "chrM", got)


def test_cli_argument_errors_exit_2_without_a_device(tmp_path):
    out = str(tmp_path / "o.tsv")
    base = [_b.CLI, "error-profile", "absent.bam", "-r", "absent.fa", "-o", out]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")

    def run(*args):
        return subprocess.run(base + list(args), capture_output=True, text=True, env=env)

    for args in ([],                                                                    # no -L
                 ["--cycles", "5"],
                 ["-L", "chrM", "--region", "100"], ["-L", "chrM", "--region", "a-b"], ["-L", "chrM", "--region", "50-50"], ["-L", "chrM", "--region=9-3"],
                 ["-L", "chrM", "--cycles", "0"], ["-L", "chrM", "--cycles=257"], ["-L", "chrM", "--cycles", "many"],
                 ["-L", "chrM", "--min-base-quality", "256"], ["-L", "chrM", "--min-base-quality", "q"],
                 ["-L", "chrM", "--exclude-flags", "0x"], ["-L", "chrM", "--exclude-flags", "70000"],
                 ["-L", "chrM", "--min-quality", "300"], ["-L", "chrM", "--no-such-flag"]):
        r = run(*args)
        assert r.returncode == 2 and r.stderr and not os.path.exists(out), (args, r.returncode, r.stderr[-300:])
    r = subprocess.run([_b.CLI, "error-profile", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "error-profile" in r.stderr and "--cycles" in r.stderr
    # the files are looked at only behind the arguments: an unreadable FASTA is exit 1 and names it
    r = run("-L", "chrM", "--cycles", "256", "--region", "5-9")
    assert r.returncode == 1 and "absent.fa" in r.stderr


def fnv(words, h=14695981039346656037):
    for w in words:
        for k in range(4):
            h = ((h ^ ((int(w) >> (8 * k)) & 255)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def fnv64(words):
    return fnv([x for w in words for x in (int(w) & 0xFFFFFFFF, int(w) >> 32)])


def test_walk_and_host_route_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "ep_walk_host")
    # (variants.cpp alone: what its file-level functions call of the engine and the readers stays unresolved -- this program
    # calls none of them)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "ep_walk_host.cpp"), os.path.join(ROOT, "decodingustools_amd", "csrc", "variants.cpp"),
           "-Wl,--unresolved-symbols=ignore-all", "-lpthread", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if any(m in r.stderr for m in ("cannot find -lasan", "cannot find -lubsan", "unrecognized command-line option", "unrecognized argument")):
            pytest.skip("sanitizer runtimes not installed here: " + r.stderr[-300:])
        pytest.fail("the sanitizer build failed:\n" + r.stderr[-3000:])
    # start end C min_quality filtered exclude_flags has_min_base_quality min_base_quality
    short = [(300, 4950, 7, 20, 1, 0x704, 1, S.MBQ), (0, S.L, 256, 0, 0, 0, 0, 0), (S.W, 2 * S.W, 1, 20, 1, 0, 0, 0), (1500, 1500, 7, 20, 0, 0, 0, 0),
             (0, S.L, 201, 20, 1, 0xFFFF, 1, S.MBQ), (2 * S.W - 1, 2 * S.W + 1, 256, 0, 1, 0, 1, S.MBQ)]
    # the long reads: the walk's range starts and ends mid-window inside reads of 70 000 bases
    long = [(33_333, 199_999, 256, 20, 1, 0x704, 1, LS.MBQ), (0, LS.LC, 256, 0, 0, 0, 0, 0), (66 * LS.W, 67 * LS.W, 1, 20, 1, 0, 0, 0),
            (LS.LC - 1000, LS.LC, 256, 0, 1, 0, 1, LS.MBQ)]
    for name, case, L, configs in (("planted-short-reference", S.planted(4900), S.L, short), ("random", S.randomised(1), S.L, short),
                                   ("long", LS.whole().as_ep, LS.LC, long)):
        rec, ev = case.rec, case.events
        lines = [f"{L} {case.ref_len} {rec.n} {len(configs)}", " ".join(map(str, case.ref.tolist()))] + LS.read_lines(rec)
        lines += [" ".join(str(x) for x in c) for c in configs]
        path = str(tmp_path / f"{name}.txt")
        open(path, "w").write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0", DUT_THREADS="3"))
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
        lo, hi = configs[0][0], min(configs[0][1], case.ref_len)
        walk = np.zeros((rec.n, 7), np.int64)
        for col, (records, with_l) in ((0, (ev["base"], False)), (3, (ev["ins"], True)), (5, (ev["dele"], True))):
            rr, p, q, l, _ = records
            keep = (p >= lo) & (p < hi)
            # (a read whose start is not a 32-bit position of the contig is walked from where its start wraps to: none here)
            np.add.at(walk[:, col], rr[keep], 1)
            if with_l:
                np.add.at(walk[:, col + 1], rr[keep], (p + q + l)[keep])
            else:
                np.add.at(walk[:, 1], rr[keep], p[keep]); np.add.at(walk[:, 2], rr[keep], q[keep])
        neg = rec.pos < 0
        walk[neg] = 0
        h = f"{fnv((walk & 0xFFFFFFFF).reshape(-1)):016x}"
        want = [f"walk {h}", f"split {h}"]
        for k, (a, b, C, mq, filtered, ex, has_bq, bq) in enumerate(configs):
            z = R.profile(ev, rec, L, case.ref, case.ref_len, a, b, C, mq, ex if filtered else None, bq if has_bq else None)
            words = [z[s] for s in ("reads", "bases", "uncomparable", "ins", "ins_bases", "dels", "del_bases")]
            for t in R.TABLES:
                words += list(z[t].reshape(-1))
            want.append(f"measure {k} {fnv64(words):016x}")
        assert r.stdout.splitlines() == want, (name, r.stdout, want)
