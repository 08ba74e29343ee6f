"""The host side of find-deletions, without a device: the fraction parser, the deletion rule in plain C++ against the
independent reference tests/dels_ref.py, the merge of candidates into events, the TSV writer, the CLI's argument checks;
and the reference itself against hand-derived columns (tests/golden/dels_kat.json)."""
import json
import os
import subprocess

import numpy as np
import pytest

import dels_ref as D
from decodingustools_amd import CallableOptions, EngineError, build as _b, variants as V
from decodingustools_amd.callable_loci import DEL_CANDIDATE, DelResult, HostStage
from decodingustools_amd.records import ContigRecords

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dels_kat.json")))["cases"]


@pytest.mark.parametrize("text,want", [("1", 10000), ("1.0000", 10000), (".0001", 1), ("0.7", 7000), ("0.5001", 5001), ("1.0", 10000),
                                       ("00.25", 2500), ("0.9999", 9999)])
def test_fraction_parser_accepts(text, want):
    assert V.del_fraction_parse(text) == want


@pytest.mark.parametrize("text", ["0", "1.0001", "0.12345", "1.00000", "junk", "", "0.0000", "2", "-0.5", "+1", ".", "1e0", "0.7x", " 1", "0,7"])
def test_fraction_parser_rejects(text):
    with pytest.raises(ValueError):
        V.del_fraction_parse(text)


def test_the_minor_fraction_parser_keeps_its_interval():
    assert V.minor_fraction_parse("0.5") == 5000
    for text in ("0.5001", "1", "0.7"):
        with pytest.raises(ValueError):
            V.minor_fraction_parse(text)


PARAMS = [(1, 1, 1), (10, 3, 7000), (5, 2, 2500), (4, 1, 10000), (7, 4, 3333)]


def test_rule_equals_the_reference_over_a_grid():
    n = {D.LOW_DEPTH: 0, D.KEPT: 0, D.DELETED: 0}
    small = [(d, x) for d in range(0, 26) for x in range(0, 26)]
    big = [(d, x) for d in (429_496, 429_497, 429_498, 1 << 20, (1 << 22) - 1, 1 << 22, (1 << 31) + 5, (1 << 32) - 1)
           for x in (0, 1, 184_070, 184_071, 613_566, 613_567, 1 << 20, 1 << 22, (1 << 22) + 1, (1 << 31), (1 << 32) - 1)]
    for n_del, depth in small + big:
        for prm in PARAMS:
            got, want = V.del_classify_counts(n_del, depth, *prm), D.classify(n_del, depth, *prm)
            assert got == want, (n_del, depth, prm, got, want)
            n[got] += 1
    assert min(n.values()) > 100, n


def test_rule_at_the_threshold_edges_and_past_32_bits():
    # 10000 * del == per_10k * span exactly, and one read below it
    for span, per_10k in ((10, 7000), (10000, 1), (3, 3333), (30000, 3333), (2, 5000), (7, 10000), (1 << 20, 7000)):
        d, rem = divmod(per_10k * span, 10000)
        d += 1 if rem else 0                                           # the smallest count at or above the threshold
        assert V.del_classify_counts(d, span - d, 1, 1, per_10k) == V.DEL_DELETED == D.classify(d, span - d, 1, 1, per_10k), (span, per_10k)
        if d > 1:
            assert V.del_classify_counts(d - 1, span - d + 1, 1, 1, per_10k) == V.DEL_KEPT == D.classify(d - 1, span - d + 1, 1, 1, per_10k)
    # the left side alone wraps 32 bits: 10000 * 429 497 = 2^32 + 2704 against 4000 * 2^20 < 2^32
    assert 10000 * 429_497 > 1 << 32 > 4000 * (1 << 20)
    assert V.del_classify_counts(429_497, (1 << 20) - 429_497, 1, 1, 4000) == V.DEL_DELETED
    # exactly at min_del_count and one below; span exactly min_depth and one below
    assert V.del_classify_counts(3, 0, 1, 3, 1) == V.DEL_DELETED and V.del_classify_counts(2, 1, 1, 3, 1) == V.DEL_KEPT
    assert V.del_classify_counts(6, 4, 10, 1, 1) == V.DEL_DELETED and V.del_classify_counts(6, 3, 10, 1, 1) == V.DEL_LOW_DEPTH
    assert V.del_classify_counts(0, 0, 1, 1, 1) == V.DEL_LOW_DEPTH and V.del_classify_counts(0, 50, 1, 1, 1) == V.DEL_KEPT
    for prm in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 10001)):
        with pytest.raises(EngineError):
            V.del_classify_counts(5, 5, *prm)


def del_cand(rows):
    c = np.zeros(len(rows), DEL_CANDIDATE)
    for i, (pos, r, n_del, depth, lf, lr, df, dr) in enumerate(rows):
        c[i] = (pos, ord(r), (0, 0, 0), n_del, depth, lf, lr, df, dr)
    return c


def ev(start, end, q, n_del, span, lf, lr, max_del):
    return {"start": start, "end": end, "length": end - start + 1, "q": q, "del": n_del, "span": span, "del_fwd": lf, "del_rev": lr, "max_del": max_del}


def strip(events):
    return [{k: v for k, v in e.items() if k != "ref"} for e in events]


def test_events_of_hand_made_lists():
    assert V.del_events(del_cand([])) == [] == D.events([])
    # single positions
    rows = [(5, "A", 9, 1, 5, 4, 1, 0), (7, "C", 4, 0, 4, 0, 0, 0), (100, "N", 3, 7, 0, 3, 7, 0)]
    want = [ev(5, 5, 5, 9, 10, 5, 4, 9), ev(7, 7, 7, 4, 4, 4, 0, 4), ev(100, 100, 100, 3, 10, 0, 3, 3)]
    assert V.del_events(del_cand(rows)) == want == strip(D.events(rows))
    # adjacent runs: 10-12 and 14-15; the smallest del in the middle / at the end of a run
    rows = [(10, "A", 8, 2, 4, 4, 1, 1), (11, "C", 6, 4, 2, 4, 2, 2), (12, "G", 9, 1, 5, 4, 1, 0),
            (14, "T", 5, 0, 5, 0, 0, 0), (15, "A", 4, 3, 1, 3, 3, 0)]
    want = [ev(10, 12, 11, 6, 10, 2, 4, 9), ev(14, 15, 15, 4, 7, 1, 3, 5)]
    assert V.del_events(del_cand(rows)) == want == strip(D.events(rows))
    assert [e["ref"] for e in D.events(rows)] == ["ACG", "TA"]
    # a tie for the smallest del: the first position wins, with its own span and strands
    rows = [(20, "A", 7, 0, 7, 0, 0, 0), (21, "C", 5, 5, 1, 4, 5, 0), (22, "G", 5, 1, 3, 2, 1, 0), (23, "T", 6, 0, 3, 3, 0, 0)]
    assert V.del_events(del_cand(rows)) == [ev(20, 23, 21, 5, 10, 1, 4, 7)] == strip(D.events(rows))
    # a run cut by the range: the list of a scan over [1024, 2048) starts and ends inside a longer deletion
    rows = [(p, "A", 10, 0, 5, 5, 0, 0) for p in range(1025, 1031)] + [(p, "C", 12, 1, 6, 6, 1, 0) for p in range(2040, 2049)]
    assert V.del_events(del_cand(rows)) == [ev(1025, 1030, 1025, 10, 10, 5, 5, 10), ev(2040, 2048, 2040, 12, 13, 6, 6, 12)] == strip(D.events(rows))
    with pytest.raises(EngineError):
        V.del_events(del_cand([(9, "A", 1, 0, 0, 0, 0, 0), (9, "A", 1, 0, 0, 0, 0, 0)]))       # positions must ascend


ROWS = ([(101, "a".upper(), 15, 6, 8, 7, 4, 2), (102, "C", 14, 7, 14, 0, 4, 3), (103, "N", 16, 5, 8, 8, 3, 2)]
        + [(2000 + k, "ACGT"[k % 4], 30 + (k % 5), 2, 15, 15 + (k % 5), 1, 1) for k in range(64)]
        + [(3000 + k, "ACGT"[k % 4], 40 - (k % 3), 0, 20, 20 - (k % 3), 0, 0) for k in range(65)]
        + [(70000, "T", 4, 40, 1, 3, 20, 20)])


def test_tsv_writer_against_the_reference_and_a_hand_written_file(tmp_path):
    res = DelResult(start=100, end=70_100, low_depth=5, kept=70_000 - 5 - len(ROWS), deleted=len(ROWS), candidates=del_cand(ROWS))
    exp = dict(low_depth=5, kept=res.kept, deleted=res.deleted, candidates=ROWS)
    out = str(tmp_path / "d.tsv")
    V.write_deletions(out, "chrM", res, 10, 20, 3, 7000, min_base_quality=20, exclude_flags=0x704, min_del_per_strand=2)
    text = open(out, "rb").read().decode()
    assert text == D.expected_tsv("chrM", exp, 100, 70_100, 10, 20, 20, 0x704, 7000, 3, 2)
    ref64 = "".join("ACGT"[k % 4] for k in range(64))
    assert text == ("##contig=chrM\n##range=100-70100\n##min_depth=10\n##min_quality=20\n##min_base_quality=20\n##exclude_flags=0x0704\n"
                    f"##min_del_fraction=0.7000\n##min_del_count=3\n##positions=70000\n##low_depth=5\n##kept={res.kept}\n##deleted=133\n##events=4\n"
                    "#contig\tstart\tend\tlength\tref\tdel\tspan\tfreq\tmax_del\tdel_fwd\tdel_rev\tfilter\n"
                    "chrM\t101\t103\t3\tACN\t14\t21\t0.6667\t16\t14\t0\tstrand\n"
                    f"chrM\t2000\t2063\t64\t{ref64}\t30\t32\t0.9375\t34\t15\t15\tPASS\n"
                    "chrM\t3000\t3064\t65\t.\t38\t38\t1.0000\t40\t20\t18\tPASS\n"
                    "chrM\t70000\t70000\t1\tT\t4\t44\t0.0909\t4\t1\t3\tstrand\n")
    # K = 0: always PASS; no base-quality threshold: "."; another fraction
    V.write_deletions(out, "chrM", res, 10, 20, 1, 125)
    text = open(out).read()
    assert "##min_base_quality=.\n##exclude_flags=0x0000\n##min_del_fraction=0.0125\n##min_del_count=1\n" in text
    assert "strand" not in text and text.count("\tPASS\n") == 4
    assert text == D.expected_tsv("chrM", exp, 100, 70_100, 10, 20, None, 0, 125, 1, 0)
    V.write_deletions(out, "chrM", DelResult(0, 10, 3, 7, 0, del_cand([])), 10, 20, 3, 10000)
    assert open(out).read() == D.expected_tsv("chrM", dict(low_depth=3, kept=7, deleted=0, candidates=[]), 0, 10, 10, 20, None, 0, 10000, 3, 0)
    with pytest.raises(ValueError):
        V.write_deletions(out, "chrM", DelResult(0, 10, 0, 7, 3, del_cand(ROWS)), 10, 20, 1, 125)     # 3 claimed, 133 given


def cli(tmp_path, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="9999")                  # no device can be opened
    return subprocess.run([_b.CLI, "find-deletions", str(tmp_path / "none.bam"), "-r", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.tsv")]
                          + list(args), capture_output=True, text=True, env=env)


@pytest.mark.parametrize("args,msg", [
    ([], "needs '-L <CONTIG>'"),
    (["-L", "chrM", "--region", "100"], "invalid value '100' for '--region'"),
    (["-L", "chrM", "--region", "200-100"], "invalid value '200-100' for '--region'"),
    (["-L", "chrM", "--region=a-b"], "invalid value 'a' for '--region'"),
    (["-L", "chrM", "--min-del-fraction", "0"], "invalid value '0' for '--min-del-fraction'"),
    (["-L", "chrM", "--min-del-fraction", "1.0001"], "invalid value '1.0001' for '--min-del-fraction'"),
    (["-L", "chrM", "--min-del-fraction=0.70001"], "invalid value '0.70001' for '--min-del-fraction'"),
    (["-L", "chrM", "--min-del-fraction", "70%"], "invalid value '70%' for '--min-del-fraction'"),
    (["-L", "chrM", "--min-del-count", "0"], "invalid value '0' for '--min-del-count'"),
    (["-L", "chrM", "--min-del-count=x"], "invalid value 'x' for '--min-del-count'"),
    (["-L", "chrM", "--min-base-quality", "256"], "invalid value '256' for '--min-base-quality'"),
    (["-L", "chrM", "--min-base-quality", "q"], "invalid value 'q' for '--min-base-quality'"),
    (["-L", "chrM", "--exclude-flags", "0xZZ"], "invalid value '0xZZ' for '--exclude-flags'"),
    (["-L", "chrM", "--exclude-flags=65536"], "invalid value '65536' for '--exclude-flags'"),
    (["-L", "chrM", "--min-del-per-strand", "-1"], "invalid value '-1' for '--min-del-per-strand'"),
    (["-L", "chrM", "--min-depth", "0"], "invalid value '0' for '--min-depth'"),
    (["-L", "chrM", "--no-such-flag"], "unexpected argument '--no-such-flag'"),
])
def test_cli_argument_errors_exit_2_before_a_device_is_opened(tmp_path, args, msg):
    r = cli(tmp_path, *args)
    assert r.returncode == 2, r.stderr
    assert msg in r.stderr, r.stderr


def test_cli_accepts_well_formed_values_and_names_the_subcommand(tmp_path):
    """The argument check passes: the run then fails on the missing BAM with exit 1, not 2, still without a device."""
    for args in (["-L", "chrM"], ["-L", "chrM", "--min-del-fraction", "1", "--min-del-count=1"],
                 ["-L", "chrM", "--region=5-6", "--exclude-flags", "0x704", "--min-base-quality", "0", "--min-del-per-strand=2", "--min-del-fraction=.0001"]):
        r = cli(tmp_path, *args)
        assert r.returncode == 1 and "invalid value" not in r.stderr, (args, r.stderr)
    r = subprocess.run([_b.CLI, "--help"], capture_output=True, text=True)
    assert "find-deletions" in r.stdout + r.stderr and "--min-del-fraction" in r.stdout + r.stderr
    r = subprocess.run([_b.CLI, "find-deletions", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "find-deletions" in r.stderr


def test_a_context_without_a_device_answers_a_device_error():
    with HostStage(CallableOptions()) as h:
        for flt in (None, (0x704, True)):
            with pytest.raises(EngineError) as e:
                h.site_scan_dels(20, 10, 3, 7000, np.zeros(100, np.uint8), filter=flt)
            assert e.value.status == -2


def dense(maps, L):
    out = np.zeros((2, L), np.int64)
    for s in (0, 1):
        for p, v in maps[s].items():
            out[s, int(p)] = v
    return out


@pytest.mark.parametrize("case", KAT, ids=[c["name"] for c in KAT])
def test_the_reference_walk_gives_the_hand_derived_columns(case):
    rec = ContigRecords.from_reads([tuple(r) for r in case["reads"]])
    L = case["contig_len"]
    depth, dels = D.walk(L, case["ref_len"], rec, case["min_quality"], case["exclude_flags"], case["min_base_quality"])
    assert np.array_equal(depth, dense(case["depth"], L)), depth
    assert np.array_equal(dels, dense(case["del"], L)), dels


def test_the_reference_reduces_and_merges_a_hand_derived_case():
    case = KAT[0]
    rec = ContigRecords.from_reads([tuple(r) for r in case["reads"]])
    L = case["contig_len"]
    ref = np.frombuffer(b"acgtacgtacgtacgtacgtacgtacgtac", np.uint8)
    depth, dels = D.walk(L, L, rec, 0)
    exp = D.reduce(depth, dels, ref, L, 1, 1, 5000, 0, L)
    # span >= 1 and del / span >= 1/2: 6 (2 of 3), 13-15, 24, 28, 29; position 3 has 1 of 3, position 5 has 1 of 4
    assert exp["candidates"] == [(7, "G", 2, 1, 2, 0, 0, 1), (14, "C", 1, 0, 1, 0, 0, 0), (15, "G", 1, 0, 1, 0, 0, 0), (16, "T", 1, 0, 1, 0, 0, 0),
                                 (25, "A", 1, 0, 0, 1, 0, 0), (29, "A", 1, 0, 1, 0, 0, 0), (30, "C", 1, 0, 1, 0, 0, 0)]
    # nothing at 0, 1, 16-19, 22, 23: 8 low; 22 positions with something, 7 of them deleted
    assert (exp["low_depth"], exp["kept"], exp["deleted"]) == (8, 15, 7)
    assert [(e["start"], e["end"], e["ref"]) for e in D.events(exp["candidates"])] == [(7, 7, "G"), (14, 16, "CGT"), (25, 25, "A"), (29, 30, "AC")]
    assert D.reduce(depth, dels, ref, L, 1, 1, 5000, 0, L, stranded=False)["candidates"][0] == (7, "G", 2, 1, 0, 0, 0, 0)
