"""The host side of find-insertions, without a device: the insertion rule in plain C++ against the independent reference
tests/ins_ref.py, the grouping of observations into alleles, the TSV writer, the CLI's argument checks; and the reference
itself against hand-derived cases (tests/golden/ins_kat.json)."""
import json
import os
import subprocess

import numpy as np
import pytest

import ins_ref as I
from decodingustools_amd import CallableOptions, EngineError, build as _b, variants as V
from decodingustools_amd.callable_loci import INS_CANDIDATE, INS_OBS, HostStage, InsResult
from decodingustools_amd.records import ContigRecords

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ins_kat.json")))["cases"]
PARAMS = [(1, 1, 1), (10, 3, 7000), (5, 2, 2500), (4, 1, 10000), (7, 4, 3333)]


def dense(maps, L):
    out = np.zeros((2, L), np.int64)
    for s in (0, 1):
        for p, v in maps[s].items():
            out[s, int(p)] = v
    return out


def kat_walk(case):
    rec = ContigRecords.from_reads([tuple(r) for r in case["reads"]])
    L = case["contig_len"]
    return rec, L, I.walk(L, case["ref_len"], rec, case["min_quality"], case["exclude_flags"], case["min_base_quality"])


@pytest.mark.parametrize("case", KAT, ids=[c["name"] for c in KAT])
def test_the_reference_walk_gives_the_hand_derived_counts_and_alleles(case):
    rec, L, (depth, ins, events) = kat_walk(case)
    assert np.array_equal(depth, dense(case["depth"], L)), depth
    assert np.array_equal(ins, dense(case["ins"], L)), ins
    assert (ins <= depth).all()
    exp = I.reduce(depth, ins, np.full(L, ord("a"), np.uint8), L, 1, 1, 1, 0, L)
    assert [c[0] - 1 for c in exp["candidates"]] == sorted({int(p) for m in case["ins"] for p in m})
    obs = I.observations(events, rec, exp["candidates"])
    assert len(obs) == int(ins.sum())
    assert [[a["pos"], a["len"], a["seq"], a["count"], a["fwd"], a["rev"]] for a in I.alleles(obs)] == case["alleles"]


def test_the_reference_reduces_a_hand_derived_case():
    rec, L, (depth, ins, events) = kat_walk(KAT[0])
    ref = np.frombuffer(b"acgtacgtacgtacgtacgtacgtacgtac", np.uint8)
    exp = I.reduce(depth, ins, ref, L, 2, 1, 5000, 0, L)
    # depth >= 2 and ins / depth >= 1/2: position 12 has 2 of 3, position 21 has 1 of 2; position 4 has 1 of 3; 27 and 28 are 1 deep
    assert exp["candidates"] == [(13, "A", 2, 3, 1, 1, 1, 2), (22, "C", 1, 2, 0, 1, 1, 1)]
    # 2 deep or more: 2-7, 10-12, 20-22; the other 18 positions are low
    assert (exp["low_depth"], exp["kept"], exp["inserted"]) == (18, 10, 2)
    assert I.reduce(depth, ins, ref, L, 2, 1, 5000, 0, L, stranded=False)["candidates"][0] == (13, "A", 2, 3, 0, 0, 0, 0)
    assert I.observations(events, rec, exp["candidates"]) == [(13, 2, 0x21 << 56, 0, 1), (13, 2, 0x88 << 56, 0, 0), (22, 1, 4 << 60, 0, 1)]
    assert I.observations(events, rec, exp["candidates"], stranded=False)[0] == (13, 2, 0x21 << 56, 0, 0)


def test_rule_equals_the_reference_over_a_grid():
    n = {I.LOW_DEPTH: 0, I.KEPT: 0, I.INSERTED: 0}
    small = [(i, d) for d in range(0, 26) for i in range(0, d + 1)]
    # 10000 * ins wraps 32 bits from 429 497 on (2^32 / 10000 = 429 496.7...)
    big = [(i, d) for d in (429_496, 429_497, 613_566, 613_567, 1 << 20, (1 << 22) + 1, 1 << 31, (1 << 32) - 1)
           for i in (0, 1, 3, 429_496, 429_497, 429_498, 613_566, 1 << 20, (1 << 31) + 5, (1 << 32) - 1) if i <= d]
    for n_ins, depth in small + big:
        for prm in PARAMS:
            got, want = V.ins_classify_counts(n_ins, depth, *prm), I.classify(n_ins, depth, *prm)
            assert got == want, (n_ins, depth, prm, got, want)
            n[got] += 1
    assert min(n.values()) > 100, n


def test_rule_at_the_threshold_edges_and_past_32_bits():
    assert V.ins_classify_counts(7, 10, 1, 1, 7000) == V.INS_INSERTED == I.classify(7, 10, 1, 1, 7000)          # 7 / 10 exactly
    assert V.ins_classify_counts(6, 10, 1, 1, 7000) == V.INS_KEPT == I.classify(6, 10, 1, 1, 7000)              # one below
    for depth, per_10k in ((10, 7000), (10000, 1), (3, 3333), (30000, 3333), (2, 5000), (7, 10000), (1 << 20, 7000), (1 << 20, 4500)):
        i, rem = divmod(per_10k * depth, 10000)
        i += 1 if rem else 0                                           # the smallest count at or above the threshold
        assert V.ins_classify_counts(i, depth, 1, 1, per_10k) == V.INS_INSERTED == I.classify(i, depth, 1, 1, per_10k), (depth, per_10k)
        if i > 1:
            assert V.ins_classify_counts(i - 1, depth, 1, 1, per_10k) == V.INS_KEPT == I.classify(i - 1, depth, 1, 1, per_10k)
    # the left side alone wraps 32 bits: 10000 * 429 497 = 2^32 + 2704 against 4000 * 2^20 < 2^32
    assert 10000 * 429_497 > 1 << 32 > 4000 * (1 << 20)
    assert V.ins_classify_counts(429_497, 1 << 20, 1, 1, 4000) == V.INS_INSERTED
    assert V.ins_classify_counts(3, 3, 1, 3, 1) == V.INS_INSERTED and V.ins_classify_counts(2, 3, 1, 3, 1) == V.INS_KEPT
    assert V.ins_classify_counts(6, 10, 10, 1, 1) == V.INS_INSERTED and V.ins_classify_counts(6, 9, 10, 1, 1) == V.INS_LOW_DEPTH
    assert V.ins_classify_counts(0, 0, 1, 1, 1) == V.INS_LOW_DEPTH and V.ins_classify_counts(0, 50, 1, 1, 1) == V.INS_KEPT
    for prm in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 10001)):
        with pytest.raises(EngineError):
            V.ins_classify_counts(5, 5, *prm)


CODE = {c: i for i, c in enumerate(I.CODES)}


def ob(pos, seq, strand, length=None):
    """An observation of the inserted sequence `seq` (length: more bases than the key shows)."""
    return (pos, len(seq) if length is None else length) + I.make_key([CODE[c] for c in seq]) + (strand,)


def ins_obs(rows):
    o = np.zeros(len(rows), INS_OBS)
    for i, (pos, l, k0, k1, strand) in enumerate(rows):
        o[i] = (pos, l, (k0, k1), strand, 0)
    return o


def ins_cand(rows):
    c = np.zeros(len(rows), INS_CANDIDATE)
    for i, (pos, r, n_ins, depth, nf, nr, df, dr) in enumerate(rows):
        c[i] = (pos, ord(r), (0, 0, 0), n_ins, depth, nf, nr, df, dr)
    return c


def same_alleles(rows):
    got = V.ins_alleles(ins_obs(rows))
    assert got == I.alleles(sorted(rows)), rows
    return [(a["pos"], a["len"], a["seq"], a["count"], a["fwd"], a["rev"]) for a in got]


A32 = "ACGT" * 8


def test_alleles_of_hand_made_observations():
    assert V.ins_alleles(ins_obs([])) == [] == I.alleles([])
    # the most observations win, whatever the order they come in; the others follow by (len, key), not by count
    rows = [ob(10, "T", 0), ob(10, "CC", 1), ob(10, "CC", 0), ob(10, "A", 0), ob(10, "G", 1), ob(10, "G", 0), ob(10, "CC", 1), ob(7, "N", 1)]
    assert same_alleles(rows) == [(7, 1, "N", 1, 0, 1), (10, 2, "CC", 3, 1, 2), (10, 1, "A", 1, 1, 0), (10, 1, "G", 2, 1, 1), (10, 1, "T", 1, 1, 0)]
    assert same_alleles(rows[::-1]) == same_alleles(rows)
    # a tie by count: the smaller len; a tie by count and len: the smaller key
    assert same_alleles([ob(5, "GG", 0), ob(5, "T", 1), ob(5, "GG", 1), ob(5, "T", 0)])[0] == (5, 1, "T", 2, 1, 1)
    assert same_alleles([ob(5, "T", 0), ob(5, "G", 1), ob(5, "C", 0), ob(5, "=", 1)]) == [(5, 1, "=", 1, 0, 1), (5, 1, "C", 1, 1, 0), (5, 1, "G", 1, 0, 1),
                                                                                             (5, 1, "T", 1, 1, 0)]
    # lengths 32 and 33 with equal prefixes are two alleles; two of length 33 (and 100) with equal prefixes are one
    rows = [ob(9, A32, 0), ob(9, A32, 1, 33), ob(9, A32, 0, 33), ob(9, A32, 1, 100), ob(9, A32, 1, 100), ob(9, A32, 0, 100)]
    assert same_alleles(rows) == [(9, 100, A32, 3, 1, 2), (9, 32, A32, 1, 1, 0), (9, 33, A32, 2, 1, 1)]
    # a key that differs only in the second word, and only in its last nibble
    rows = [ob(3, "A" * 31 + "C", 0), ob(3, "A" * 31 + "A", 1), ob(3, "A" * 16 + "T" + "A" * 15, 0), ob(3, "A" * 31 + "C", 1)]
    assert same_alleles(rows) == [(3, 32, "A" * 31 + "C", 2, 1, 1), (3, 32, "A" * 32, 1, 0, 1), (3, 32, "A" * 16 + "T" + "A" * 15, 1, 1, 0)]
    assert V.ins_alleles(ins_obs(rows))[0]["key"] == (0x1111111111111111, 0x1111111111111112)
    # every code decodes, at an even and an odd nibble
    assert same_alleles([ob(2, I.CODES, 0), ob(2, "A" + I.CODES, 1)])[:2] == [(2, 16, I.CODES, 1, 1, 0), (2, 17, "A" + I.CODES, 1, 0, 1)]


CAND = [(101, "A", 4, 6, 2, 2, 3, 3), (102, "C", 3, 3, 3, 0, 3, 0), (5000, "N", 3, 40, 1, 2, 20, 20), (70000, "T", 2, 2, 1, 1, 1, 1)]
OBS = ([ob(101, "C", 0), ob(101, "CC", 1), ob(101, "C", 1), ob(101, "CC", 0)] + [ob(102, "GAT", 0)] * 3
       + [ob(5000, A32, 0, 33), ob(5000, A32, 1, 33), ob(5000, A32, 1, 32)] + [ob(70000, A32, 0), ob(70000, "R=N", 1)])


def test_tsv_writer_against_the_reference_and_a_hand_written_file(tmp_path):
    res = InsResult(start=100, end=70_100, low_depth=5, kept=70_000 - 5 - len(CAND), inserted=len(CAND), candidates=ins_cand(CAND), observations=ins_obs(OBS))
    exp = dict(low_depth=5, kept=res.kept, inserted=res.inserted, candidates=CAND)
    out = str(tmp_path / "i.tsv")
    V.write_insertions(out, "chrM", res, 10, 20, 3, 7000, min_base_quality=20, exclude_flags=0x704, min_ins_per_strand=2)
    text = open(out, "rb").read().decode()
    assert text == I.expected_tsv("chrM", exp, sorted(OBS), 100, 70_100, 10, 20, 20, 0x704, 7000, 3, 2)
    assert text == ("##contig=chrM\n##range=100-70100\n##min_depth=10\n##min_quality=20\n##min_base_quality=20\n##exclude_flags=0x0704\n"
                    f"##min_ins_fraction=0.7000\n##min_ins_count=3\n##positions=70000\n##low_depth=5\n##kept={res.kept}\n##inserted=4\n"
                    "#contig\tpos\tref\tins\tdepth\tfreq\talleles\tlength\tseq\tallele_count\tallele_fwd\tallele_rev\tins_fwd\tins_rev\tfilter\n"
                    "chrM\t101\tA\t4\t6\t0.6667\t2\t1\tC\t2\t1\t1\t2\t2\tPASS\n"
                    "chrM\t102\tC\t3\t3\t1.0000\t1\t3\tGAT\t3\t3\t0\t3\t0\tstrand\n"
                    f"chrM\t5000\tN\t3\t40\t0.0750\t2\t33\t{A32}...\t2\t1\t1\t1\t2\tstrand\n"
                    "chrM\t70000\tT\t2\t2\t1.0000\t2\t3\tR=N\t1\t0\t1\t1\t1\tstrand\n")
    # K = 0: always PASS; no base-quality threshold: "."; another fraction
    V.write_insertions(out, "chrM", res, 10, 20, 1, 125)
    text = open(out).read()
    assert "##min_base_quality=.\n##exclude_flags=0x0000\n##min_ins_fraction=0.0125\n##min_ins_count=1\n" in text
    assert "strand" not in text and text.count("\tPASS\n") == 4
    assert text == I.expected_tsv("chrM", exp, sorted(OBS), 100, 70_100, 10, 20, None, 0, 125, 1, 0)
    none = InsResult(0, 10, 3, 7, 0, ins_cand([]), ins_obs([]))
    V.write_insertions(out, "chrM", none, 10, 20, 3, 10000)
    assert open(out).read() == I.expected_tsv("chrM", dict(low_depth=3, kept=7, inserted=0, candidates=[]), [], 0, 10, 10, 20, None, 0, 10000, 3, 0)
    with pytest.raises(ValueError):
        V.write_insertions(out, "chrM", InsResult(0, 10, 0, 7, 3, ins_cand(CAND), ins_obs(OBS)), 10, 20, 1, 125)     # 3 claimed, 4 given
    with pytest.raises(EngineError):                                    # a candidate with fewer observations than its ins
        V.write_insertions(out, "chrM", InsResult(100, 70_100, 5, res.kept, 4, ins_cand(CAND), ins_obs(OBS[1:])), 10, 20, 1, 125)
    with pytest.raises(EngineError):                                    # observations where no candidate is
        V.write_insertions(out, "chrM", InsResult(100, 70_100, 5, res.kept, 4, ins_cand(CAND), ins_obs(OBS + [ob(9, "A", 0)])), 10, 20, 1, 125)


def cli(tmp_path, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="9999")                  # no device can be opened
    return subprocess.run([_b.CLI, "find-insertions", str(tmp_path / "none.bam"), "-r", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.tsv")]
                          + list(args), capture_output=True, text=True, env=env)


@pytest.mark.parametrize("args,msg", [
    ([], "needs '-L <CONTIG>'"),
    (["-L", "chrM", "--region", "100"], "invalid value '100' for '--region'"),
    (["-L", "chrM", "--region", "200-100"], "invalid value '200-100' for '--region'"),
    (["-L", "chrM", "--min-ins-fraction", "0"], "invalid value '0' for '--min-ins-fraction'"),
    (["-L", "chrM", "--min-ins-fraction", "1.0001"], "invalid value '1.0001' for '--min-ins-fraction'"),
    (["-L", "chrM", "--min-ins-fraction=0.70001"], "invalid value '0.70001' for '--min-ins-fraction'"),
    (["-L", "chrM", "--min-ins-fraction", "70%"], "invalid value '70%' for '--min-ins-fraction'"),
    (["-L", "chrM", "--min-ins-count", "0"], "invalid value '0' for '--min-ins-count'"),
    (["-L", "chrM", "--min-ins-count=x"], "invalid value 'x' for '--min-ins-count'"),
    (["-L", "chrM", "--min-base-quality", "256"], "invalid value '256' for '--min-base-quality'"),
    (["-L", "chrM", "--exclude-flags", "0xZZ"], "invalid value '0xZZ' for '--exclude-flags'"),
    (["-L", "chrM", "--min-ins-per-strand", "-1"], "invalid value '-1' for '--min-ins-per-strand'"),
    (["-L", "chrM", "--min-depth", "0"], "invalid value '0' for '--min-depth'"),
    (["-L", "chrM", "--min-del-fraction", "0.5"], "unexpected argument '--min-del-fraction'"),
])
def test_cli_argument_errors_exit_2_before_a_device_is_opened(tmp_path, args, msg):
    r = cli(tmp_path, *args)
    assert r.returncode == 2, r.stderr
    assert msg in r.stderr, r.stderr


def test_cli_accepts_well_formed_values_and_names_the_subcommand(tmp_path):
    """The argument check passes: the run then fails on the missing BAM with exit 1, not 2, still without a device."""
    for args in (["-L", "chrM"], ["-L", "chrM", "--min-ins-fraction", "1", "--min-ins-count=1"],
                 ["-L", "chrM", "--region=5-6", "--exclude-flags", "0x704", "--min-base-quality", "0", "--min-ins-per-strand=2", "--min-ins-fraction=.0001"]):
        r = cli(tmp_path, *args)
        assert r.returncode == 1 and "invalid value" not in r.stderr, (args, r.stderr)
    r = subprocess.run([_b.CLI, "--help"], capture_output=True, text=True)
    assert "find-insertions" in r.stdout + r.stderr and "--min-ins-fraction" in r.stdout + r.stderr
    r = subprocess.run([_b.CLI, "find-insertions", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "find-insertions" in r.stderr


def test_a_context_without_a_device_answers_a_device_error():
    with HostStage(CallableOptions()) as h:
        for flt in (None, (0x704, True)):
            with pytest.raises(EngineError) as e:
                h.site_scan_ins(20, 10, 3, 7000, np.zeros(100, np.uint8), filter=flt)
            assert e.value.status == -2
