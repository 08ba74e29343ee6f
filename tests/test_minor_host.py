"""The host side of find-minor-alleles, without a device: the fraction parser, the second-allele rule in plain C++ against
the independent reference tests/minor_ref.py, the TSV writer against a hand-written file, the CLI's argument checks."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import minor_ref as M
from decodingustools_amd import CallableOptions, EngineError, build as _b, variants as V
from decodingustools_amd.callable_loci import MINOR_CANDIDATE, HostStage, MinorResult


@pytest.mark.parametrize("text,want", [("0.05", 500), ("0.5", 5000), (".0125", 125), ("0.5000", 5000), ("0.0001", 1), ("00.25", 2500),
                                       ("0.3", 3000), (".5", 5000)])
def test_fraction_parser_accepts(text, want):
    assert V.minor_fraction_parse(text) == want


@pytest.mark.parametrize("text", ["0", "0.50001", "0.6", "0.12345", "", "1e-2", "0.05x", "0.0", "0.0000", "1", "-0.1", "+0.1", ".", "0.5001",
                                  " 0.05", "0,05"])
def test_fraction_parser_rejects(text):
    with pytest.raises(ValueError):
        V.minor_fraction_parse(text)


PARAMS = [(1, 1, 1), (2, 1, 2500), (5, 3, 500), (10, 2, 5000), (4, 4, 3333)]


def test_rule_equals_the_reference_on_every_small_count_vector():
    n = {M.LOW_DEPTH: 0, M.SINGLE: 0, M.MINOR: 0}
    for a, c, g, t in itertools.product(range(13), repeat=4):
        for other in (0, 3):
            depth = a + c + g + t + other
            for prm in PARAMS[:3] if (a + c + g + t) % 3 else PARAMS:       # (every vector meets three triples, a third of them all five)
                got = V.minor_classify_counts(a, c, g, t, depth, *prm)
                want = M.classify(a, c, g, t, depth, *prm)
                assert got == want, ((a, c, g, t, other), prm, got, want)
                n[got[0]] += 1
    assert min(n.values()) > 500, n


def test_the_reference_over_arrays_equals_the_reference_of_one_position():
    rng = np.random.default_rng(3)
    acgt = np.concatenate([rng.integers(0, 6, (4000, 4)), rng.integers(0, 1 << 31, (500, 4)), np.array([[(1 << 20) - 429_497, 429_497, 0, 0]])])
    depth = acgt.sum(1) + rng.integers(0, 4, acgt.shape[0]) * rng.integers(0, 50, acgt.shape[0])
    for prm in PARAMS + [(1, 1, 4000)]:
        cls, mi, ni = M.classify_arrays(acgt, depth, *prm)
        for k in range(acgt.shape[0]):
            assert (int(cls[k]), "ACGT"[mi[k]], "ACGT"[ni[k]]) == M.classify(*acgt[k], depth[k], *prm), (acgt[k], depth[k], prm)


def test_rule_at_the_threshold_edges_and_past_32_bits():
    # 10000 * c2 == per_10k * depth exactly, and one count below it
    for depth, per_10k in ((10000, 500), (40, 2500), (10000, 1), (3, 3333), (30000, 3333), (2, 5000)):
        c2, rem = divmod(per_10k * depth, 10000)
        if rem:
            c2 += 1                                                    # the smallest count at or above the threshold
        got = V.minor_classify_counts(depth - c2, 0, c2, 0, depth, 1, 1, per_10k)
        assert got == (V.MINOR_MINOR, "A", "G") == M.classify(depth - c2, 0, c2, 0, depth, 1, 1, per_10k), (depth, per_10k)
        if c2 > 1:
            got = V.minor_classify_counts(depth - c2 + 1, 0, c2 - 1, 0, depth, 1, 1, per_10k)
            assert got == (V.MINOR_SINGLE, "A", "G") == M.classify(depth - c2 + 1, 0, c2 - 1, 0, depth, 1, 1, per_10k), (depth, per_10k)
    # exactly at min_minor_count and one below
    assert V.minor_classify_counts(20, 3, 0, 0, 23, 1, 3, 1)[0] == V.MINOR_MINOR
    assert V.minor_classify_counts(20, 2, 0, 0, 22, 1, 3, 1)[0] == V.MINOR_SINGLE
    # products past 2^32: 10000 * 2^22 = 5000 * 2^23 = 41 943 040 000; and a column whose left side alone wraps
    # (10000 * 429 497 = 2^32 + 2704 against 4000 * 2^20 < 2^32: a 32-bit product calls it single)
    assert V.minor_classify_counts((1 << 20) - 429_497, 429_497, 0, 0, 1 << 20, 1, 1, 4000) == (V.MINOR_MINOR, "A", "C") == \
        M.classify((1 << 20) - 429_497, 429_497, 0, 0, 1 << 20, 1, 1, 4000)
    c2, depth = 1 << 22, 1 << 23
    assert V.minor_classify_counts(depth - c2, 0, 0, c2, depth, 1, 1, 5000) == (V.MINOR_MINOR, "A", "T") == M.classify(depth - c2, 0, 0, c2, depth, 1, 1, 5000)
    assert V.minor_classify_counts(depth - c2 + 1, 0, 0, c2 - 1, depth, 1, 1, 5000)[0] == V.MINOR_SINGLE
    # depth counts N and the other codes: 5 of 10 named bases are a second allele at 0.5, 5 of 10 + 3 others are not
    assert V.minor_classify_counts(5, 5, 0, 0, 10, 1, 1, 5000)[0] == V.MINOR_MINOR
    assert V.minor_classify_counts(5, 5, 0, 0, 13, 1, 1, 5000)[0] == V.MINOR_SINGLE
    assert V.minor_classify_counts(5, 5, 0, 0, 13, 14, 1, 1)[0] == V.MINOR_LOW_DEPTH


def test_rule_breaks_ties_in_the_order_a_c_g_t():
    for counts, want in (((7, 7, 0, 0), ("A", "C")), ((9, 4, 4, 4), ("A", "C")), ((1, 4, 4, 4), ("C", "G")), ((5, 5, 5, 5), ("A", "C")),
                         ((0, 0, 0, 0), ("A", "C")), ((0, 3, 0, 3), ("C", "T")), ((2, 0, 2, 9), ("T", "A")), ((0, 0, 6, 0), ("G", "A")),
                         ((0, 0, 0, 6), ("T", "A")), ((6, 0, 0, 0), ("A", "C")), ((3, 8, 3, 3), ("C", "A")), ((3, 3, 8, 8), ("G", "T"))):
        got = V.minor_classify_counts(*counts, sum(counts), 1, 1, 1)
        assert got[1:] == want == M.classify(*counts, sum(counts), 1, 1, 1)[1:], counts


def test_rule_refuses_what_the_scan_refuses():
    for prm in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 5001)):
        with pytest.raises(EngineError):
            V.minor_classify_counts(5, 5, 0, 0, 10, *prm)
    with pytest.raises(EngineError):
        V.minor_classify_counts(5, 5, 0, 0, 9, 1, 1, 1)                  # the named bases exceed the depth


ROWS = [(101, "A", "A", "C", 15, 6, 0, 0, 21, 8, 7, 4, 2), (2500, "G", "T", "G", 0, 1, 10, 20, 32, 20, 0, 10, 0),
        (2501, "N", "C", "A", 6, 7, 0, 0, 13, 0, 7, 1, 5), (70000, "T", "G", "T", 0, 0, 40, 4, 44, 20, 20, 2, 2)]


def minor_cand(rows):
    c = np.zeros(len(rows), MINOR_CANDIDATE)
    for i, (pos, r, major, minor, a, cc, g, t, depth, mf, mr, nf, nr) in enumerate(rows):
        c[i] = (pos, ord(r), ord(major), ord(minor), 0, a, cc, g, t, depth, mf, mr, nf, nr)
    return c


def test_tsv_writer_against_a_hand_written_file(tmp_path):
    res = MinorResult(start=100, end=70_100, low_depth=5, single=69_991, minor=4, candidates=minor_cand(ROWS))
    out = str(tmp_path / "m.tsv")
    V.write_minor(out, "chrM", res, 10, 20, 3, 500, min_base_quality=20, exclude_flags=0x704, min_minor_per_strand=2)
    want = ("##contig=chrM\n##range=100-70100\n##min_depth=10\n##min_quality=20\n##min_base_quality=20\n##exclude_flags=0x0704\n"
            "##min_minor_fraction=0.0500\n##min_minor_count=3\n##positions=70000\n##low_depth=5\n##single=69991\n##minor=4\n"
            "#contig\tpos\tref\tmajor\tminor\tdepth\tA\tC\tG\tT\tminor_freq\tmajor_fwd\tmajor_rev\tminor_fwd\tminor_rev\tfilter\n"
            "chrM\t101\tA\tA\tC\t21\t15\t6\t0\t0\t0.2857\t8\t7\t4\t2\tPASS\n"
            "chrM\t2500\tG\tT\tG\t32\t0\t1\t10\t20\t0.3125\t20\t0\t10\t0\tstrand\n"
            "chrM\t2501\tN\tC\tA\t13\t6\t7\t0\t0\t0.4615\t0\t7\t1\t5\tstrand\n"
            "chrM\t70000\tT\tG\tT\t44\t0\t0\t40\t4\t0.0909\t20\t20\t2\t2\tPASS\n")
    assert open(out, "rb").read() == want.encode()
    exp = dict(low_depth=5, single=69_991, minor=4, candidates=ROWS)
    assert want == M.expected_tsv("chrM", exp, 100, 70_100, 10, 20, 20, 0x704, 500, 3, 2)
    # K = 0: always PASS; no base-quality threshold: "."; another fraction
    V.write_minor(out, "chrM", res, 10, 20, 1, 125)
    text = open(out).read()
    assert "##min_base_quality=.\n##exclude_flags=0x0000\n##min_minor_fraction=0.0125\n##min_minor_count=1\n" in text
    assert "strand" not in text and text.count("\tPASS\n") == 4
    assert text == M.expected_tsv("chrM", exp, 100, 70_100, 10, 20, None, 0, 125, 1, 0)
    with pytest.raises(ValueError):
        V.write_minor(out, "chrM", MinorResult(0, 10, 0, 7, 3, minor_cand(ROWS)), 10, 20, 1, 125)     # 3 claimed, 4 given


def cli(tmp_path, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="9999")                  # no device can be opened
    return subprocess.run([_b.CLI, "find-minor-alleles", str(tmp_path / "none.bam"), "-r", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.tsv")]
                          + list(args), capture_output=True, text=True, env=env)


@pytest.mark.parametrize("args,msg", [
    ([], "needs '-L <CONTIG>'"),
    (["-L", "chrM", "--region", "100"], "invalid value '100' for '--region'"),
    (["-L", "chrM", "--region", "200-100"], "invalid value '200-100' for '--region'"),
    (["-L", "chrM", "--region=a-b"], "invalid value 'a' for '--region'"),
    (["-L", "chrM", "--min-minor-fraction", "0"], "invalid value '0' for '--min-minor-fraction'"),
    (["-L", "chrM", "--min-minor-fraction", "0.6"], "invalid value '0.6' for '--min-minor-fraction'"),
    (["-L", "chrM", "--min-minor-fraction=0.50001"], "invalid value '0.50001' for '--min-minor-fraction'"),
    (["-L", "chrM", "--min-minor-fraction", "1e-2"], "invalid value '1e-2' for '--min-minor-fraction'"),
    (["-L", "chrM", "--min-minor-fraction", "5%"], "invalid value '5%' for '--min-minor-fraction'"),
    (["-L", "chrM", "--min-minor-count", "0"], "invalid value '0' for '--min-minor-count'"),
    (["-L", "chrM", "--min-minor-count=x"], "invalid value 'x' for '--min-minor-count'"),
    (["-L", "chrM", "--min-base-quality", "256"], "invalid value '256' for '--min-base-quality'"),
    (["-L", "chrM", "--exclude-flags", "0xZZ"], "invalid value '0xZZ' for '--exclude-flags'"),
    (["-L", "chrM", "--exclude-flags=65536"], "invalid value '65536' for '--exclude-flags'"),
    (["-L", "chrM", "--min-minor-per-strand", "-1"], "invalid value '-1' for '--min-minor-per-strand'"),
    (["-L", "chrM", "--min-depth", "0"], "invalid value '0' for '--min-depth'"),
    (["-L", "chrM", "--no-such-flag"], "unexpected argument '--no-such-flag'"),
])
def test_cli_argument_errors_exit_2_before_a_device_is_opened(tmp_path, args, msg):
    r = cli(tmp_path, *args)
    assert r.returncode == 2, r.stderr
    assert msg in r.stderr, r.stderr


def test_cli_accepts_well_formed_values(tmp_path):
    """The argument check passes: the run then fails on the missing BAM with exit 1, not 2, still without a device."""
    for args in (["-L", "chrM"], ["-L", "chrM", "--min-minor-fraction", ".0125", "--min-minor-count=1"],
                 ["-L", "chrM", "--region=5-6", "--exclude-flags", "0x704", "--min-base-quality", "0", "--min-minor-per-strand=2", "--min-minor-fraction=0.5"]):
        r = cli(tmp_path, *args)
        assert r.returncode == 1 and "invalid value" not in r.stderr, (args, r.stderr)


def test_a_context_without_a_device_answers_a_device_error():
    with HostStage(CallableOptions()) as h:
        with pytest.raises(EngineError) as e:
            h.site_scan_minor(20, 10, 3, 500, np.zeros(100, np.uint8))
        assert e.value.status == -2
        with pytest.raises(EngineError) as e:
            h.site_scan_minor(20, 10, 3, 500, np.zeros(100, np.uint8), filter=(0x704, True))
        assert e.value.status == -2
