"""The host side of the filtered, strand-aware site scan, without a device: the independent reference tests/scan_ref.py
tied to the committed oracle, the extended TSV writer, the CLI's argument checks, the pass-bit realignment of
cl_site_attach_quals (qual_off numbering -> seq_off numbering) and its refusal on a context without a device."""
import subprocess

import numpy as np
import pytest

import oracle
import scan_ref as R
from helpers import load_kats
from decodingustools_amd import CallableOptions, EngineError, build as _b, synth, variants as V
from decodingustools_amd.callable_loci import SCAN_CANDIDATE, SCAN_CANDIDATE_EX, HostStage, ScanResult, site_pass_bits
from decodingustools_amd.records import ContigRecords, pack_seq4

KATS = load_kats()


def oracle_hist(L, ref, rec, min_quality):
    return oracle.site_pileup(1, min_quality, L, ref, rec, np.arange(1, L + 1, dtype=np.uint32))["hist"]


def with_random_seq(rec, seed, all_codes=True):
    rng = np.random.default_rng(seed)
    n = int(rec.qual_off[-1])
    codes = rng.integers(0, 16, n, dtype=np.uint8) if all_codes else np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, n)]
    rec.seq_off = rec.qual_off.copy()
    rec.seq4 = pack_seq4(codes)
    return rec


def tie(L, ref, rec, qualities, what):
    for mq in qualities:
        h2 = R.stranded_hist(L, ref.shape[0], rec, mq)
        want = oracle_hist(L, ref, rec, mq)
        got = h2[0] + h2[1]
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (what, mq, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("case", KATS["site_cases"], ids=[c["name"] for c in KATS["site_cases"]])
def test_reference_equals_the_oracle_on_site_kats(case):
    rec = ContigRecords.from_reads([tuple(r) for r in case["reads"]])
    ref = np.frombuffer(case["ref"].encode(), dtype=np.uint8).copy()
    tie(case["contig_len"], ref, rec, (0, case["min_quality"], 61), case["name"])


def test_reference_equals_the_oracle_on_adversarial_and_short_read_tiles():
    for seed, L, n, overhang in ((1, 3000, 600, False), (2, 5000, 1500, True), (3, 2048, 900, True), (4, 700, 300, False)):
        rec = with_random_seq(synth.adversarial_contig(L, n, seed, overhang=overhang, deep=(seed == 2)), 100 + seed)
        # flags must not matter with the filter off: every bit somewhere
        rec.flag = np.random.default_rng(seed).integers(0, 1 << 16, rec.n, dtype=np.uint16)
        ref = synth.make_reference(L, 50 + seed, lowercase=True)
        tie(L, ref, rec, (0, 10, 61), ("adversarial", seed))
        tie(L, ref[:L - 300], rec, (10,), ("adversarial, short reference", seed))
    L = 30_000
    ref = synth.make_reference(L, 7)
    tie(L, ref, synth.short_read_contig(L, 30, 11, with_seq=True, ref=ref), (0, 20), "short reads")


def test_reference_filters_do_something_and_only_remove():
    L = 20_000
    ref = synth.make_reference(L, 7)
    rec = synth.short_read_contig(L, 30, 13, with_seq=True, ref=ref)
    rec.flag = rec.flag | (np.random.default_rng(1).integers(0, 2, rec.n).astype(np.uint16) << np.uint16(4))
    off = R.stranded_hist(L, L, rec, 20)
    assert off[0].sum() > 0 and off[1].sum() > 0
    last = off
    for ex, bq in ((0x704, None), (0x704, 20), (0xFFFF, 20)):
        h = R.stranded_hist(L, L, rec, 20, ex, bq)
        assert (h <= last).all() and 0 < int(h.sum()) < int(last.sum())
        last = h
    # exclude_flags == 0xFFFF counts only reads with flag == 0: none of them is reverse
    assert R.stranded_hist(L, L, rec, 20, 0xFFFF)[1].sum() == 0 and np.count_nonzero(rec.flag == 0) > 0


def cand_ex(rows):
    c = np.zeros(len(rows), SCAN_CANDIDATE_EX)
    for i, (pos, r, alt, a, cc, g, t, depth, af, ar, rf, rr) in enumerate(rows):
        c[i] = (pos, ord(r), ord(alt), (0, 0), a, cc, g, t, depth, af, ar, rf, rr)
    return c


ROWS = [(101, "A", "C", 1, 20, 0, 0, 21, 11, 9, 1, 0), (2500, "G", "T", 0, 0, 2, 30, 32, 30, 0, 1, 1),
        (2501, "C", "A", 12, 1, 0, 0, 13, 2, 10, 0, 1), (70000, "T", "G", 0, 0, 40, 3, 44, 20, 20, 3, 0)]


def test_extended_tsv_writer_against_a_hand_written_file(tmp_path):
    res = ScanResult(start=100, end=70_100, low_depth=5, mixed=6, uncomparable=7, match=69_978, variant=4, candidates=cand_ex(ROWS))
    out = str(tmp_path / "x.tsv")
    V.write_variants_ex(out, "chrY", res, 10, 20, min_base_quality=20, exclude_flags=0x704, min_alt_per_strand=3)
    head = ("##contig=chrY\n##range=100-70100\n##min_depth=10\n##min_quality=20\n##min_base_quality=20\n##exclude_flags=0x0704\n"
            "##positions=70000\n##low_depth=5\n##mixed=6\n##uncomparable=7\n##match=69978\n##variant=4\n"
            "#contig\tpos\tref\talt\tdepth\tA\tC\tG\tT\tfreq\tstatus\tnames\talleles\talt_fwd\talt_rev\tref_fwd\tref_rev\tfilter\n")
    want = head + ("chrY\t101\tA\tC\t21\t1\t20\t0\t0\t0.9524\t.\t.\t.\t11\t9\t1\t0\tPASS\n"
                   "chrY\t2500\tG\tT\t32\t0\t0\t2\t30\t0.9375\t.\t.\t.\t30\t0\t1\t1\tstrand\n"
                   "chrY\t2501\tC\tA\t13\t12\t1\t0\t0\t0.9231\t.\t.\t.\t2\t10\t0\t1\tstrand\n"
                   "chrY\t70000\tT\tG\t44\t0\t0\t40\t3\t0.9091\t.\t.\t.\t20\t20\t3\t0\tPASS\n")
    assert open(out).read() == want
    # K = 0: always PASS; no base-quality threshold: "."; the reference's own builder writes the same text
    V.write_variants_ex(out, "chrY", res, 10, 20, exclude_flags=0)
    text = open(out).read()
    assert "##min_base_quality=.\n##exclude_flags=0x0000\n" in text and "strand" not in text and text.count("\tPASS\n") == 4
    exp = dict(low_depth=5, mixed=6, uncomparable=7, match=69_978, variant=4, candidates=ROWS)
    assert text == R.expected_tsv_ex("chrY", exp, 100, 70_100, 10, 20, None, 0, 0)
    assert want == R.expected_tsv_ex("chrY", exp, 100, 70_100, 10, 20, 20, 0x704, 3)


def test_annotated_extended_tsv_has_a_known_and_a_novel_line(tmp_path):
    import json
    from decodingustools_amd import haplogroup as H

    def node(i, name, root, parent, children, variants):
        n = {"haplogroupId": i, "name": name, "isRoot": root, "root": "R", "kitsCount": 1, "subBranches": 0, "bigYCount": 2,
             "variants": variants, "children": children}
        if parent:
            n["parentId"] = parent
        return n
    x1 = {"variant": "X1", "ancestral": "G", "derived": "T", "region": "x", "id": 7, "position": 2500}
    text = json.dumps({"allNodes": {"1": node(1, "R", True, 0, [2], []), "2": node(2, "R-X1", False, 1, [], [x1])}})
    t = H.HaplogroupTree(text, H.FTDNA, H.YDNA)
    res = ScanResult(start=100, end=70_100, low_depth=5, mixed=6, uncomparable=7, match=69_978, variant=4, candidates=cand_ex(ROWS))
    out = str(tmp_path / "x.tsv")
    V.write_variants_ex(out, "chrY", res, 10, 20, min_base_quality=20, exclude_flags=0x704, min_alt_per_strand=1, tree=t, build_id="GRCh38")
    lines = [l for l in open(out).read().splitlines() if not l.startswith("#")]
    assert lines[0] == "chrY\t101\tA\tC\t21\t1\t20\t0\t0\t0.9524\tnovel\t.\t.\t11\t9\t1\t0\tPASS"
    assert lines[1] == "chrY\t2500\tG\tT\t32\t0\t0\t2\t30\t0.9375\tknown\tX1\tderived\t30\t0\t1\t1\tstrand"
    assert [l.split("\t")[10] for l in lines] == ["novel", "known", "novel", "novel"]


def test_old_writer_bytes_are_unchanged(tmp_path):
    c = np.zeros(2, SCAN_CANDIDATE)
    c[0] = (101, ord("A"), ord("C"), (0, 0), 1, 20, 0, 0, 21)
    c[1] = (2500, ord("G"), ord("T"), (0, 0), 0, 0, 2, 30, 32)
    res = ScanResult(start=0, end=3000, low_depth=1, mixed=2, uncomparable=3, match=2992, variant=2, candidates=c)
    out = str(tmp_path / "o.tsv")
    V.write_variants(out, "chrM", res, 10, 20)
    assert open(out).read() == ("##contig=chrM\n##range=0-3000\n##min_depth=10\n##min_quality=20\n##positions=3000\n##low_depth=1\n##mixed=2\n"
                                "##uncomparable=3\n##match=2992\n##variant=2\n"
                                "#contig\tpos\tref\talt\tdepth\tA\tC\tG\tT\tfreq\tstatus\tnames\talleles\n"
                                "chrM\t101\tA\tC\t21\t1\t20\t0\t0\t0.9524\t.\t.\t.\n"
                                "chrM\t2500\tG\tT\t32\t0\t0\t2\t30\t0.9375\t.\t.\t.\n")


@pytest.mark.parametrize("flag,value", [("--min-base-quality", "256"), ("--exclude-flags", "65536"), ("--exclude-flags", "0xZZ"),
                                        ("--min-alt-per-strand", "x"), ("--exclude-flags", "0x"), ("--min-base-quality", "-1")])
def test_cli_refuses_malformed_filter_values(tmp_path, flag, value):
    for args in ([flag, value], [f"{flag}={value}"]):
        r = subprocess.run([_b.CLI, "find-variants", str(tmp_path / "none.bam"), "-r", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.tsv"),
                            "-L", "chrY"] + args, capture_output=True, text=True)
        assert r.returncode == 2, r.stderr
        assert f"invalid value '{value}' for '{flag}'" in r.stderr, r.stderr


def test_cli_accepts_well_formed_filter_values(tmp_path):
    """Decimal and 0x masks pass the argument check: the run then fails on the missing BAM with exit 1, not 2."""
    for args in (["--exclude-flags", "0x704"], ["--exclude-flags=1796", "--min-base-quality", "0"], ["--min-alt-per-strand=2"], ["--exclude-flags", "0XfFfF"]):
        r = subprocess.run([_b.CLI, "find-variants", str(tmp_path / "none.bam"), "-r", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.tsv"),
                            "-L", "chrY"] + args, capture_output=True, text=True)
        assert r.returncode == 1 and "invalid value" not in r.stderr, (args, r.stderr)


def test_attachment_on_a_context_without_a_device_is_a_device_error():
    rec = ContigRecords.from_reads([(10, "20M", 60, 30, 0, "a", "ACGT" * 5)])
    with HostStage(CallableOptions()) as h:
        with pytest.raises(EngineError) as e:
            h.site_attach_quals(rec, 20)
        assert e.value.status == -2
        with pytest.raises(EngineError) as e:
            h.site_scan_ex(20, 10, np.zeros(100, np.uint8), 0x704, True)
        assert e.value.status == -2


def numpy_pass_bits(rec, thr):
    n = int(rec.seq_off[-1])
    bits = np.zeros(((n + 63) // 64) * 64, np.uint8)
    for r in range(rec.n):
        s0, s1 = int(rec.seq_off[r]), int(rec.seq_off[r + 1])
        q0, q1 = int(rec.qual_off[r]), int(rec.qual_off[r + 1])
        for i in range(s1 - s0):
            bits[s0 + i] = 1 if i >= q1 - q0 else int(rec.qual[q0 + i] >= thr)
    return np.packbits(bits, bitorder="little").view(np.uint64)


def test_pass_bits_are_realigned_from_quality_to_base_numbering():
    rng = np.random.default_rng(9)
    reads = []
    for i in range(400):
        l = int(rng.choice([1, 7, 63, 64, 65, 100, 128, 150, 300, 1000]))
        kind = i % 5
        if kind == 0:
            q = None                                                        # no quality values at all
        elif kind == 1:
            q = [int(x) for x in rng.integers(0, 45, max(0, l - int(rng.integers(1, l + 1))))]   # fewer values than bases
        elif kind == 2:
            q = [255] * l                                                   # absent qualities
        else:
            q = [int(x) for x in rng.choice([2, 12, 19, 20, 21, 37, 255], l)]
        seq = "".join(rng.choice(list("ACGTN"), l))
        reads.append((i * 3, f"{l}M", 60, q, 0, f"r{i}", seq))
    rec = ContigRecords.from_reads(reads)
    assert not np.array_equal(rec.seq_off, rec.qual_off)
    for thr in (0, 20, 21, 255):
        got = site_pass_bits(rec, thr)
        want = numpy_pass_bits(rec, thr)
        assert np.array_equal(got, want), thr
    # a sliced tile: base offsets that do not start at zero, bits before the first read are zero
    sl = rec.slice(100, 300)
    assert int(sl.seq_off[0]) > 0
    want = numpy_pass_bits(sl, 20)
    assert np.array_equal(site_pass_bits(sl, 20), want) and not want[:int(sl.seq_off[0]) // 64].any()
    # a threshold that separates: some bits differ between 20 and 21, 0xFF and missing values pass at 255
    assert not np.array_equal(site_pass_bits(rec, 20), site_pass_bits(rec, 21))
    assert int(np.unpackbits(site_pass_bits(rec, 255).view(np.uint8)).sum()) > 0
