"""The host side of the per-target summaries, no device: tests/targets_ref.py against a per-position loop, the BED reader
(dut_targets_parse), the threshold list, the table writer against golden text, and the tool's argument errors."""
import os
import subprocess

import numpy as np
import pytest

import targets_ref
from decodingustools_amd import EngineError, TargetStats, build as _b, parse_targets, thresholds_parse, write_target_stats

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def run(*args, cwd=None):
    return subprocess.run([_b.CLI] + list(args), capture_output=True, text=True, cwd=cwd)


# ---- the reference rule itself ----
@pytest.mark.parametrize("seed", range(6))
def test_reference_against_the_per_position_loop(seed):
    rng = np.random.default_rng(seed)
    extent = [0, 1, 7, 40, 64, 100][seed]
    raw = rng.integers(0, 40, extent)
    qc = np.minimum(raw, rng.integers(0, 40, extent))
    state = rng.integers(0, 6, extent)
    starts = rng.integers(0, extent + 10, 60)
    ends = starts + np.where(rng.random(60) < 0.3, 0, rng.integers(0, extent + 10, 60))
    for thr in ((), (1,), (1, 10, 20, 30), (1, 2, 3, 5, 8, 13, 21, 1000)):
        a = targets_ref.target_stats(raw, qc, state, starts, ends, thr)
        b = targets_ref.target_stats_loop(raw, qc, state, starts, ends, thr)
        targets_ref.same(a, b, (seed, thr))
        assert np.array_equal(a["state"].sum(axis=1), a["len"])


def test_reference_clips_and_keeps_the_order():
    raw = np.arange(10); qc = raw // 2; state = np.array([0, 1, 1, 1, 2, 3, 4, 5, 1, 1])
    st = targets_ref.target_stats(raw, qc, state, [8, 0, 10, 5, 3], [12, 10, 15, 100, 3], (1, 5))
    assert st["start"].tolist() == [8, 0, 10, 5, 3] and st["end"].tolist() == [10, 10, 10, 10, 3] and st["len"].tolist() == [2, 10, 0, 5, 0]
    assert st["sum_raw"].tolist() == [17, 45, 0, 35, 0] and st["sum_qc"].tolist() == [8, 20, 0, 16, 0]
    assert st["state"][1].tolist() == [1, 5, 1, 1, 1, 1] and st["ge_raw"][1].tolist() == [9, 5] and st["ge_qc"][1].tolist() == [8, 0]


# ---- the BED reader ----
def test_parser_groups_by_contig_in_file_order():
    text = ("track name=x\nbrowser position chr1\n# comment\n\nchr2\t5\t9\tb1\textra\tcolumns\nchr1\t0\t10\r\nchr2 7 7 b2\n"
            "chr1\t4294967295\t4294967295\tlast\n   \nchr3\t1\t2\tno_newline")
    got = parse_targets(text)
    assert [g[0] for g in got] == ["chr2", "chr1", "chr3"]
    assert got[0][1].tolist() == [5, 7] and got[0][2].tolist() == [9, 7] and got[0][3] == ["b1", "b2"]
    assert got[1][1].tolist() == [0, 4294967295] and got[1][2].tolist() == [10, 4294967295] and got[1][3] == [".", "last"]
    assert got[2][1].tolist() == [1] and got[2][3] == ["no_newline"]
    assert got[0][1].dtype == np.uint32
    assert parse_targets("") == [] and parse_targets("# only\n\ntrack t\n") == [] and parse_targets(b"chrM\t1\t2\n")[0][0] == "chrM"


@pytest.mark.parametrize("text,line,what", [("chr1\t5\n", 1, "fewer than 3 columns"), ("chr1\t1\t2\nchr1\tx\t9\n", 2, "malformed start 'x'"),
                                            ("#c\nchr1\t1\t2\nchr1\t3\t-4\n", 3, "malformed end '-4'"), ("chr1\t1.5\t9\n", 1, "malformed start"),
                                            ("chr1\t9\t3\n", 1, "start 9 > end 3"), ("chr1\t1\t4294967296\n", 1, "malformed end"),
                                            ("\r\nchr1\t1\t2\r\nchr1\t1\t\r\n", 3, "fewer than 3 columns")])
def test_parser_refuses_with_the_line_number(text, line, what):
    with pytest.raises(EngineError) as e:
        parse_targets(text)
    assert e.value.status == -1 and str(e.value).count(f"line {line}: ") == 1 and what in str(e.value), str(e.value)


def test_threshold_list():
    assert thresholds_parse(None) == [1, 10, 20, 30] and thresholds_parse("") == [1, 10, 20, 30]
    assert thresholds_parse("5") == [5] and thresholds_parse("1,2,3,4,5,6,7,4294967295") == [1, 2, 3, 4, 5, 6, 7, 4294967295]
    for bad, what in (("0,5", "first is 0"), ("5,5", "ascending"), ("9,3", "ascending"), ("1,,2", "not a whole number"), ("1,x", "not a whole number"),
                      ("1,2,", "not a whole number"), (",", "not a whole number"), ("1,2,3,4,5,6,7,8,9", "more than 8"), ("1,4294967296", "not a whole number"),
                      ("-1", "not a whole number"), ("1 ,2", "not a whole number")):
        with pytest.raises(EngineError) as e:
            thresholds_parse(bad)
        assert e.value.status == -1 and what in str(e.value), (bad, str(e.value))


# ---- the table ----
def _golden_input():
    thr = (1, 10, 30)
    a = dict(start=np.array([0, 100, 700], np.uint32), end=np.array([50, 400, 700], np.uint32), len=np.array([50, 300, 0], np.uint32),
             sum_raw=np.array([1234, 10**12 + 7, 0], np.uint64), sum_qc=np.array([999, 5 * 10**11, 0], np.uint64),
             state=np.array([[1, 40, 2, 3, 0, 4], [0, 299, 0, 0, 1, 0], [0] * 6], np.uint32),
             ge_raw=np.array([[48, 30, 1], [300, 300, 299], [0, 0, 0]], np.uint32), ge_qc=np.array([[45, 20, 0], [300, 290, 200], [0, 0, 0]], np.uint32))
    b = dict(start=np.array([4096], np.uint32), end=np.array([4099], np.uint32), len=np.array([3], np.uint32), sum_raw=np.array([1], np.uint64),
             sum_qc=np.array([0], np.uint64), state=np.array([[3, 0, 0, 0, 0, 0]], np.uint32), ge_raw=np.array([[1, 0, 0]], np.uint32),
             ge_qc=np.array([[0, 0, 0]], np.uint32))
    return thr, [("chr1", a, ["exon1", ".", "empty"]), ("chrY", b, ["P8"])]


def test_writer_against_golden_text(tmp_path):
    thr, contigs = _golden_input()
    golden = open(os.path.join(GOLDEN, "target_stats.tsv")).read()
    assert "\tNA\tNA\t0\tNA\t" in golden and golden.splitlines()[-1].startswith("total\t.\t.\t.\t353\t") and golden.startswith("#contig\tstart\tend\tname\tlength\t")
    assert targets_ref.table_text(contigs, thr) == golden
    path = str(tmp_path / "t.tsv")
    write_target_stats(path, [(n, TargetStats(thresholds=np.asarray(thr, np.uint32), **st), nm) for n, st, nm in contigs], thr)
    assert open(path).read() == golden
    # no threshold, no target: the header and a total of NA
    write_target_stats(path, [], ())
    lines = open(path).read().splitlines()
    assert len(lines) == 2 and lines[0].endswith("\tpoor_mapping_quality") and lines[1] == "total\t.\t.\t.\t0\tNA\tNA\t0\tNA\t0\t0\t0\t0\t0"


# ---- the tool: every argument error ends with status 2 before a device is opened ----
def test_cli_argument_errors(tmp_path):
    good = str(tmp_path / "good.bed")
    open(good, "w").write("chr1\t1\t2\n")
    bad = str(tmp_path / "bad.bed")
    open(bad, "w").write("chr1\t1\t2\nchr1\t7\t3\n")
    base = ["coverage", "no_such.bam", "-r", "no_such.fa"]
    for extra, what in ((["--target-out", "t.tsv"], "'--target-out' needs '--targets <BED>'"),
                        (["--target-thresholds", "1,5"], "'--target-thresholds' needs '--targets <BED>'"),
                        (["--targets", good], "'--targets' needs '--target-out <FILE>'"),
                        (["--targets", good, "--target-out", "t.tsv", "--target-thresholds", "1,x"], "invalid value '1,x' for '--target-thresholds'"),
                        (["--targets", good, "--target-out", "t.tsv", "--target-thresholds", "5,1"], "ascending"),
                        (["--targets", good, "--target-out", "t.tsv", "--target-thresholds", "0,1"], "first is 0"),
                        (["--targets", good, "--target-out", "t.tsv", "--target-thresholds", "1,2,3,4,5,6,7,8,9"], "more than 8"),
                        (["--targets", bad, "--target-out", "t.tsv"], "line 2: start 7 > end 3"),
                        (["--targets", str(tmp_path / "missing.bed"), "--target-out", "t.tsv"], "cannot read")):
        r = run(*(base + extra), cwd=str(tmp_path))
        assert r.returncode == 2 and what in r.stderr, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "t.tsv").exists()
    # well-formed flags get as far as the (missing) BAM: status 1, as without them
    r = run(*(base + ["--targets", good, "--target-out", "t.tsv"]), cwd=str(tmp_path))
    assert r.returncode == 1 and "Failed to collect BAM stats" in r.stderr
    assert "--targets BED --target-out FILE" in run("--help").stderr
