"""The host side of the per-target order statistics, no device: tests/order_ref.py against a per-position loop, the table
writers with and without the ten columns, the tool's argument error, and the piece list (target_pieces.h) in a stand-alone
program under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import order_ref
import targets_ref
from decodingustools_amd import EngineError, TargetOrder, TargetStats, build as _b, write_target_stats
from decodingustools_amd.bam import coverage_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- the reference rule itself ----
@pytest.mark.parametrize("seed", range(8))
def test_reference_against_the_per_position_loop(seed):
    rng = np.random.default_rng(seed)
    extent = [0, 1, 2, 5, 7, 40, 64, 100][seed]
    raw = rng.integers(0, 40, extent) if seed != 6 else np.full(extent, 17)      # (all depths equal)
    qc = np.minimum(raw, rng.integers(0, 40, extent))
    starts = np.concatenate((rng.integers(0, extent + 10, 60), np.zeros(6, np.int64)))
    ends = np.concatenate((starts[:60] + np.where(rng.random(60) < 0.3, 0, rng.integers(0, extent + 10, 60)), np.arange(6)))   # len 0 .. 5 too
    a = order_ref.target_order(raw, qc, starts, ends)
    b = order_ref.target_order_loop(raw, qc, starts, ends)
    order_ref.same(a, b, seed)
    assert (a["raw"][:, :-1] <= a["raw"][:, 1:]).all() and (a["qc"][:, :-1] <= a["qc"][:, 1:]).all() and (a["qc"] <= a["raw"]).all()
    assert not a["raw"][a["len"] == 0].any() and not a["qc"][a["len"] == 0].any()


def test_reference_lengths_one_to_five_and_the_lower_median():
    raw = np.array([9, 3, 7, 1, 5, 5, 5]); qc = raw // 2
    o = order_ref.target_order(raw, qc, [0, 0, 0, 0, 0, 0, 4, 6, 9], [0, 1, 2, 3, 4, 5, 7, 20, 12])
    assert o["len"].tolist() == [0, 1, 2, 3, 4, 5, 3, 1, 0] and o["end"].tolist() == [0, 1, 2, 3, 4, 5, 7, 7, 7]
    # min, q1, median, q3, max: element (j * len + 3) // 4 - 1 of the sorted depths
    assert o["raw"].tolist() == [[0] * 5, [9] * 5, [3, 3, 3, 9, 9], [3, 3, 7, 9, 9], [1, 1, 3, 7, 9], [1, 3, 5, 7, 9], [5] * 5, [5] * 5, [0] * 5]
    assert o["qc"][4].tolist() == [0, 0, 1, 3, 4]
    assert order_ref.ranks(4) == [0, 0, 1, 2, 3] and order_ref.ranks(8) == [0, 1, 3, 5, 7] and order_ref.ranks(1) == [0] * 5


# ---- the table ----
def _input():
    thr = (1, 10, 30)
    a = dict(start=np.array([0, 100, 700], np.uint32), end=np.array([50, 400, 700], np.uint32), len=np.array([50, 300, 0], np.uint32),
             sum_raw=np.array([1234, 10**12 + 7, 0], np.uint64), sum_qc=np.array([999, 5 * 10**11, 0], np.uint64),
             state=np.array([[1, 40, 2, 3, 0, 4], [0, 299, 0, 0, 1, 0], [0] * 6], np.uint32),
             ge_raw=np.array([[48, 30, 1], [300, 300, 299], [0, 0, 0]], np.uint32), ge_qc=np.array([[45, 20, 0], [300, 290, 200], [0, 0, 0]], np.uint32))
    b = dict(start=np.array([4096], np.uint32), end=np.array([4099], np.uint32), len=np.array([3], np.uint32), sum_raw=np.array([1], np.uint64),
             sum_qc=np.array([0], np.uint64), state=np.array([[3, 0, 0, 0, 0, 0]], np.uint32), ge_raw=np.array([[1, 0, 0]], np.uint32),
             ge_qc=np.array([[0, 0, 0]], np.uint32))
    oa = dict(start=a["start"], end=a["end"], len=a["len"], raw=np.array([[0, 9, 24, 31, 33], [29, 3 * 10**9, 4 * 10**9, 4294967295, 4294967295], [0] * 5], np.uint32),
              qc=np.array([[0, 7, 20, 22, 29], [9, 10, 11, 12, 4294967295], [0] * 5], np.uint32))
    ob = dict(start=b["start"], end=b["end"], len=b["len"], raw=np.array([[0, 0, 0, 1, 1]], np.uint32), qc=np.zeros((1, 5), np.uint32))
    return thr, [("chr1", a, ["exon1", ".", "empty"], oa), ("chrY", b, ["P8"], ob)]


def test_writers_with_the_order_columns_and_without(tmp_path):
    thr, contigs = _input()
    stats = [(n, TargetStats(thresholds=np.asarray(thr, np.uint32), **st), nm) for n, st, nm, _ in contigs]
    order = [TargetOrder(**od) for _, _, _, od in contigs]
    want = order_ref.table_text(contigs, thr)
    lines = want.splitlines()
    assert lines[0].endswith("\tqc_ge_30\traw_min\traw_q1\traw_median\traw_q3\traw_max\tqc_min\tqc_q1\tqc_median\tqc_q3\tqc_max")
    assert lines[1].endswith("\t0\t9\t24\t31\t33\t0\t7\t20\t22\t29") and lines[2].endswith("\t29\t3000000000\t4000000000\t4294967295\t4294967295\t9\t10\t11\t12\t4294967295")
    assert lines[3].endswith("\t0\t0\t0" + "\tNA" * 10) and lines[-1].startswith("total\t.\t.\t.\t353\t") and lines[-1].endswith("\tNA" * 10)
    path = str(tmp_path / "t.tsv")
    write_target_stats(path, stats, thr, order=order)
    assert open(path).read() == want
    # without the records: the existing text, byte for byte
    golden = open(os.path.join(GOLDEN, "target_stats.tsv")).read()
    write_target_stats(path, stats, thr)
    assert open(path).read() == golden == targets_ref.table_text([c[:3] for c in contigs], thr)
    write_target_stats(path, stats, thr, order=None)
    assert open(path).read() == golden
    # every line of the wider table starts with its line of the narrower one
    assert all(w.startswith(g + "\t") for w, g in zip(lines, golden.splitlines()))
    # no threshold, no target: the header and a total of NA
    write_target_stats(path, [], (), order=[])
    got = open(path).read().splitlines()
    assert len(got) == 2 and got[0].endswith("\tpoor_mapping_quality\traw_min\traw_q1\traw_median\traw_q3\traw_max\tqc_min\tqc_q1\tqc_median\tqc_q3\tqc_max")
    assert got[1] == "total\t.\t.\t.\t0\tNA\tNA\t0\tNA\t0\t0\t0\t0\t0" + "\tNA" * 10
    # records of other targets, or too few of them, are refused
    other = TargetOrder(**{**contigs[1][3], "start": np.array([4095], np.uint32)})
    for bad in ([order[0], other], [order[0]], [order[0], order[0]]):
        with pytest.raises(EngineError):
            write_target_stats(path, stats, thr, order=bad)


# ---- the tool and the file-level call: the flag without targets ends before a device is opened ----
def test_target_quantiles_needs_targets(tmp_path):
    base = ["coverage", "no_such.bam", "-r", "no_such.fa"]
    r = subprocess.run([_b.CLI] + base + ["--target-quantiles"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2 and "'--target-quantiles' needs '--targets <BED>'" in r.stderr, (r.returncode, r.stderr)
    good = str(tmp_path / "good.bed")
    open(good, "w").write("chr1\t1\t2\n")
    # with targets the flag gets as far as the (missing) BAM: status 1, as without it
    r = subprocess.run([_b.CLI] + base + ["--targets", good, "--target-out", "t.tsv", "--target-quantiles"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "Failed to collect BAM stats" in r.stderr
    assert "--target-quantiles" in subprocess.run([_b.CLI, "--help"], capture_output=True, text=True).stderr
    with pytest.raises(EngineError) as e:
        coverage_files("no_such.bam", "no_such.fa", str(tmp_path / "g.bed"), target_quantiles=True)
    assert "target_quantiles needs targets" in str(e.value)
    # the library's own refusal (dut_coverage_files_ex4), before the BAM is looked at
    import ctypes as C
    from decodingustools_amd import _lib
    lib = _lib.load()
    err = C.create_string_buffer(512)
    oc = _lib.cl_options()
    dev = (C.c_int * 1)(0)
    for targets, flags, what in ((None, 1, "need a BED of regions"), (_lib.dut_target_options(None, b"t.tsv", None, 0), 1, "need a BED of regions"),
                                 (_lib.dut_target_options(good.encode(), b"t.tsv", None, 0), 2, "unknown target flags")):
        st = lib.dut_coverage_files_ex4(b"no_such.bam", b"no_such.fa", b"g.bed", None, None, C.byref(oc), None, 0, dev, 1, 0, None, None,
                                        C.byref(targets) if targets is not None else None, flags, err, 512)
        assert st == -1 and what in err.value.decode(), err.value


def test_host_only_context_and_the_abi():
    import ctypes as C
    from decodingustools_amd import CallableOptions, _lib
    from decodingustools_amd.callable_loci import HostStage, TARGET_ORDER
    hs = HostStage(CallableOptions())
    with pytest.raises(EngineError) as e:
        hs.target_order([0], [10])
    assert e.value.status == -2                                # CL_ERR_DEVICE
    hs.close()
    lib = _lib.load()
    for name in ("cl_contig_target_order", "cl_contig_target_order_ms", "dut_targets_write_header_ex", "dut_targets_write_ex",
                 "dut_targets_write_total_ex", "dut_coverage_files_ex4", "dut_coverage_files_ex3", "cl_contig_targets"):
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.cl_target_order) == 52 == TARGET_ORDER.itemsize
    assert _lib.CL_TARGET_ORDER_MAX_PIECES == 1 << 26 and _lib.DUT_TARGETS_ORDER == 1 and lib.cl_abi_version() == 1


# ---- the piece list under the sanitizers ----
def test_piece_list_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "target_pieces_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "target_pieces_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if any(m in r.stderr for m in ("cannot find -lasan", "cannot find -lubsan", "unrecognized command-line option", "unrecognized argument")):
            pytest.skip("sanitizer runtimes not installed here: " + r.stderr[-300:])
        pytest.fail("the sanitizer build failed:\n" + r.stderr[-3000:])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0"))
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 80, r.stdout
