"""The host layer of the depth profile (no device): dut_depth_stats, the accumulator and its three writers against
tests/depth_ref.py, the command line tool's argument errors, and the refusal of a host-only context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_ref
from decodingustools_amd import (CallableOptions, DepthAccumulator, DepthProfile, EngineError, _lib, build as _b,
                                 depth_stats)
from decodingustools_amd.callable_loci import HostStage


def same_stats(got, exp):
    assert got["positions"] == exp["positions"]
    assert got["mean"] == exp["mean"]                              # one f64 division on both sides
    for k in ("q1", "median", "q3"):
        assert got[k] == exp[k], (k, got[k], exp[k])
    assert got["frac_at_least"] == exp["frac_at_least"]


HAND = [
    ([0, 7], 7),                                   # all in the last bin: every quartile saturated
    ([9, 0], 0),                                   # a single bin
    ([0, 0, 5, 0], 10),
    ([1, 1, 1, 1, 0], 6),                          # even count: quartiles at 1, 2, 3 of 4
    ([1, 1, 1, 1, 1, 0], 10),                      # odd count: ceil(5/4) = 2, ceil(5/2) = 3, ceil(15/4) = 4
    ([2, 2, 2, 2, 0], 12),                         # boundaries that fall exactly on a bin's end
    ([0, 0, 0], 0),                                # no positions
    ([3] + [0] * 99 + [1], 100),                   # threshold 100 is the last bin itself: available
    ([3] + [0] * 98 + [1], 99),                    # ... and here it lies beyond: not available
    ([5, 4, 3, 2, 1] * 25, 1234),
]


@pytest.mark.parametrize("hist,total", HAND, ids=[str(i) for i in range(len(HAND))])
def test_depth_stats_on_hand_written_histograms(hist, total):
    same_stats(depth_stats(hist, total), depth_ref.stats(hist, total))


def test_depth_stats_values_spelled_out():
    s = depth_stats([1, 1, 1, 1, 1, 0], 10)
    assert s["positions"] == 5 and s["mean"] == 2.0
    assert (s["q1"], s["median"], s["q3"]) == ((1, False), (2, False), (3, False))
    assert s["frac_at_least"][1] == 0.8 and s["frac_at_least"][5] == 0.0 and s["frac_at_least"][10] is None
    s = depth_stats([0, 7], 700)
    assert s["median"] == (1, True) and s["mean"] == 100.0 and s["frac_at_least"][1] == 1.0 and s["frac_at_least"][5] is None
    s = depth_stats([0, 0, 0], 0)
    assert s["positions"] == 0 and s["mean"] == 0.0 and s["median"] == (0, False) and s["frac_at_least"][1] == 0.0
    with pytest.raises(EngineError):
        depth_stats([4], 0)


def test_depth_stats_on_random_histograms():
    rng = np.random.default_rng(11)
    for _ in range(200):
        n_bins = int(rng.integers(2, 300))
        hist = rng.integers(0, 1000, n_bins) * (rng.random(n_bins) < rng.random())
        total = int((hist * np.arange(n_bins)).sum()) + int(rng.integers(0, 50))
        same_stats(depth_stats(hist, total), depth_ref.stats(hist, total))
    big = np.array([2 ** 61, 2 ** 61, 2 ** 61 + 1], np.uint64)           # no overflow in the quartile targets
    same_stats(depth_stats(big, 3 * 2 ** 61), depth_ref.stats(big, 3 * 2 ** 61))


def _as_profile(p):
    return DepthProfile(n_bins=p["n_bins"], window=p["window"], n_windows=p["n_windows"], extent=p["extent"], sum_raw=p["sum_raw"],
                        sum_qc=p["sum_qc"], hist_raw=p["hist_raw"], hist_qc=p["hist_qc"], win_raw=p.get("win_raw"), win_qc=p.get("win_qc"))


def _random_contigs(seed, n_bins, window):
    rng = np.random.default_rng(seed)
    contigs = []
    for i, L in enumerate([5000, 1, 0, 2048, 777]):
        raw = rng.poisson(30 if i != 3 else 3, L).astype(np.uint64)
        if i == 4:
            raw[:] = 0                                              # an empty contig: everything in bin 0
        qc = raw - np.minimum(raw, rng.integers(0, 4, L).astype(np.uint64))
        contigs.append((f"chr{i + 1}", depth_ref.profile(raw, qc, n_bins, window)))
    return contigs


@pytest.mark.parametrize("n_bins,window", [(1001, 500), (17, 16), (2, 2049), (4096, 0)])
def test_accumulator_and_writers_byte_for_byte(n_bins, window, tmp_path):
    contigs = _random_contigs(n_bins, n_bins, window)
    wpath = str(tmp_path / "w.tsv") if window else None
    acc = DepthAccumulator(n_bins, window, wpath)
    for name, p in contigs:
        acc.add(name, _as_profile(p))
    hr, hq, sr, sq = acc.total()
    assert np.array_equal(hr, sum(p["hist_raw"] for _, p in contigs)) and np.array_equal(hq, sum(p["hist_qc"] for _, p in contigs))
    assert sr == sum(p["sum_raw"] for _, p in contigs) and sq == sum(p["sum_qc"] for _, p in contigs)
    acc.finish(str(tmp_path / "d.tsv"), str(tmp_path / "s.tsv"))
    acc.close()
    dist = open(tmp_path / "d.tsv").read()
    assert dist == depth_ref.dist_text(contigs)
    assert open(tmp_path / "s.tsv").read() == depth_ref.summary_text(contigs)
    if window:
        assert open(wpath).read() == depth_ref.windows_text(contigs)
    if n_bins == 17:                                               # the saturating bin and the total are there
        assert "\nchr1\traw\t16+\t" in dist and "\ntotal\tqc\t" in dist
    assert dist.splitlines()[0] == "#contig\tkind\tdepth\tpositions\tfraction_at_or_above"


def test_accumulator_refuses_what_the_engine_refuses(tmp_path):
    for n_bins, window in ((1, 0), (4097, 0), (100, 7), (100, 15)):
        with pytest.raises(EngineError):
            DepthAccumulator(n_bins, window)
    with pytest.raises(EngineError):
        DepthAccumulator(100, 500, str(tmp_path / "no" / "such" / "dir" / "w.tsv"))
    acc = DepthAccumulator(100, 0)
    with pytest.raises(EngineError):                                # a profile of another shape
        acc.add("c", _as_profile(depth_ref.profile(np.zeros(5), np.zeros(5), 101, 0)))


def run(*args, cwd=None):
    return subprocess.run([_b.CLI] + list(args), capture_output=True, text=True, cwd=cwd)


def test_cli_argument_errors_come_before_the_device(tmp_path):
    """as tests/test_cli.py::test_errors_before_the_device_is_needed: exit 2 and a message, no GPU on this path (the
    files do not even exist)"""
    _b.build()
    base = ("coverage", str(tmp_path / "missing.bam"), "-r", str(tmp_path / "missing.fa"))
    for extra, text in ((("--depth-windows", "w.tsv", "--window", "15"), "'--window'"),
                        (("--depth-windows", "w.tsv", "--window", "0"), "'--window'"),
                        (("--depth-windows", "w.tsv"), "needs '--window"),
                        (("--window", "500"), "needs '--depth-windows"),
                        (("--depth-dist", "d.tsv", "--depth-cap", "0"), "'--depth-cap'"),
                        (("--depth-dist", "d.tsv", "--depth-cap", "4096"), "'--depth-cap'"),
                        (("--depth-dist", "d.tsv", "--depth-cap", "x"), "invalid value 'x'"),
                        (("--depth-windows", "w.tsv", "--window", "-3"), "invalid value '-3'")):
        r = run(*base, *extra, cwd=str(tmp_path))
        assert r.returncode == 2 and text in r.stderr, (extra, r.returncode, r.stderr)
        assert not os.listdir(tmp_path)
    # well-formed depth flags: the run gets as far as the missing input, like one without them
    r = run(*base, "--depth-dist", "d.tsv", "--depth-windows", "w.tsv", "--window=16", "--depth-summary", "s.tsv", "--depth-cap", "4095",
            cwd=str(tmp_path))
    assert r.returncode == 1 and "Failed to collect BAM stats" in r.stderr
    r = run("--help")
    for flag in ("--depth-dist", "--depth-windows", "--window", "--depth-summary", "--depth-cap"):
        assert flag in r.stderr


def test_file_entry_checks_its_options_without_a_device(tmp_path):
    """dut_coverage_files_ex refuses a bad bin count or window before a file is opened (the inputs do not exist)"""
    lib = _lib.load()
    err = C.create_string_buffer(256)
    opt = CallableOptions().to_c()
    dv = (C.c_int * 1)(0)

    def call(depth):
        return lib.dut_coverage_files_ex(b"missing.bam", b"missing.fa", str(tmp_path / "o.bed").encode(), None, None, C.byref(opt), None, 0,
                                         dv, 1, 0, C.byref(depth) if depth is not None else None, err, 256)
    d = str(tmp_path / "d.tsv").encode()
    w = str(tmp_path / "w.tsv").encode()
    for o in (_lib.dut_depth_options(1, 0, d, None, None), _lib.dut_depth_options(4097, 0, d, None, None),
              _lib.dut_depth_options(100, 15, None, w, None), _lib.dut_depth_options(100, 0, None, w, None)):
        assert call(o) == -1 and b"depth profile" in err.value and not os.listdir(tmp_path)
    # well-formed, or nothing asked: the run gets as far as the missing input
    for o in (_lib.dut_depth_options(1001, 500, d, w, None), _lib.dut_depth_options(0, 0, None, None, None), None):
        assert call(o) == -1 and b"Failed to collect BAM stats" in err.value


def test_host_only_context_has_no_depth_profile():
    hs = HostStage(CallableOptions())
    with pytest.raises(EngineError) as e:
        hs.depth_profile(1001, 500)
    assert e.value.status == -2                                    # CL_ERR_DEVICE
    hs.close()


def test_symbols_and_struct_layouts():
    lib = _lib.load()
    for name in ("cl_contig_depth_profile", "dut_depth_stats", "dut_depth_acc_new", "dut_depth_acc_add", "dut_depth_acc_total",
                 "dut_depth_acc_finish", "dut_depth_acc_free", "cl_contig_depth_profile_ms", "dut_coverage_files_ex"):
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.cl_depth_profile) == 8 + 4 * 8 + 4 * 8
    assert C.sizeof(_lib.dut_depth_summary) == 8 + 8 + 12 + 4 + 8 * 8
    assert C.sizeof(_lib.dut_depth_options) == 8 + 3 * 8
    th = (C.c_uint32 * 8).in_dll(lib, "dut_depth_thresholds")
    assert tuple(th) == depth_ref.THRESHOLDS == _lib.DEPTH_THRESHOLDS
    assert lib.cl_abi_version() == 1
