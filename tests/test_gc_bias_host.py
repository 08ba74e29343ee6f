"""The host layer of the GC-bias profile (no device): the reference's two bit planes (cl_debug_gc_bits) against numpy,
dut_gc_bias_add, dut_gc_bias_stats and the two writers against tests/gc_ref.py, the command line tool's argument errors,
and the refusal of a host-only context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gc_ref
from decodingustools_amd import (CallableOptions, EngineError, GcBias, _lib, build as _b, gc_bias_stats, write_gc_bias,
                                 write_gc_summary)
from decodingustools_amd.bam import coverage_files
from decodingustools_amd.callable_loci import HostStage

LEVELS = (0, 1, 2)                                 # scalar, SSE2, AVX2 where the CPU has it (else SSE2)


def gc_bits(ref, n_words, level):
    ref = np.ascontiguousarray(ref, np.uint8)
    gc = np.full(max(n_words, 1), 0xAAAAAAAAAAAAAAAA, np.uint64)
    va = np.full(max(n_words, 1), 0x5555555555555555, np.uint64)
    st = _lib.load().cl_debug_gc_bits(ref.ctypes.data if ref.size else None, ref.size, n_words, level, gc.ctypes.data, va.ctypes.data)
    assert st == 0
    return gc[:n_words], va[:n_words]


@pytest.mark.parametrize("level", LEVELS)
def test_gc_bits_of_all_256_byte_values(level):
    ref = np.arange(256, dtype=np.uint8)
    gc, va = gc_bits(ref, 4, level)
    e_gc, e_va = gc_ref.bit_words(ref, 4)
    assert np.array_equal(gc, e_gc) and np.array_equal(va, e_va)
    # the classes themselves, spelt out: 4 GC bytes, 8 valid ones, S and N and the rest invalid
    bits = lambda w: {64 * i + j for i, x in enumerate(w) for j in range(64) if (int(x) >> j) & 1}   # noqa: E731
    assert bits(gc) == set(b"GCgc") and bits(va) == set(b"ACGTacgt")


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 63, 64, 65, 127, 129, 4099])
def test_gc_bits_lengths_and_words_beyond_the_reference(n, level):
    rng = np.random.default_rng(n)
    ref = rng.choice(np.frombuffer(b"ACGTacgtNnSRYKMWxz*-", np.uint8), n)
    for extra in (0, 1, 3):                                       # words beyond the reference: all invalid
        n_words = -(-n // 64) + extra
        gc, va = gc_bits(ref, n_words, level)
        e_gc, e_va = gc_ref.bit_words(ref, n_words)
        assert np.array_equal(gc, e_gc) and np.array_equal(va, e_va), (n, extra)
        assert not gc[-(-n // 64):].any() and not va[-(-n // 64):].any()
    if n > 64:                                                    # fewer words than the bases fill: nothing behind them is written
        gc, va = gc_bits(ref, 1, level)
        e_gc, e_va = gc_ref.bit_words(ref[:64], 1)
        assert np.array_equal(gc, e_gc) and np.array_equal(va, e_va)
    assert _lib.load().cl_debug_gc_bits(None, 5, 1, level, None, None) == -1
    assert _lib.load().cl_debug_gc_bits(None, 0, 0, 3, None, None) == -1


def record(positions, sum_raw, sum_qc, zero_raw, window=100, max_invalid=4, extent=None, n_skipped=0):
    pad = lambda d: np.asarray([int(dict(d).get(b, 0)) for b in range(gc_ref.BINS)], np.uint64)   # noqa: E731
    pos = pad(positions)
    return GcBias(window=window, max_invalid=max_invalid, extent=int(pos.sum()) + n_skipped if extent is None else extent,
                  n_skipped=n_skipped, positions=pos, sum_raw=pad(sum_raw), sum_qc=pad(sum_qc), zero_raw=pad(zero_raw))


def _random_record(seed):
    rng = np.random.default_rng(seed)
    bins = rng.choice(gc_ref.BINS, 30, replace=False)
    pos = {int(b): int(rng.integers(1, 10 ** 7)) for b in bins}
    raw = {b: int(n * rng.uniform(0, 60)) for b, n in pos.items()}
    qc = {b: int(r * rng.uniform(0.3, 1.0)) for b, r in raw.items()}
    zero = {b: int(n * rng.uniform(0, 0.2)) for b, n in pos.items()}
    return record(pos, raw, qc, zero, n_skipped=int(rng.integers(0, 1000)))


CASES = {
    "empty": record({}, {}, {}, {}),
    "skipped_only": record({}, {}, {}, {}, n_skipped=77),
    "single_bin": record({41: 1000}, {41: 30500}, {41: 28111}, {41: 3}),
    "no_raw_depth": record({10: 5, 60: 7}, {}, {}, {10: 5, 60: 7}),                 # S_raw == S_qc == 0
    "no_qc_depth": record({10: 5, 60: 7}, {10: 50, 60: 71}, {}, {}),               # S_qc == 0 alone
    "at_only": record({0: 10, 17: 400, 50: 33}, {0: 1, 17: 9000, 50: 700}, {0: 0, 17: 8000, 50: 650}, {0: 9, 17: 2}),
    "gc_only": record({51: 10, 77: 400, 100: 33}, {51: 100, 77: 9000, 100: 70}, {51: 90, 77: 8000, 100: 65}, {100: 20}),
    "both_sides": record({20: 1000, 45: 5000, 55: 4000, 80: 500}, {20: 12000, 45: 160000, 55: 120000, 80: 3000},
                         {20: 10000, 45: 150000, 55: 110000, 80: 2000}, {20: 100, 80: 200}, window=1024, max_invalid=0),
    "large_counts": record({33: 2 ** 40 + 7, 66: 2 ** 41 + 1}, {33: 2 ** 45 + 3, 66: 2 ** 46 + 11}, {33: 2 ** 44, 66: 2 ** 45 + 5}, {33: 1, 66: 2 ** 30}),
    "random_1": _random_record(1),
    "random_2": _random_record(2),
}


def same_stats(got, exp):
    for k in ("positions", "sum_raw", "sum_qc"):
        assert got[k] == exp[k], k
    # the same f64 operations in the same order on both sides: equal, not close
    for k in ("total_mean_raw", "total_mean_qc", "at_dropout_raw", "gc_dropout_raw", "at_dropout_qc", "gc_dropout_qc"):
        assert got[k] == exp[k], (k, got[k], exp[k])
    for k in ("mean_raw", "mean_qc", "norm_raw", "norm_qc", "zero_frac"):
        for b in range(gc_ref.BINS):
            g, e = got[k][b], exp[k][b]
            assert (e is None and np.isnan(g)) or g == e, (k, b, g, e)


@pytest.mark.parametrize("name", list(CASES))
def test_stats_against_the_restatement(name):
    g = CASES[name]
    got, exp = gc_bias_stats(g), gc_ref.stats(g)
    same_stats(got, exp)
    if name in ("empty", "skipped_only"):
        assert got["total_mean_raw"] is None and got["at_dropout_raw"] is None and np.isnan(got["mean_raw"]).all()
    if name == "no_raw_depth":
        assert got["total_mean_raw"] == 0.0 and got["at_dropout_raw"] is None and np.isnan(got["norm_raw"][10]) and got["zero_frac"][10] == 1.0
    if name == "no_qc_depth":
        assert got["at_dropout_raw"] is not None and got["at_dropout_qc"] is None and got["gc_dropout_qc"] is None
    if name == "at_only":
        assert got["gc_dropout_raw"] == 0.0 and got["at_dropout_raw"] > 0.0
    if name == "gc_only":
        assert got["at_dropout_raw"] == 0.0 and got["gc_dropout_raw"] > 0.0
    if name == "single_bin":
        assert got["norm_raw"][41] == 1.0 and got["at_dropout_raw"] == 0.0 and got["gc_dropout_raw"] == 0.0


def test_add_sums_the_bins_and_refuses_other_windows():
    a, b, c = CASES["at_only"], CASES["gc_only"], CASES["random_1"]
    t = GcBias.empty() + a + b + c
    gc_ref.same(t, gc_ref.add(gc_ref.add(gc_ref.add(None, a), b), c), "sum")
    assert (t.window, t.max_invalid) == (100, 4) and t.extent == a.extent + b.extent + c.extent
    gc_ref.same(a + b, b.add(a), "commutes")
    big = record({5: 1}, {}, {}, {}, extent=0xFFFFFFF0)
    assert (big + big).extent == 0xFFFFFFFF                         # saturates
    with pytest.raises(EngineError):
        a + CASES["both_sides"]                                     # window 1024 / max_invalid 0
    with pytest.raises(EngineError):
        a + record({1: 1}, {}, {}, {}, max_invalid=5)
    before = a.tobytes()
    with pytest.raises(EngineError):
        a.add(record({1: 1}, {}, {}, {}, window=99))
    assert a.tobytes() == before


@pytest.mark.parametrize("total", [True, False])
def test_writers_against_the_restatement(tmp_path, total):
    contigs = [(name, CASES[name]) for name in ("single_bin", "empty", "at_only", "gc_only", "no_raw_depth", "no_qc_depth", "random_1", "large_counts")]
    for wr, text, tol, fn in ((write_gc_bias, gc_ref.bias_text, gc_ref.BIAS_TOL, "b.tsv"), (write_gc_summary, gc_ref.summary_text, gc_ref.SUMMARY_TOL, "s.tsv")):
        p = str(tmp_path / fn)
        wr(p, contigs, total=total)
        got, exp = open(p).read(), text(contigs, total=total)
        gc_ref.same_text(got, exp, tol, fn)
        assert ("\ntotal\t" in got) == total
        assert "\tNA" in got
    # one record of another window: the total cannot be formed
    with pytest.raises(EngineError):
        write_gc_bias(str(tmp_path / "x.tsv"), [("a", CASES["at_only"]), ("b", CASES["both_sides"])])
    lines = open(tmp_path / "b.tsv").read().split("\n")
    assert lines[0].split("\t") == "#contig gc positions mean_raw mean_qc norm_raw norm_qc zero_frac".split()
    assert lines[1] == "single_bin\t41\t1000\t30.5000\t28.1110\t1.000000\t1.000000\t0.003000"
    s = open(tmp_path / "s.tsv").read().split("\n")
    assert s[0].split("\t") == ("#contig window max_invalid positions skipped mean_raw mean_qc at_dropout_raw gc_dropout_raw "
                                "at_dropout_qc gc_dropout_qc").split()
    assert s[2] == "empty\t100\t4\t0\t0\tNA\tNA\tNA\tNA\tNA\tNA"


def test_same_text_holds_its_tolerances():
    h = gc_ref.BIAS_HEADER
    gc_ref.same_text(h + "c\t1\t2\t1.0001\t1.0000\t0.000001\tNA\t0.500000\n", h + "c\t1\t2\t1.0000\t1.0001\t0.000002\tNA\t0.500001\n", gc_ref.BIAS_TOL)
    for bad in ("c\t1\t2\t1.0002\t1.0000\t0.000001\tNA\t0.500000\n", "c\t1\t3\t1.0000\t1.0000\t0.000001\tNA\t0.500000\n",
                "c\t1\t2\t1.0000\t1.0000\t0.000003\tNA\t0.500000\n", "c\t1\t2\t1.0000\t1.0000\t0.000001\t0.000000\t0.500000\n"):
        with pytest.raises(AssertionError):
            gc_ref.same_text(h + bad, h + "c\t1\t2\t1.0000\t1.0000\t0.000001\tNA\t0.500000\n", gc_ref.BIAS_TOL)


def run(*args, cwd=None):
    return subprocess.run([_b.CLI] + list(args), capture_output=True, text=True, cwd=cwd)


def test_cli_argument_errors_come_before_the_device(tmp_path):
    """exit 2 and a message, no GPU on this path (the files do not even exist)"""
    _b.build()
    base = ("coverage", str(tmp_path / "missing.bam"), "-r", str(tmp_path / "missing.fa"))
    for extra, text in ((("--gc-window", "50"), "'--gc-window' needs '--gc-bias"),
                        (("--gc-max-n", "2"), "'--gc-max-n' needs '--gc-bias"),
                        (("--gc-bias", "b.tsv", "--gc-window", "0"), "'--gc-window': 1..1024"),
                        (("--gc-summary", "s.tsv", "--gc-window", "1025"), "'--gc-window': 1..1024"),
                        (("--gc-bias", "b.tsv", "--gc-window", "4"), "'--gc-max-n'"),          # the default K = 4 is not below 4
                        (("--gc-bias", "b.tsv", "--gc-max-n", "100"), "'--gc-max-n'"),
                        (("--gc-bias", "b.tsv", "--gc-window=10", "--gc-max-n=10"), "'--gc-max-n'"),
                        (("--gc-bias", "b.tsv", "--gc-window", "x"), "invalid value 'x' for '--gc-window'"),
                        (("--gc-summary", "s.tsv", "--gc-max-n", "-1"), "invalid value '-1' for '--gc-max-n'"),
                        (("--gc-summary", "s.tsv", "--gc-max-n", "3k"), "invalid value '3k' for '--gc-max-n'")):
        r = run(*base, *extra, cwd=str(tmp_path))
        assert r.returncode == 2 and text in r.stderr, (extra, r.returncode, r.stderr)
        assert not os.listdir(tmp_path)
    # well-formed GC flags, alone and with the other families: the run gets as far as the missing input
    for extra in (("--gc-bias", "b.tsv", "--gc-summary", "s.tsv", "--gc-window", "1024", "--gc-max-n", "1023"),
                  ("--gc-bias", "b.tsv", "--gc-window", "1", "--gc-max-n", "0", "--depth-dist", "d.tsv", "--depth-bed", "p.bed")):
        r = run(*base, *extra, cwd=str(tmp_path))
        assert r.returncode == 1 and "missing.bam" in r.stderr, (extra, r.returncode, r.stderr)


def test_library_argument_errors_come_before_any_file(tmp_path):
    bam, fa = str(tmp_path / "missing.bam"), str(tmp_path / "missing.fa")
    for kw, text in ((dict(gc_window=50), "need gc_bias"), (dict(gc_bias="b.tsv", gc_window=0), "gc_window"),
                     (dict(gc_summary="s.tsv", gc_window=1025), "gc_window"), (dict(gc_bias="b.tsv", gc_max_invalid=100), "gc_max_invalid"),
                     (dict(gc_bias="b.tsv", gc_window=3), "gc_max_invalid")):
        with pytest.raises(EngineError) as e:
            coverage_files(bam, fa, str(tmp_path / "g.bed"), None, CallableOptions(), **kw)
        assert text in str(e.value)
    # the library's own check (dut_coverage_files_ex5), reached without the Python layer's
    lib = _lib.load()
    err = C.create_string_buffer(512)
    oc = CallableOptions().to_c()
    dv = (C.c_int * 1)(0)
    for w, k, text in ((0, 0, "window"), (1025, 4, "window"), (100, 100, "invalid bases")):
        go = _lib.dut_gc_options(str(tmp_path / "b.tsv").encode(), None, w, k)
        st = lib.dut_coverage_files_ex5(bam.encode(), fa.encode(), str(tmp_path / "g.bed").encode(), None, None, C.byref(oc), None, 0, dv, 1, 0,
                                        None, None, None, 0, C.byref(go), err, 512)
        assert st == -1 and text in err.value.decode(), (w, k, err.value)
    assert not os.listdir(tmp_path)


def test_a_host_only_context_has_no_device():
    with HostStage(CallableOptions()) as h:
        h.contig_begin(0, 100, np.frombuffer(b"ACGT" * 25, np.uint8))
        with pytest.raises(EngineError) as e:
            h.gc_bias(b"ACGT" * 25)
        assert e.value.status == -2 and "host-only" in str(e.value)
