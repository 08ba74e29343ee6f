"""The depth path of k_pileup_rows (-m gpu): heads -> the +-1 scatter of raw_depth and low_mapq_count into difference
arrays -> prefix sums within a thread, a wave and across the waves -> the two per-position tests; and the two forms of a
head, 8 bytes or 4 (pileup_rows.hip.h: HEAD4), which the depth profile and the depth runs read too.

Every case is a contig of a few windows (T = 2048) in the pass-bit form, held against the oracle twice: per position
(raw, low, qc, state: Engine.debug_depths, the DEBUG instantiation of the kernel) and as BED text, state counts and
summary fields (the production instantiation)."""
import functools
import os
import tempfile

import numpy as np
import pytest

import depth_contigs
import depth_ref
import order_ref
import runs_ref
import targets_ref
from helpers import make_options, oracle_run
from decodingustools_amd import CallableOptions, CallableProfiler, ContigProfiler, Engine, process_single_contig, synth
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu

T = 2048
SUMS = ("n_covered_bases", "summed_coverage", "summed_baseq", "summed_mapq", "quality_bases", "n_reads")


@pytest.fixture(autouse=True)
def pass_bit_form(monkeypatch):
    monkeypatch.delenv("DUT_QUAL_FORM", raising=False)


def _engine_opts(d):
    o = make_options(d)
    return CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                           o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def check_against_oracle(reads, L, tmp_path, opt_dict=None, seed=77):
    """reads: (pos, cigar, mapq[, qual]) tuples in any order.  Returns the oracle's dumps (raw, qc, low, state, extent)
    and the engine's layout record."""
    reads = sorted(reads, key=lambda r: r[0])
    rec = ContigRecords.from_reads([(r[0], r[1], r[2], r[3] if len(r) > 3 else 30, 0, f"q{i}") for i, r in enumerate(reads)])
    ref = synth.make_reference(L, seed)
    o_res, o_bed = oracle_run([("chrT", 0, L, ref, rec)], make_options(opt_dict), str(tmp_path / "o.bed"), dump=True)
    ro, qo, lo, so, eo = o_res["chrT"]["dumps"]
    opt = _engine_opts(opt_dict)
    with Engine(opt, 0) as eng:
        counter = CallableProfiler(str(tmp_path / "g.bed"))
        st = ContigProfiler("chrT", L)
        process_single_contig(eng, counter, st, opt, 0, rec, ref)
        counts = counter.get_contig_counts("chrT")
        counter.close()
        lay = eng.contig_layout()
        extent = int(eng.contig_collect().summary.extent)
        rg, qg, lg, sg = eng.debug_depths(extent)
    assert extent == max(eo, L)
    for name, want, got in (("raw", ro, rg), ("low", lo, lg), ("qc", qo, qg), ("state", so, sg)):
        bad = np.flatnonzero(want != got[:eo])
        assert bad.size == 0, (name, bad[:8].tolist(), want[bad[:8]].tolist(), got[bad[:8]].tolist())
    for k in SUMS:
        assert getattr(st, k) == o_res["chrT"]["stats"][k], k
    assert counts == o_res["chrT"]["state_counts"]
    assert open(tmp_path / "g.bed").read() == o_bed
    return (ro, qo, lo, so, eo), lay


def test_ends_outnumber_starts_within_a_thread_and_across_the_waves(tmp_path):
    """About 300 mapq-0 reads start on the first 16 positions of window 1 (one thread's) and end 20 to 40 positions on:
    the two threads behind see only ends, so their sums of differences are negative for both counts (and whatever packs
    two counts or two positions into a word borrows across the fields there).  The same again from position 1010 of the window, so that the negative sums lie in the
    second wave (position 1024 on) and its offset from the first carries what they take away.  A few mapq-60 reads lie
    over both stretches, so that raw != low."""
    rng = np.random.default_rng(5)
    W = T
    reads = []
    for base in (0, 1010):
        for i in range(300):
            reads.append((W + base + int(rng.integers(0, 16)), f"{int(rng.integers(20, 41))}M", 0))
        for i in range(5):
            reads.append((W + base - 3 + 2 * i if base else W + 2 * i, "60M", 60))
    reads.append((100, "50M", 60))
    reads.append((2 * T + 10, "50M", 60))
    (raw, _, low, state, _), _ = check_against_oracle(reads, 2 * T + 300, tmp_path)
    assert raw[W + 15] >= 290 and low[W + 15] >= 285 and raw[W + 15] > low[W + 15]
    assert raw[W + 1025] >= 290 and raw[W + 1070] <= 5
    assert low[W + 56] == 0 and raw[W + 56] == 5


@pytest.mark.parametrize("n", [32767, 32768])
def test_the_most_candidates_a_16_bit_difference_takes(n, tmp_path):
    """A window with exactly 32 767 candidates, all mapq 0, all on one position: raw = low = 32 767, the largest count of
    the form without DEEP (16-bit difference fields).  One candidate more and the contig takes DEEP (32-bit difference
    words); both agree with the oracle."""
    p = 777                                                # (not position 0: the pileup's depth cap bites only there)
    reads = [(p, "2M", 0)] * n
    reads += [(T + 5, "40M", 60), (T + 20, "40M", 0), (2 * T - 40, "40M", 60)]
    (raw, _, low, state, _), _ = check_against_oracle(reads, 2 * T, tmp_path, dict(max_depth=100000))
    assert raw[p] == n and low[p] == n and raw[p + 2] == 0 and raw[p - 1] == 0
    assert state[p] in (0, 5) and state[p + 2] in (0, 2)  # POOR_MAPPING_QUALITY, NO_COVERAGE (REF_N where the reference has it)


def test_fast_and_general_path_in_one_window(tmp_path):
    """300 mapq-0 reads on 100 positions: the threads there see a raw depth of 255 or more and take the general path (the
    32-bit threshold table), while the window still has 8 counter planes (a mapq-0 read has no row).  The rest of the window is at
    depth 12 with one low read (1/12 <= 0.1: not poor) and with two (2/12 > 0.1: POOR_MAPPING_QUALITY): the byte table of
    the fast path, either side of its threshold at the default options."""
    W = T
    reads = [(W + 100, "100M", 0)] * 300
    reads += [(W + 300, "700M", 60)] * 11 + [(W + 300, "700M", 0)]
    reads += [(W + 1100, "700M", 60)] * 10 + [(W + 1100, "700M", 0)] * 2
    reads += [(50, "100M", 60)] * 5
    (raw, _, low, state, _), lay = check_against_oracle(reads, 2 * T + 100, tmp_path)
    assert lay["max_groups"] <= 63
    assert raw[W + 150] == 300 and low[W + 150] == 300
    assert raw[W + 500] == 12 and low[W + 500] == 1 and state[W + 500] == 1      # CALLABLE
    assert raw[W + 1500] == 12 and low[W + 1500] == 2 and state[W + 1500] == 5   # POOR_MAPPING_QUALITY


def test_window_edges(tmp_path):
    """Reads that start before the window, a read that ends exactly with it (no -1 is written), an extent that ends
    inside window 2 and inside a thread's 16 positions, and low reads that are clipped at both ends of window 1."""
    W = T
    L = 2 * T + 700 + 7
    reads = [(W - 30, "50M", 0), (W - 1, "2M", 60), (W - 7, "7M", 0), (W - 7, "8M", 0)]
    reads += [(2 * W - 40, "40M", 0), (2 * W - 40, "40M", 60), (2 * W - 1, "1M", 0), (2 * W - 1, "2M", 0)]
    reads += [(W - 500, "3000M", 0), (W - 1, f"{T + 2}M", 0), (W, f"{T}M", 0)]
    reads += [(L - 20, "20M", 0), (L - 33, "30M", 60), (2 * W + 100, "300M", 60)]
    (raw, _, low, state, eo), _ = check_against_oracle(reads, L, tmp_path, dict(min_depth=1, min_depth_for_low_mapq=2))
    assert eo == L
    assert raw[W] == 6 and low[W] == 5 and raw[W - 1] == 6
    assert raw[2 * W - 1] == 7 and low[2 * W - 1] == 6 and raw[2 * W] == 3
    assert raw[W + 1000] == 3 and low[W + 1000] == 3


# ---- 4-byte heads: pos & 0xFFFF | span << 16 | low << 31 where every head of a contig fits, 8-byte heads otherwise ----
H_L = 70 * T + 1234                                # 144 594 positions: past 65 536 and 131 072, the extent ends mid-window
H_B = 40 * T                                       # a window boundary; H_B - 16 383 = 65 537, just past the first wrap
H_EDGES = [1, 4, 10]
H_TARGET_WINDOW, H_THR = 32, (1, 4, 10)            # targets around position 65 536, where the planted reads meet a seam


def _h_records(which):
    base = synth.short_read_contig(H_L, 5, 4242)
    planted = [(65536 - 70, "150M", 60), (65536 - 1, "1M", 0), (65535, "2M", 0), (65536, "100M", 0),
               (131072 - 70, "150M", 0), (131072 - 149, "150M", 60), (131072, "100M", 60),
               # a span of exactly 16 384 (kWideSpan: the longest an ordinary read has) that reaches ONE position into window
               # 40: that window decodes the offset -16 383, the most negative the 16 bits of a 4-byte head are to give
               (H_B - 16383, "100M16184D100M", 60), (H_B - 16383, "100M16184D100M", 0)]
    if which == "wide":
        planted.append((3 * T + 5, "100M19800N100M", 60))          # a span of 20 000: one wide read, every head keeps 8 bytes
    planted.sort(key=lambda r: r[0])
    extra = ContigRecords.from_reads([(p, c, mq, 30, 0, f"p{i}") for i, (p, c, mq) in enumerate(planted)])
    return depth_contigs.merge(base, extra)


@functools.lru_cache(maxsize=None)
def _h_oracle(which):
    rec = _h_records(which)
    ref = synth.make_reference(H_L, 4243)
    with tempfile.TemporaryDirectory() as d:
        o_res, bed = oracle_run([("chrH", 0, H_L, ref, rec)], make_options({}), os.path.join(d, "o.bed"), dump=True)
    return rec, ref, o_res["chrH"], bed


@functools.lru_cache(maxsize=None)
def _h_engine(which, heads8, head_span=None):
    """the contig through the product path in one head form, and everything the tests look at while it is resident"""
    rec, ref, _, _ = _h_oracle(which)
    saved = {k: os.environ.get(k) for k in ("DUT_HEADS8", "DUT_HEAD_SPAN")}
    try:
        for k, v in (("DUT_HEADS8", "1" if heads8 else None), ("DUT_HEAD_SPAN", head_span)):
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        opt = _engine_opts({})
        with tempfile.TemporaryDirectory() as d, Engine(opt, 0) as eng:
            counter = CallableProfiler(os.path.join(d, "g.bed"))
            st = ContigProfiler("chrH", H_L)
            process_single_contig(eng, counter, st, opt, 0, rec, ref)
            out = dict(counts=counter.get_contig_counts("chrH"), sums={k: getattr(st, k) for k in SUMS})
            counter.close()
            out["bed"] = open(os.path.join(d, "g.bed")).read()
            out["layout"] = eng.contig_layout()
            out["bytes"] = eng.contig_bytes()
            extent = int(eng.contig_collect().summary.extent)
            out["extent"] = extent
            out["dumps"] = eng.debug_depths(extent)
            out["profile"] = eng.depth_profile(1001, 500)
            out["runs"] = {(kind, bool(e)): eng.depth_runs(kind, e) for kind in ("raw", "qc") for e in (None, H_EDGES)}
            eng.contig_collect()                                   # (the dump ran the contig again)
            out["targets"] = eng.target_stats(*targets_ref.window_edge_targets(extent, H_TARGET_WINDOW), H_THR)
            out["target_order"] = eng.target_order(*targets_ref.window_edge_targets(extent, H_TARGET_WINDOW))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


def _h_same_as_oracle(g, which):
    _, _, o, bed = _h_oracle(which)
    ro, qo, lo, so, eo = o["dumps"]
    assert g["extent"] == max(eo, H_L)
    for name, want, got in zip(("raw", "qc", "low", "state"), (ro, qo, lo, so), g["dumps"]):
        bad = np.flatnonzero(want != got[:eo])
        assert bad.size == 0, (name, bad[:8].tolist(), want[bad[:8]].tolist(), got[bad[:8]].tolist())
    assert g["sums"] == {k: o["stats"][k] for k in SUMS}
    assert g["counts"] == o["state_counts"]
    assert g["bed"] == bed


def _h_targets_same_as_oracle(g, which, what):
    """k_target_depth and k_target_order rebuild the depths with the code of the profile and the runs: the five targets
    around window H_TARGET_WINDOW against the references over the oracle's depths"""
    ro, qo, _, so, eo = _h_oracle(which)[2]["dumps"]
    raw, qc = depth_ref.pad(ro, g["extent"]), depth_ref.pad(qo, g["extent"])
    state = targets_ref.oracle_state(so, eo, g["dumps"][3], g["extent"])
    a, b = targets_ref.window_edge_targets(g["extent"], H_TARGET_WINDOW)
    assert g["targets"].len.tolist() == g["target_order"].len.tolist() == [0, 12, 700, 150, 100]
    targets_ref.same(g["targets"], targets_ref.target_stats(raw, qc, state, a, b, H_THR), what)
    order_ref.same(g["target_order"], order_ref.target_order(raw, qc, a, b), what)


def test_heads4_position_wrap_and_the_most_negative_offset():
    rec, _, o, _ = _h_oracle("short")
    raw = o["dumps"][0]
    assert int(depth_contigs.ref_spans(rec).max()) == depth_contigs.WIDE_SPAN
    assert raw[H_B] >= 2 and raw[65536] >= 3 and raw[131072] >= 3      # the planted reads are in the pileup
    g4, g8 = _h_engine("short", False), _h_engine("short", True)
    _h_same_as_oracle(g4, "short")
    _h_same_as_oracle(g8, "short")
    n_heads = g4["layout"]["n_records"]
    assert 0 < n_heads == g8["layout"]["n_records"] <= rec.n   # one head per read with a reference span
    assert g8["bytes"][0] - g4["bytes"][0] == 4 * n_heads
    assert g8["layout"]["upload_h2d_bytes"] - g4["layout"]["upload_h2d_bytes"] == 4 * (n_heads + 1)
    assert g8["bytes"][1] == g4["bytes"][1]


def test_heads_stay_8_bytes_with_a_wide_read_or_a_cut_span():
    wide, wide8 = _h_engine("wide", False), _h_engine("wide", True)
    _h_same_as_oracle(wide, "wide")
    assert wide["bytes"] == wide8["bytes"] and wide["layout"]["upload_h2d_bytes"] == wide8["layout"]["upload_h2d_bytes"]
    _h_targets_same_as_oracle(wide, "wide", "wide")
    _h_targets_same_as_oracle(wide8, "wide", "wide, DUT_HEADS8")
    cut, cut8 = _h_engine("short", False, 37), _h_engine("short", True, 37)
    _h_same_as_oracle(cut, "short")
    assert cut["layout"]["n_records"] > 2 * _h_engine("short", True)["layout"]["n_records"]   # spans cut into heads of 37 positions
    assert cut["bytes"] == cut8["bytes"] and cut["layout"]["upload_h2d_bytes"] == cut8["layout"]["upload_h2d_bytes"]
    # (and the 4-byte form of the same reads is smaller than either: it is the form, not the input, that differs)
    assert _h_engine("short", False)["bytes"][0] < _h_engine("short", True)["bytes"][0] < cut["bytes"][0]


@pytest.mark.parametrize("heads8", [False, True])
def test_depth_profile_and_depth_runs_in_both_head_forms(heads8):
    _, _, o, _ = _h_oracle("short")
    g = _h_engine("short", heads8)
    ro, qo, _, so, eo = o["dumps"]
    depth = {"raw": depth_ref.pad(ro, g["extent"]), "qc": depth_ref.pad(qo, g["extent"])}
    exp = depth_ref.profile(depth["raw"], depth["qc"], 1001, 500)
    got = g["profile"]
    assert (got.sum_raw, got.sum_qc) == (exp["sum_raw"], exp["sum_qc"])
    for k in ("hist_raw", "hist_qc", "win_raw", "win_qc"):
        assert np.array_equal(getattr(got, k), exp[k]), k
    for (kind, banded), r in g["runs"].items():
        s, v = runs_ref.runs(depth[kind], H_EDGES if banded else None)
        assert r.n_runs == len(s), (kind, banded)
        assert np.array_equal(r.start, s) and np.array_equal(r.value, v), (kind, banded)
    # k_target_depth rebuilds the depths with the same code: in this head form, and with the spans cut into heads of 37
    for gt in (g, _h_engine("short", heads8, 37)):
        state = targets_ref.oracle_state(so, eo, gt["dumps"][3], gt["extent"])
        a, b = targets_ref.window_edge_targets(gt["extent"], H_TARGET_WINDOW)
        assert gt["targets"].len.tolist() == [0, 12, 700, 150, 100]
        targets_ref.same(gt["targets"], targets_ref.target_stats(depth["raw"], depth["qc"], state, a, b, H_THR), (heads8, gt is g))
        _h_targets_same_as_oracle(gt, "short", (heads8, gt is g))
