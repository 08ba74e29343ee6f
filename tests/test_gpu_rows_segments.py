"""The pass-bit rows with a stack per SEGMENT of 256 positions (-m gpu; pass_rows.h: rows_window_segments,
pileup_rows.hip.h: row_lane): lanes 8 s .. 8 s + 7 of a wave read the units of segment s and no others, as many as
that segment is high, from where the heights of the segments in front of it put them.

Every case is a contig of at most 4 windows (T = 2048), run as the upload lays it out and once more with
DUT_ROWS_UNIFORM=1 (every segment as high as the window's highest, the heights' word 0: the equal-heights decode), and
held against the oracle per position (raw, low, qc, state: the DEBUG instantiation of k_pileup_rows), as BED text, state
counts and sums (the production instantiation), and through k_depth_profile, k_depth_runs, k_target_depth and
k_target_order, which read the same rows."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import depth_ref
import order_ref
import runs_ref
import targets_ref
from helpers import make_options, oracle_run
from decodingustools_amd import CallableOptions, CallableProfiler, ContigProfiler, Engine, process_single_contig, synth
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu

T, S = 2048, 256
SUMS = ("n_covered_bases", "summed_coverage", "summed_baseq", "summed_mapq", "quality_bases", "n_reads")
EDGES = [1, 4, 10]
N_BINS, WINDOW = 1100, 500
THR = (1, 4, 10)


@pytest.fixture(autouse=True)
def pass_bit_form(monkeypatch):
    monkeypatch.delenv("DUT_QUAL_FORM", raising=False)


def _stack(p, n, cigar="100M", step=0):
    """n reads from position p on (each `step` behind the one before); every third below the base-quality threshold
    (a row of zeros), every seventh at mapq 0 (no row at all)"""
    return [(p + i * step, cigar, 0 if i % 7 == 6 else 60, 10 if i % 3 == 2 else 30) for i in range(n)]


def _case(name):
    """-> (reads as (pos, cigar, mapq, qual), contig length)"""
    L = 3 * T + 500
    if name in ("segment0", "segment7", "odd_segments"):
        # rows in the chosen segments of every window and nowhere else: the others have height 0, among them the first
        # and / or the last segment of the last window (which has no unit of its own behind it)
        segs = {"segment0": [0], "segment7": [7], "odd_segments": [1, 3, 5]}[name]
        L = 4 * T - 10
        reads = []
        for w in range(4):
            for s in segs:
                if w * T + s * S + 140 < L:
                    reads += _stack(w * T + s * S + 20, 5 + s + w, "100M", 2)
        return reads, L
    if name == "behind_an_empty_window":
        return _stack(300, 9, "120M", 5) + _stack(2 * T + 7 * S + 10, 6, "80M", 3), 3 * T
    if name == "seams":
        reads = [(S - 100, "100M", 60, 30), (S - 50, "100M", 60, 30), (S, "40M", 60, 30), (3 * S - 1, "2M", 60, 30),
                 (T - 150, "150M", 60, 30), (T - 70, "150M", 60, 30), (T, "30M", 60, 30), (T - 1, "1M", 60, 30),
                 (2 * T - 300, "600M", 60, 30), (2 * T + S - 64, "64M", 60, 30), (2 * T + S - 32, "64M", 60, 10)]
        return reads, L
    if name == "heights_4k_and_4k_plus_1":
        return [(2 * S + 10, "100M", 60, 30)] * 8 + [(3 * S + 10, "100M", 60, 30)] * 9 + \
               [(T + 5 * S + 10, "100M", 60, 30)] * 13 + [(T + 6 * S + 10, "100M", 60, 30)] * 12, 2 * T
    if name == "second_trip_for_some_lanes":
        # 60 rows (15 groups: groups 12 .. 14 are the second trip of the six-in-flight loop) in segment 3, one group elsewhere
        reads = [(T + 3 * S + 40 + i, "100M", 60, 30 if i % 4 else 10) for i in range(60)]
        for s in (0, 1, 5, 7):
            reads += _stack(T + s * S + 30, 3, "150M", 9)
        reads += _stack(100, 4, "150M", 30)
        return reads, 2 * T + 100
    if name in ("255_groups", "256_groups"):
        # 1020 rows on one stretch of segment 5: 255 units, the most a byte of the heights' word holds; 1021: the
        # equal-heights form.  Both beyond 63 groups: 16 counter planes.
        n = 1020 if name == "255_groups" else 1021
        reads = [(T + 5 * S + 20 + (i % 8), "64M", 60, 30) for i in range(n)]
        reads += _stack(T + 6 * S + 1, 5, "40M", 3) + _stack(50, 6, "150M", 40) + _stack(2 * T + 10, 3, "150M", 40)
        return reads, 2 * T + 300
    if name == "long_reads_with_gaps":
        reads = [(5 * S + 17, "500M300D400M1200N600M", 60, 30), (5 * S + 90, "700M20D30M", 60, 30),
                 (6 * S, "50M5000N50M", 60, 30),                   # a span far beyond its bases: walked per window
                 (T + 100, "20S300M2I400M100N300M", 60, 30), (T + 7 * S - 10, "30M", 0, 30)]
        reads += _stack(2 * T + 3 * S, 7, "200M50D100M", 11)
        return reads, 4 * T - 77
    if name == "short_reads":
        return None, 4 * T - 100
    raise KeyError(name)


CASES = ["segment0", "segment7", "odd_segments", "behind_an_empty_window", "seams", "heights_4k_and_4k_plus_1",
         "second_trip_for_some_lanes", "255_groups", "256_groups", "long_reads_with_gaps", "short_reads"]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    reads, L = _case(name)
    if reads is None:
        rec = synth.short_read_contig(L, 30, synth.seed_for(2, 41))
    else:
        reads = sorted(reads, key=lambda r: r[0])
        rec = ContigRecords.from_reads([(p, c, mq, q, 0, f"q{i}") for i, (p, c, mq, q) in enumerate(reads)])
    ref = synth.make_reference(L, 4243)
    opts = dict(max_depth=5000) if name.endswith("_groups") else {}
    with tempfile.TemporaryDirectory() as d:
        o_res, bed = oracle_run([("chrS", 0, L, ref, rec)], make_options(opts), os.path.join(d, "o.bed"), dump=True)
    return rec, ref, L, opts, o_res["chrS"], bed


def _engine_opts(d):
    o = make_options(d)
    return CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                           o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def run_case(name, uniform):
    """The case through the product path, everything compared with the oracle; returns the layout record."""
    rec, ref, L, opts, o, bed = _oracle(name)
    ro, qo, lo, so, eo = o["dumps"]
    saved = os.environ.get("DUT_ROWS_UNIFORM")
    try:
        os.environ.pop("DUT_ROWS_UNIFORM", None)
        if uniform:
            os.environ["DUT_ROWS_UNIFORM"] = "1"                   # (read when the engine is made)
        opt = _engine_opts(opts)
        with tempfile.TemporaryDirectory() as d, Engine(opt, 0) as eng:
            counter = CallableProfiler(os.path.join(d, "g.bed"))
            st = ContigProfiler("chrS", L)
            process_single_contig(eng, counter, st, opt, 0, rec, ref)
            counts = counter.get_contig_counts("chrS")
            counter.close()
            got_bed = open(os.path.join(d, "g.bed")).read()
            lay = eng.contig_layout()
            extent = int(eng.contig_collect().summary.extent)
            dumps = eng.debug_depths(extent)
            prof = eng.depth_profile(N_BINS, WINDOW)
            runs = {(kind, bool(e)): eng.depth_runs(kind, e) for kind in ("raw", "qc") for e in (None, EDGES)}
            eng.contig_collect()                                   # (the dump ran the contig again)
            tg_a, tg_b = targets_ref.window_edge_targets(extent, 1)
            tg = eng.target_stats(tg_a, tg_b, THR)
            tg_order = eng.target_order(tg_a, tg_b)
    finally:
        os.environ.pop("DUT_ROWS_UNIFORM", None)
        if saved is not None:
            os.environ["DUT_ROWS_UNIFORM"] = saved
    assert extent == max(eo, L)
    for what, want, got in zip(("raw", "qc", "low", "state"), (ro, qo, lo, so), dumps):
        bad = np.flatnonzero(want != got[:eo])
        assert bad.size == 0, (what, bad[:8].tolist(), want[bad[:8]].tolist(), got[bad[:8]].tolist())
    assert {k: getattr(st, k) for k in SUMS} == {k: o["stats"][k] for k in SUMS}
    assert counts == o["state_counts"]
    assert got_bed == bed
    depth = {"raw": depth_ref.pad(ro, extent), "qc": depth_ref.pad(qo, extent)}
    exp = depth_ref.profile(depth["raw"], depth["qc"], N_BINS, WINDOW)
    assert (prof.sum_raw, prof.sum_qc) == (exp["sum_raw"], exp["sum_qc"])
    for k in ("hist_raw", "hist_qc", "win_raw", "win_qc"):
        assert np.array_equal(getattr(prof, k), exp[k]), k
    for (kind, banded), r in runs.items():
        s, v = runs_ref.runs(depth[kind], EDGES if banded else None)
        assert r.n_runs == len(s), (kind, banded)
        assert np.array_equal(r.start, s) and np.array_equal(r.value, v), (kind, banded)
    assert tg.len.tolist() == [0, 12, 700, 150, 100]
    targets_ref.same(tg, targets_ref.target_stats(depth["raw"], depth["qc"], targets_ref.oracle_state(so, eo, dumps[3], extent), tg_a, tg_b, THR))
    assert tg_order.len.tolist() == [0, 12, 700, 150, 100]
    order_ref.same(tg_order, order_ref.target_order(depth["raw"], depth["qc"], tg_a, tg_b))
    return lay


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_case_against_the_oracle(name, uniform):
    lay = run_case(name, uniform)
    qc = _oracle(name)[4]["dumps"][1]
    assert qc.max() > 0
    if name.endswith("_groups"):
        assert lay["max_groups"] == (255 if name == "255_groups" else 256) and lay["counter_planes"] == 16
    elif name != "short_reads":
        assert lay["counter_planes"] == 8


@pytest.mark.parametrize("name", ["segment0", "segment7", "second_trip_for_some_lanes", "256_groups"])
def test_units_follow_the_heights(name):
    """What is resident: with rows in one segment per window the equal-heights form stores eight times the units; a
    window with a segment beyond 255 units is stored in that form either way."""
    a, b = run_case(name, False)["row_groups"], run_case(name, True)["row_groups"]
    if name in ("segment0", "segment7"):
        assert 0 < 8 * a == b
    elif name == "256_groups":
        # only the window of 256 groups is in the equal-heights form of itself; the other windows still differ
        assert 8 * 256 < a < b
    else:
        assert 0 < a < b


_ROW_CHUNK_CASE = r"""
import os, sys
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import test_gpu_rows_segments as M
for uniform in (False, True):
    assert M.run_case("short_reads", uniform)["row_groups"] > 0
    assert M.run_case("second_trip_for_some_lanes", uniform)["row_groups"] > 0
    assert M.run_case("odd_segments", uniform)["row_groups"] > 0
print("ROW_CHUNK_OK")
"""


@pytest.mark.parametrize("chunk", ["1", "3"])
def test_units_through_small_pinned_buffers(chunk):
    """DUT_ROW_CHUNK kilobytes (8 units) per pinned buffer: 1 -- every window of the short-read contig is larger than a
    buffer and travels as a block of its own; 3 -- 24 units: a few shallow windows per buffer and the buffer-full path with
    the window started over (odd_segments), oversized windows beside it.  (The knob is read once per process.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DUT_ROW_CHUNK=chunk)
    env.pop("DUT_ROWS_UNIFORM", None)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {root!r}\n" + _ROW_CHUNK_CASE], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ROW_CHUNK_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
