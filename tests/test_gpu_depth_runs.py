"""The depth runs on the device (-m gpu): cl_contig_depth_runs against tests/runs_ref.py applied to the CPU oracle's
per-position raw_depth / qc_depth, and to the engine's own cl_debug_depths.  Everything is exact."""
import json
import os
import subprocess
import time

import numpy as np
import pytest

import depth_contigs
import depth_ref
import runs_ref
import sparse_ref
from bamio import write_bam, write_fasta
from helpers import contig_inputs, load_kats, make_options, oracle_run
from decodingustools_amd import (CallableOptions, CallableProfiler, ContigProfiler, Engine, EngineError, build as _b,
                                 process_single_contig, synth)
from decodingustools_amd.bam import coverage_files
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu
KATS = load_kats()
E64 = list(range(1, 49)) + [50, 64, 100, 128, 200, 255, 256, 257, 500, 1000, 4096, 65535, 65536, 70000, 10 ** 6, 2 ** 32 - 1]
EDGE_SETS = (None, [1], [1, 4, 100], [2, 3, 5, 17, 255, 256, 70000], E64)
AROUND_THE_PLANES = [254, 255, 256, 257, 65534, 65535, 65536, 65537]   # both sides of the 8- and 16-plane limits
assert len(E64) == 64 and sorted(set(E64)) == E64


def _opts(d):
    o = make_options(d)
    return CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                           o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def same_runs(got, depth, edges, what):
    s, v = runs_ref.runs(depth, edges)
    assert got.extent == len(depth) and got.n_runs == len(s), (what, got.n_runs, len(s))
    assert np.array_equal(got.start, s), (what, "start")
    assert np.array_equal(got.value, v), (what, "value")


def check(contigs, opt_dict, tmp_path, edge_sets=EDGE_SETS, expect=None, o_res=None):
    """every contig through the product path on one engine; while it is resident: the runs of both kinds for every edge
    set against the oracle's depths and the engine's own dump, the invariants, the ties to the depth profile, a repeated
    call, and the run repeated.  expect(name, kind, edges, runs): what a case wants to see beyond that.  o_res: what
    oracle_run gave for these contigs and options, where a case has it already."""
    opt = _opts(opt_dict)
    if o_res is None:
        o_res, _ = oracle_run(contigs, make_options(opt_dict), str(tmp_path / "o.bed"), dump=True)
    with Engine(opt, 0) as eng:
        counter = CallableProfiler(str(tmp_path / "g.bed"))
        for name, tid, length, ref, rec in contigs:
            process_single_contig(eng, counter, ContigProfiler(name, length), opt, tid, rec, ref)
            before = eng.contig_collect()
            extent = int(before.summary.extent)
            ro, qo, _, _, eo = o_res[name]["dumps"]
            assert extent == max(eo, length)
            oracle = {"raw": depth_ref.pad(ro, extent), "qc": depth_ref.pad(qo, extent)}
            d_raw, d_qc, _, _ = eng.debug_depths(extent)
            dump = {"raw": d_raw, "qc": d_qc}
            prof = eng.depth_profile(4096, 0)
            for kind in ("raw", "qc"):
                for edges in edge_sets:
                    got = eng.depth_runs(kind, edges)
                    what = (name, kind, edges and len(edges))
                    same_runs(got, oracle[kind], edges, what + ("oracle",))
                    same_runs(got, dump[kind], edges, what + ("debug_depths",))
                    if extent:
                        assert got.start[0] == 0, what
                        assert np.all(got.start[1:] > got.start[:-1]), what
                        assert np.all(got.value[1:] != got.value[:-1]), what
                        assert int(got.start[-1]) < extent, what
                    else:
                        assert got.n_runs == 0 and got.start.shape == (0,), what
                    if edges:
                        assert got.n_runs == 0 or int(got.value.max()) <= len(edges), what
                    else:
                        # what ties the exact runs to the depth profile
                        ln = got.ends() - got.start.astype(np.uint64)
                        total, hist = (prof.sum_raw, prof.hist_raw) if kind == "raw" else (prof.sum_qc, prof.hist_qc)
                        assert int((ln * got.value.astype(np.uint64)).sum()) == total, what
                        if hist[-1] == 0:
                            per = np.bincount(got.value.astype(np.int64), weights=ln.astype(np.float64), minlength=4096)
                            assert np.array_equal(per.astype(np.uint64), hist), what
                    again = eng.depth_runs(kind, edges)
                    assert np.array_equal(again.start, got.start) and np.array_equal(again.value, got.value), what
                    if expect:
                        expect(name, kind, edges, got)
            # the runs left the run's results alone, and the contig runs again as before
            eng.contig_run()
            after = eng.contig_collect()
            assert after.as_dict() == before.as_dict()
            assert np.array_equal(np.asarray(after.intervals), np.asarray(before.intervals))
        counter.close()


@pytest.mark.parametrize("case", KATS["cases"], ids=[c["name"] for c in KATS["cases"]])
def test_kats(case, tmp_path):
    opt = {**KATS["default_options"], **case.get("options", {})}
    contigs = []
    for i, c in enumerate(case["contigs"]):
        rec, ref = contig_inputs(c)
        contigs.append((c["name"], c.get("tid", i), c["len"], ref, rec))
    check(contigs, opt, tmp_path)


@pytest.mark.parametrize("seed", [1, 3, 4, 6, 7])
def test_adversarial_contigs_with_overhang(seed, tmp_path):
    """lengths 2048, 2049, 4096, 6143 and 1: the extent on, one past and far from a window boundary, some with overhang"""
    L = [777, 2048, 2049, 4096, 5000, 6143, 1, 300][seed]
    n = [200, 500, 500, 900, 1200, 700, 5, 2000][seed]
    rec = synth.adversarial_contig(L, n, 1000 + seed, max_len=min(300, max(2, L)), deep=(seed in (3, 7)), overhang=(seed in (1, 4, 6)))
    ref = synth.make_reference(L, 50 + seed, lowercase=(seed % 2 == 0))
    check([("chrA", seed % 3, L, ref, rec)], dict(min_depth=2, min_depth_for_low_mapq=3), tmp_path)


def _hand(reads):
    return ContigRecords.from_reads([(p, cig, 60, 30, 0, f"h{i}") for i, (p, cig) in enumerate(reads)])


def _sees_one(edges):
    """whether the values tell depth 1 from depth 0"""
    return not edges or edges[0] == 1


def _seam(reads, tmp_path, expect):
    L = 10_000
    seen = []

    def exp(name, kind, edges, got):
        seen.append(kind)
        expect(kind, edges, got)
    check([("chrS", 0, L, synth.make_reference(L, 77), _hand(reads))], dict(), tmp_path, expect=exp)
    assert seen.count("raw") == len(EDGE_SETS) and seen.count("qc") == len(EDGE_SETS)


def test_seam_one_read_across_two_boundaries(tmp_path):
    def expect(kind, edges, got):
        assert 2048 not in got.start and 4096 not in got.start
        assert (got.start.tolist(), got.value.tolist()) == (([0, 1000, 5000], [0, 1, 0]) if _sees_one(edges) else ([0], [0]))
    _seam([(1000, "4000M")], tmp_path, expect)


def test_seam_a_run_that_ends_on_a_boundary(tmp_path):
    def expect(kind, edges, got):                                   # depth 1 on both sides of 2048: one run
        assert (got.start.tolist(), got.value.tolist()) == (([0, 2148], [1, 0]) if _sees_one(edges) else ([0], [0]))
    _seam([(0, "2048M"), (2048, "100M")], tmp_path, expect)

    def expect2(kind, edges, got):                                  # depth 1 up to the boundary, 2 behind it
        if not edges or 2 in edges:
            assert got.start.tolist() == [0, 2048, 2148]
        else:
            assert 2048 not in got.start
    (tmp_path / "b").mkdir()
    _seam([(0, "2048M"), (2048, "100M"), (2048, "100M")], tmp_path / "b", expect2)


def test_seam_zero_depth_across_whole_empty_windows(tmp_path):
    def expect(kind, edges, got):
        exp = ([0, 100, 150, 3 * 2048 + 5, 3 * 2048 + 55], [0, 1, 0, 1, 0]) if _sees_one(edges) else ([0], [0])
        assert (got.start.tolist(), got.value.tolist()) == exp
    _seam([(100, "50M"), (3 * 2048 + 5, "50M")], tmp_path, expect)


def test_seam_abutting_reads_drop_and_keep(tmp_path):
    def dropped(kind, edges, got):                                  # equal depth on both sides of 4096
        assert (got.start.tolist(), got.value.tolist()) == (([0, 3596, 4596], [0, 1, 0]) if _sees_one(edges) else ([0], [0]))
    (tmp_path / "d").mkdir()
    _seam([(3596, "500M"), (4096, "500M")], tmp_path / "d", dropped)

    def kept(kind, edges, got):                                     # 2 below 4096, 1 from it
        if not edges or (1 in edges and 2 in edges):
            assert got.start.tolist() == [0, 3596, 3896, 4096, 4596] and got.value[2] != got.value[3]
        elif 2 in edges:                                            # depths 0 and 1 share a band
            assert got.start.tolist() == [0, 3896, 4096] and got.value.tolist() == [0, 1, 0]
        else:
            assert got.start.tolist() == [0, 3596, 4596]            # 1 and 2 share a band: no start at the seam
    (tmp_path / "k").mkdir()
    _seam([(3596, "500M"), (3896, "200M"), (4096, "500M")], tmp_path / "k", kept)


def test_short_reads_2mb_30x(tmp_path):
    L = 2_000_000
    rec = synth.short_read_contig(L, 30, synth.seed_for(2, 20))
    check([("chr21", 20, L, synth.make_reference(L, synth.seed_for(2, 20)), rec)], dict(), tmp_path)


SCAN_EDGE_SETS = (None, [1, 4, 100], E64)


def _runs_around(start, value, B):
    """the (start, value) of the runs that start inside the zone cleared around B -- behind its first position, where the
    background's last run may end --, and the value at B"""
    lo, hi = np.searchsorted(start, [B - depth_contigs.SCAN_CLEAR + 1, B + depth_contigs.SCAN_CLEAR])
    at = int(value[np.searchsorted(start, B, side="right") - 1])
    return [(int(s), int(v)) for s, v in zip(start[lo:hi], value[lo:hi])], at


def _scan_boundaries_as_planted(start, value, edges, what):
    B1, B2, B3 = depth_contigs.SCAN_B
    # B_1, one read across: no start at it, the provisional start of window 1024 is dropped across the step
    assert _runs_around(start, value, B1) == ([(B1 - 500, 1), (B1 + 500, 0)], 1), what
    # B_2, nothing: depth 0 goes on
    assert _runs_around(start, value, B2) == ([], 0), what
    # B_3, 1 and 2 below it, 1 from it: a start of its own unless 1 and 2 share a band
    if edges == [1, 4, 100]:
        assert _runs_around(start, value, B3) == ([(B3 - 500, 1), (B3 + 500, 0)], 1), what
    else:
        assert _runs_around(start, value, B3) == ([(B3 - 500, 1), (B3 - 200, 2), (B3, 1), (B3 + 500, 0)], 1), what


def test_scan_of_four_steps_with_runs_across_its_step_boundaries(tmp_path):
    """3078 windows: k_depth_runs_scan takes four steps of 1024 windows.  Around the first positions of windows 1024, 2048
    and 3072 the background is cleared and the three ways of a run to meet a step boundary are planted."""
    contig, o_res, extent, depths = depth_contigs.scan_steps()
    assert extent == depth_contigs.SCAN_L and -(-extent // depth_contigs.T) == 3078
    # from the reference alone: every step's offset carry is non-zero and every later step has runs to place, and the
    # boundaries are what the planted reads say
    for kind in ("raw", "qc"):
        for edges in SCAN_EDGE_SETS:
            s, v = runs_ref.runs(depths[kind], edges)
            n_from = [int((s >= B).sum()) for B in (0,) + depth_contigs.SCAN_B]
            assert n_from[0] > n_from[1] > n_from[2] > n_from[3] > 10, (kind, edges, n_from)
            _scan_boundaries_as_planted(s, v, edges, (kind, edges, "reference"))
    seen = []

    def expect(name, kind, edges, got):
        seen.append(kind)
        _scan_boundaries_as_planted(got.start, got.value, edges, (kind, edges))
    check([contig], {}, tmp_path, edge_sets=SCAN_EDGE_SETS, expect=expect, o_res=o_res)
    assert seen.count("raw") == seen.count("qc") == len(SCAN_EDGE_SETS)


def test_contig_beyond_the_grid_of_65536_workgroups():
    """65540 windows: workgroups 0..3 of k_depth_runs take a second window in both passes, the scan takes 65 steps, every
    workgroup of k_depth_profile takes 32 or 33 windows.  134,223,877 positions are too many for the oracle and for
    per-position arrays: a few thousand reads of one M each, against tests/sparse_ref.py.
    Residents and kernels follow the 65540 window records, not the positions: on an MI355X the whole test takes 0.08 s
    (begin to finish 0.02 s, the eight depth_runs and the six depth_profile calls under 0.01 s each lot); it prints the
    stage times (-s)."""
    T, B, L = depth_contigs.T, depth_contigs.BIG_B, depth_contigs.BIG_L
    rec, raw, qc = depth_contigs.beyond_the_runs_grid()
    reads = {"raw": raw, "qc": qc}
    assert -(-L // T) == depth_contigs.RUNS_GRID + 4 and B % (1024 * T) == 0
    # from the reference alone: a workgroup's two windows hold depth of both kinds, and not the same; the boundaries
    per_window = sparse_ref.profile(raw, qc, L, 2, T)
    for w in (1, 2, 3, depth_contigs.RUNS_GRID, depth_contigs.RUNS_GRID + 1, depth_contigs.RUNS_GRID + 2, depth_contigs.RUNS_GRID + 3):
        assert per_window["win_raw"][w] > per_window["win_qc"][w], w
    for kind in ("raw", "qc"):
        win = per_window["win_" + kind]
        for k in range(4):
            assert win[k] > 0 and win[depth_contigs.RUNS_GRID + k] > 0 and win[k] != win[depth_contigs.RUNS_GRID + k], (kind, k)
        for edges in (None, [1, 2]):
            s, v = sparse_ref.runs(*reads[kind], L, edges)
            at = dict(zip(s.tolist(), v.tolist()))
            assert B not in at and B - 50 in at and at[B - 50] == 2            # 2 on both sides of B: no start
            assert at[B + T - 100] == 2 and at[B + T] == 1                     # 2 below B + 2048, 1 from it: a start
            assert int((s >= B).sum()) > 10
    t = [time.perf_counter()]
    opt = _opts({})
    with Engine(opt, 0) as eng:
        eng.contig_begin(7, L, None)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        before = eng.contig_finish()
        t.append(time.perf_counter())
        summary = before.summary
        assert int(summary.extent) == L
        for kind in ("raw", "qc"):
            for edges in (None, [1, 2]):
                got = eng.depth_runs(kind, edges)
                s, v = sparse_ref.runs(*reads[kind], L, edges)
                assert got.extent == L and got.n_runs == len(s), (kind, edges, got.n_runs, len(s))
                assert np.array_equal(got.start, s), (kind, edges, "start")
                assert np.array_equal(got.value, v), (kind, edges, "value")
                again = eng.depth_runs(kind, edges)
                assert np.array_equal(again.start, got.start) and np.array_equal(again.value, got.value), (kind, edges)
        t.append(time.perf_counter())
        for nb, S in ((1001, 0), (17, 500), (4096, 100_000)):
            got = eng.depth_profile(nb, S)
            exp = sparse_ref.profile(raw, qc, L, nb, S)
            what = (nb, S)
            assert (got.n_bins, got.window, got.n_windows, got.extent) == (nb, S, exp["n_windows"], L), what
            assert (got.sum_raw, got.sum_qc) == (exp["sum_raw"], exp["sum_qc"]), what
            assert got.sum_raw != got.sum_qc
            assert np.array_equal(got.hist_raw, exp["hist_raw"]) and np.array_equal(got.hist_qc, exp["hist_qc"]), what
            if S:
                assert np.array_equal(got.win_raw, exp["win_raw"]) and np.array_equal(got.win_qc, exp["win_qc"]), what
            else:
                assert got.win_raw is None and got.win_qc is None
            assert got.sum_raw == summary.summed_coverage and got.sum_qc == summary.quality_bases, what
            assert L - int(got.hist_raw[0]) == summary.n_covered_bases, what
            assert int(got.hist_raw.sum()) == int(got.hist_qc.sum()) == L, what
            again = eng.depth_profile(nb, S)
            assert np.array_equal(again.hist_raw, got.hist_raw) and np.array_equal(again.hist_qc, got.hist_qc), what
            assert (again.sum_raw, again.sum_qc) == (got.sum_raw, got.sum_qc), what
            if S:
                assert np.array_equal(again.win_raw, got.win_raw) and np.array_equal(again.win_qc, got.win_qc), what
        t.append(time.perf_counter())
        eng.contig_run()
        after = eng.contig_collect()
        assert after.as_dict() == before.as_dict()
        assert np.array_equal(np.asarray(after.intervals), np.asarray(before.intervals))
        t.append(time.perf_counter())
    print("134,223,877 positions: begin to finish %.2f s, 8 depth_runs %.2f s, 6 depth_profile %.2f s, run again %.2f s"
          % tuple(b - a for a, b in zip(t, t[1:])))


def test_candidates_beyond_32767_in_a_window(tmp_path):
    """k_depth_runs has its own copy of the window-depth rebuild: the difference words must hold these counts too"""
    L = 5000
    rng = np.random.default_rng(5)
    reads = [(int(p), "30M", 60, 30, 0, f"r{i}") for i, p in enumerate(np.sort(rng.integers(100, 1900, 40_000)))]
    check([("chrP", 0, L, synth.make_reference(L, 9), ContigRecords.from_reads(reads))], dict(max_depth=1_000_000), tmp_path)


@pytest.mark.parametrize("head_span", ["37", "1000"])
def test_spans_cut_into_several_heads(head_span, tmp_path, monkeypatch):
    monkeypatch.setenv("DUT_HEAD_SPAN", head_span)
    rec = synth.long_read_contig(60_000, 8, 17)
    check([("chrL", 2, 60_000, synth.make_reference(60_000, 3), rec)], None, tmp_path)


def test_windows_that_only_the_wide_list_covers(tmp_path):
    contig, o_res, extent, depths = depth_contigs.wide_list()
    assert extent == depth_contigs.WIDE_L
    depth_contigs.assert_wide_only_windows(contig[4], depths)
    check([contig], depth_contigs.WIDE_OPTIONS, tmp_path, o_res=o_res)


def test_long_reads_indel_rich(tmp_path):
    """deletions and skips count in raw only: the two kinds differ"""
    L = 300_000
    rec = synth.long_read_contig(L, 50, synth.seed_for(3, 23))
    kinds = {}
    check([("chrY", 23, L, synth.make_reference(L, synth.seed_for(3, 23)), rec)], dict(), tmp_path,
          expect=lambda name, kind, edges, got: kinds.setdefault((kind, None if not edges else len(edges)), got))
    assert not np.array_equal(kinds[("raw", None)].start, kinds[("qc", None)].start)


@pytest.mark.parametrize("depth,planes", [(300, 16), (66_000, 32)])
def test_deep_piles_select_the_16_and_32_plane_kernels(depth, planes, tmp_path):
    L = 7000
    rng = np.random.default_rng(depth)
    reads = [[int(p), "120M" if depth < 1000 else "20M", int(rng.choice([10, 20, 60, 60])), int(rng.choice([10, 20, 40])), 0, f"d{i}"]
             for i, p in enumerate(np.sort(rng.integers(2000, 2060 if depth < 1000 else 2004, depth)))]
    rec = ContigRecords.from_reads([tuple(r) for r in reads])
    ref = synth.make_reference(L, 8)
    top = {}
    check([("chrD", 3, L, ref, rec)], dict(max_depth=1_000_000), tmp_path, edge_sets=EDGE_SETS + (AROUND_THE_PLANES,),
          expect=lambda name, kind, edges, got: top.setdefault(kind, int(got.value.max())) if not edges else None)
    assert top["raw"] == depth and 0 < top["qc"] <= depth
    with Engine(_opts(dict(max_depth=1_000_000)), 0) as eng:
        eng.contig_begin(3, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        assert eng.contig_layout()["counter_planes"] == planes


def test_empty_contigs(tmp_path):
    check([("e1", 0, 0, None, ContigRecords.empty()), ("e2", 1, 5000, None, ContigRecords.empty()),
           ("e3", 2, 4096, synth.make_reference(4096, 3), ContigRecords.empty())], dict(), tmp_path)
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, 5000, None)
        eng.contig_finish()
        r = eng.depth_runs("qc", [1, 4])
        assert (r.n_runs, r.start.tolist(), r.value.tolist(), r.extent) == (1, [0], [0], 5000)


def test_profiling_times_both_launches():
    L = 50_000
    rec = synth.short_read_contig(L, 20, 3)
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, L, synth.make_reference(L, 4))
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        assert eng.depth_runs("raw").kernel_ms == 0.0
        eng.set_profiling(True)
        assert eng.depth_runs("raw").kernel_ms > 0.0 and eng.depth_runs("qc", [1, 4, 100]).kernel_ms > 0.0
        eng.set_profiling(False)
        assert eng.depth_runs("qc").kernel_ms == 0.0


def test_refusals(monkeypatch):
    L = 3000
    rec = synth.short_read_contig(L, 10, 5)
    ref = synth.make_reference(L, 6)
    with Engine(CallableOptions(), 0) as eng:
        def refused(kind, edges, text):
            with pytest.raises(EngineError) as e:
                eng.depth_runs(kind, edges)
            assert e.value.status == -1 and text in str(e.value), str(e.value)
        refused("raw", None, "has been run")                       # nothing resident
        eng.contig_begin(0, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        refused("raw", None, "has been run")                       # begun, not run
        eng.contig_upload()
        refused("qc", [1], "has been run")                         # uploaded, not run
        eng.contig_run()
        s = eng.contig_collect().summary
        refused("raw", [0, 1, 4], "first edge")
        refused("raw", [4, 1], "ascending")
        refused("qc", [1, 4, 4], "ascending")
        refused("raw", list(range(1, 66)), "64 edges")
        refused(2, None, "kind")
        r = eng.depth_runs("raw", list(range(1, 65)))
        assert r.extent == s.extent and r.start[0] == 0
    monkeypatch.setenv("DUT_QUAL_FORM", "bytes")
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        with pytest.raises(EngineError) as e:
            eng.depth_runs("raw")
        assert e.value.status == -1 and "pass-bit form only" in str(e.value)


def test_depth_bed_files_one_device_several_contexts_and_the_tool(tmp_path):
    names = ["chr1", "chr2", "chrM"]
    lens = [150_000, 60_000, 16_569]
    recs = {0: synth.short_read_contig(lens[0], 30, 900), 1: synth.long_read_contig(lens[1], 20, 902),
            2: synth.short_read_contig(lens[2], 20, 905)}
    refs = [synth.make_reference(l, 950 + i, lowercase=(i == 2)) for i, l in enumerate(lens)]
    bam = str(tmp_path / "m.bam"); fa = str(tmp_path / "m.fa")
    write_bam(bam, list(zip(names, lens)), recs, block_every=800)
    write_fasta(fa, list(zip(names, refs)))
    contigs = [(n, t, lens[t], refs[t], recs[t]) for t, n in enumerate(names)]
    o_res, o_bed = oracle_run(contigs, make_options({}), str(tmp_path / "o.bed"), dump=True)
    depths, profs = {"raw": [], "qc": []}, []
    for name, _, length, _, _ in contigs:
        ro, qo, _, _, eo = o_res[name]["dumps"]
        ext = max(eo, length)
        depths["raw"].append((name, depth_ref.pad(ro, ext))); depths["qc"].append((name, depth_ref.pad(qo, ext)))
        profs.append((name, depth_ref.profile(depths["raw"][-1][1], depths["qc"][-1][1], 41, 0)))

    def text(kind, edges):
        return "".join(runs_ref.bed_text_of(n, d, edges) for n, d in depths[kind])
    plain = tmp_path / "plain"; plain.mkdir()
    coverage_files(bam, fa, str(plain / "g.bed"), str(plain / "s.json"), CallableOptions())
    assert open(plain / "g.bed").read() == o_bed

    def same_summary(d, how):
        assert open(d / "g.bed").read() == o_bed, how
        a, b = json.load(open(plain / "s.json")), json.load(open(d / "s.json"))
        a["files"] = b["files"] = None                              # (the paths differ)
        assert a == b, how

    for q, edges in ((None, None), ("0:1:4:100:", [1, 4, 100])):
        outs = []
        for devs in ([0], [0, 0, 0]):
            d = tmp_path / ("q%d_dev%d" % (bool(q), len(devs))); d.mkdir()
            coverage_files(bam, fa, str(d / "g.bed"), str(d / "s.json"), CallableOptions(), devices=devs, depth_bed=str(d / "d.bed"), quantize=q)
            outs.append(open(d / "d.bed").read())
            same_summary(d, (q, devs))
        assert outs[0] == outs[1] == text("raw", edges), q
    assert "\t100:inf\n" not in text("raw", [1, 4, 100]) and "\t4:100\n" in text("raw", [1, 4, 100])
    # together with the depth profile's flags: both outputs
    d = tmp_path / "both"; d.mkdir()
    coverage_files(bam, fa, str(d / "g.bed"), str(d / "s.json"), CallableOptions(), devices=[0, 0], depth_bed=str(d / "d.bed"), depth_bed_kind="qc",
                   quantize="1:4:100", depth_dist=str(d / "d.tsv"), depth_cap=40)
    assert open(d / "d.bed").read() == text("qc", [1, 4, 100])
    assert open(d / "d.tsv").read() == depth_ref.dist_text(profs)
    same_summary(d, "both")
    # through the tool (it writes ./summary.json)
    d = tmp_path / "cli"; d.mkdir()
    r = subprocess.run([_b.CLI, "coverage", bam, "-r", fa, "-o", "g.bed", "-s", "r.html", "--depth-bed", "d.bed", "--depth-bed-kind", "qc",
                        "--quantize", "1:4:100"], cwd=str(d), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    os.rename(d / "summary.json", d / "s.json")
    assert open(d / "d.bed").read() == text("qc", [1, 4, 100])
    same_summary(d, "cli")
    with pytest.raises(EngineError):                                # the keyword arguments' own rules
        coverage_files(bam, fa, str(d / "x.bed"), None, CallableOptions(), quantize="1:4")
    with pytest.raises(EngineError):
        coverage_files(bam, fa, str(d / "x.bed"), None, CallableOptions(), depth_bed=str(d / "x.dbed"), quantize="4:1")
    assert not (d / "x.bed").exists()
