"""The GC-bias profile on the device (-m gpu): cl_contig_gc_bias against tests/gc_ref.py applied to the CPU oracle's
per-position raw_depth / qc_depth, and to the engine's own cl_debug_depths.  The call takes its own reference, so the
contigs of tests/depth_contigs.py are reused with designed references built here.  Counts: everything is exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import depth_contigs
import depth_ref
import gc_ref
from bamio import write_bam, write_fasta
from helpers import contig_inputs, load_kats, make_options, oracle_run
from decodingustools_amd import (CallableOptions, CallableProfiler, ContigProfiler, Engine, EngineError, _lib, build as _b,
                                 process_single_contig, synth)
from decodingustools_amd.bam import coverage_files
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu
KATS = load_kats()
T = depth_contigs.T
HOOKS = ("DUT_HEADS8", "DUT_HEAD_SPAN", "DUT_QUAL_FORM", "DUT_ROWS_UNIFORM")   # (read when an engine is made)
KAT_WINDOWS = (1, 2, 3, 15, 16, 17, 100, 1024)


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)


def _opts(d):
    o = make_options(d)
    return CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                           o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def limits(W):
    """K in (0, 4, W - 1), those the contract admits (K < W); the others must be refused"""
    return sorted({k for k in (0, 4, W - 1) if k < W}), sorted({k for k in (0, 4, W - 1) if k >= W})


def designed_ref(L, seed=0):
    """blocks of pure AT, pure GC and alternating composition, N runs, a soft-masked stretch, IUPAC S and R; block
    lengths from 1 to 97 so that every window length of the tests sees block edges at every phase"""
    rng = np.random.default_rng(1000 + seed)
    kinds = (b"AT", b"GC", b"AGTC", b"N", b"atgc", b"S", b"R", b"ATTA", b"GCCG", b"n", b"gc", b"at")
    weights = np.asarray([4, 4, 3, 1, 2, 1, 1, 2, 2, 1, 1, 1], float)
    out = np.zeros(L, np.uint8)
    p = 0
    while p < L:
        k = kinds[int(rng.choice(len(kinds), p=weights / weights.sum()))]
        n = int(rng.integers(1, 98)) if k not in (b"N", b"n", b"S", b"R") else int(rng.integers(1, 9))
        n = min(n, L - p)
        out[p:p + n] = np.resize(np.frombuffer(k, np.uint8), n)
        p += n
    return out


def clean_ref(L, seed=0):
    """A C G T only"""
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(2000 + seed).integers(0, 4, L)].copy()


def compare(eng, ref, combos, depths, what, extent):
    """eng.gc_bias(ref, W, K) for every (W, K) against gc_ref over every (label, raw, qc) of depths; the invariant that
    ties it to the extent.  Returns the records."""
    out = {}
    for W, K in combos:
        got = eng.gc_bias(ref, W, K)
        for label, raw, qc in depths:
            gc_ref.same(got, gc_ref.profile(raw, qc, ref, W, K), (what, W, K, label))
        assert int(got.positions.sum()) + got.n_skipped == extent == got.extent, (what, W, K)
        out[(W, K)] = got
    return out


def make_resident(eng, opt, contig, tmp_path):
    """the contig through the product path (admission of the reads included), left resident and collected: its extent"""
    name, tid, length, ref, rec = contig
    counter = CallableProfiler(str(tmp_path / "g.bed"))
    process_single_contig(eng, counter, ContigProfiler(name, length), opt, tid, rec, ref)
    counter.close()
    return int(eng.contig_collect().summary.extent)


def run_contigs(contigs, opt_dict, tmp_path, refs, combos, o_res=None):
    """every contig through the product path on one engine; while it is resident: the record for every designed reference
    of refs(name, length, extent) and every (W, K) against the oracle's depths and the engine's own dump; then the run
    repeated: it gives what it gave"""
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
            d_raw, d_qc, _, _ = eng.debug_depths(extent)
            depths = [("oracle", depth_ref.pad(ro, extent), depth_ref.pad(qo, extent)), ("debug_depths", d_raw, d_qc)]
            for label, gref in refs(name, length, extent):
                compare(eng, gref, combos, depths, (name, label), extent)
            eng.contig_run()
            after = eng.contig_collect()
            assert after.as_dict() == before.as_dict()
            assert np.array_equal(np.asarray(after.intervals), np.asarray(before.intervals))
        counter.close()


# ---- 1. the known-answer contigs ----
@pytest.mark.parametrize("case", KATS["cases"], ids=[c["name"] for c in KATS["cases"]])
def test_kats(case, tmp_path):
    opt = {**KATS["default_options"], **case.get("options", {})}
    contigs = []
    for i, c in enumerate(case["contigs"]):
        rec, ref = contig_inputs(c)
        contigs.append((c["name"], c.get("tid", i), c["len"], ref, rec))
    combos = [(W, K) for W in KAT_WINDOWS for K in limits(W)[0]]
    assert len(combos) == 1 + 2 + 2 + 3 * 5 and (1024, 1023) in combos and (1, 0) in combos
    run_contigs(contigs, opt, tmp_path, lambda name, length, extent: [("designed", designed_ref(extent, length))], combos)
    # K = 4 where the window is no longer than that: the contract's refusal, not a case
    name, tid, length, ref, rec = contigs[0]
    with Engine(_opts(opt), 0) as eng:
        eng.contig_begin(tid, length, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        for W in KAT_WINDOWS:
            for K in limits(W)[1]:
                with pytest.raises(EngineError) as e:
                    eng.gc_bias(designed_ref(length), W, K)
                assert e.value.status == -1 and "max_invalid" in str(e.value)


# ---- 2. composition steps and N runs planted at the engine's boundaries ----
EDGE_L = 3 * T + 17


def edge_ref(W, K):
    """AT -> GC -> AT ... steps at the first window boundary as the halo of W sees it (2048 - W/2, 2048, 2048 + W - W/2),
    at a thread boundary +- 1 (16 * 50) and at the bit-word boundaries 32 and 64 +- 1; a run of exactly K and one of K + 1
    'N' around position 4096, the second window boundary"""
    steps = sorted({31, 32, 33, 63, 64, 65, 799, 800, 801, T - W // 2, T, T + W - W // 2, 3 * T - 1, 3 * T, 3 * T + 16})
    ref = np.zeros(EDGE_L, np.uint8)
    prev, gc = 0, False
    for s in steps + [EDGE_L]:
        ref[prev:s] = np.resize(np.frombuffer(b"GC" if gc else b"AT", np.uint8), s - prev)
        prev, gc = s, not gc
    a = 2 * T - K // 2                                              # K 'N' across 4096 (K = 0: none)
    ref[a:a + K] = ord("N")
    b = a + K + W + 5                                               # ... and K + 1 of them one window further
    ref[b:b + K + 1] = ord("N")
    return ref, (a, b)


@pytest.fixture(scope="module")
def edge_contig():
    rec = synth.short_read_contig(EDGE_L, 10, 77, read_len=50)
    return depth_contigs._with_oracle(("chrE", 1, EDGE_L, synth.make_reference(EDGE_L, 78), rec), {})


@pytest.mark.parametrize("W", [2, 33, 100, 1023, 1024])
def test_edges_at_engine_boundaries(W, edge_contig, tmp_path):
    contig, o_res, extent, depths = edge_contig
    assert extent == EDGE_L
    K = 1 if W == 2 else 4
    ref, (a, b) = edge_ref(W, K)
    # from the rule alone: the run of K leaves every position around it counted, the run of K + 1 skips exactly the
    # W - K positions whose window holds it whole
    _, v = gc_ref.window_counts(ref, extent, W)
    first = b + K + 1 - (W - W // 2)                                # the first position whose window ends behind the run
    assert int(v[a - W:first].max()) == K                           # (no window holds bases of both runs: W + 5 lie between)
    assert (v[first:first + W - K] == K + 1).all() and v[first - 1] == K and v[first + W - K] == K
    run_contigs([contig], {}, tmp_path, lambda *_: [("edges", ref)], [(W, k) for k in sorted({0, K, W - 1})], o_res=o_res)


# ---- 3. the contig's ends ----
def test_overhanging_reads_and_reference_lengths(tmp_path):
    L = 777
    rec = synth.adversarial_contig(L, 200, 1001, max_len=300, overhang=True)
    contig = ("chrA", 1, L, synth.make_reference(L, 51), rec)
    seen = {}

    def refs(name, length, extent):
        assert extent > length                                      # the reads overhang
        seen["extent"] = extent
        full = designed_ref(extent + 300, 5)
        return [("ref_len < contig_len", full[:500]), ("ref_len == contig_len", full[:length]), ("ref_len == extent", full[:extent]),
                ("ref_len > extent", full), ("ref_len == 0", np.zeros(0, np.uint8)), ("no reference", None), ("one base", full[:1])]
    run_contigs([contig], dict(min_depth=2, min_depth_for_low_mapq=3), tmp_path, refs, [(1, 0), (16, 4), (100, 4), (100, 99), (1024, 1023)])
    assert seen["extent"] > L


def test_a_contig_of_length_one(tmp_path):
    rec = ContigRecords.from_reads([(0, "1M", 60, 30, 0, "a"), (0, "1M", 60, 30, 0, "b"), (0, "1M", 5, 30, 0, "c")])
    ref = np.frombuffer(b"G", np.uint8)
    run_contigs([("one", 0, 1, ref, rec)], dict(min_depth=1), tmp_path,
                lambda *_: [("G", ref), ("A", np.frombuffer(b"A", np.uint8)), ("N", np.frombuffer(b"N", np.uint8)), ("GG", np.frombuffer(b"GGGG", np.uint8))],
                [(1, 0), (2, 1), (3, 2), (100, 99), (1024, 1023)])
    with Engine(_opts(dict(min_depth=1)), 0) as eng:
        eng.contig_begin(0, 1, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        g = eng.gc_bias(ref, 1, 0)
        assert g.extent == 1 and g.n_skipped == 0 and g.positions[100] == 1 and g.sum_raw[100] >= g.sum_qc[100] == 2
        g = eng.gc_bias(ref, 2, 0)                                  # the window [-1, 1) holds an invalid position
        assert g.n_skipped == 1 and not g.positions.any() and not g.sum_raw.any()
        # an empty contig: nothing counted, nothing skipped
        eng.contig_begin(1, 0, None)
        eng.contig_finish()
        g = eng.gc_bias(ref, 100, 4)
        assert g.extent == 0 and g.n_skipped == 0 and not g.positions.any()


# ---- 4. two windows per workgroup: the grid of k_gc_bias is min(windows, 2048), as k_depth_profile's ----
def test_two_windows_per_workgroup(tmp_path):
    """3078 windows on a grid of 2048: workgroups 0..1029 take windows w and w + 2048, both in their LDS bins, with the
    second stretch of bit words loaded over the first; the composition steps at the first position of window 2048"""
    contig, o_res, extent, depths = depth_contigs.scan_steps()
    B2 = depth_contigs.SCAN_B[1]
    assert extent == depth_contigs.SCAN_L and -(-extent // T) == 2048 + 1030 and B2 == 2048 * T
    ref = np.resize(np.frombuffer(b"ATTAAATT" * 8 + b"ACGT" * 16 + b"NNN" + b"AGTC" * 9, np.uint8), extent).copy()
    ref[B2:] = np.resize(np.frombuffer(b"GCCGGGCC" * 8 + b"ACGG" * 16 + b"SSSSS" + b"GGTC" * 9, np.uint8), extent - B2)
    d = [("oracle", depths["raw"], depths["qc"])]
    opt = _opts({})
    with Engine(opt, 0) as eng:
        assert make_resident(eng, opt, contig, tmp_path) == extent
        # (K = 30 at W = 1024: a window there holds six or seven of the runs of three 'N' or five 'S')
        got = compare(eng, ref, [(100, 4), (1024, 30)], d, "scan_steps", extent)
    for g in got.values():
        # both halves of the step are there: bins below 50 from the first 2048 windows, above from the others
        assert int(g.positions[:50].sum()) > 200 * T and int(g.positions[51:].sum()) > 200 * T and g.n_skipped > 50 * T


# ---- 5. the forms the rebuild takes: the wide list, a second trip of the candidate loop, 16 planes; both head forms ----
FORMS = {"wide_list": (depth_contigs.wide_list, depth_contigs.WIDE_OPTIONS, None),
         "wide_pile": (lambda: depth_contigs.wide_pile(140), depth_contigs.PILE_OPTIONS, None),
         "deep_pile": (lambda: depth_contigs.deep_pile(300), depth_contigs.DEEP_OPTIONS, 16)}


@pytest.mark.parametrize("name", list(FORMS))
def test_rebuild_forms_under_both_head_forms(name, monkeypatch, tmp_path):
    build, options, planes = FORMS[name]
    contig, o_res, extent, depths = build()
    ref = designed_ref(extent, 9)
    d = [("oracle", depths["raw"], depths["qc"])]
    seen = {}
    for heads8 in (False, True):
        if heads8:
            monkeypatch.setenv("DUT_HEADS8", "1")
        opt = _opts(options)
        with Engine(opt, 0) as eng:
            assert make_resident(eng, opt, contig, tmp_path) == extent
            lay = eng.contig_layout()
            if planes:
                assert lay["counter_planes"] == planes
            d_raw, d_qc, _, _ = eng.debug_depths(extent)
            got = compare(eng, ref, [(1, 0), (100, 4), (1024, 1023)], d + [("debug_depths", d_raw, d_qc)], (name, heads8), extent)
            seen[heads8] = (eng.contig_bytes()[0], lay["n_records"], {k: v.tobytes() for k, v in got.items()})
    # which head form ran: the hook costs 4 bytes a head where the contig takes 4-byte heads by itself, nothing otherwise
    (b4, n4, r4), (b8, n8, r8) = seen[False], seen[True]
    assert n4 == n8 > 0 and b8 - b4 in (0, 4 * n4) and r4 == r8
    if name == "deep_pile":
        assert b8 - b4 == 4 * n4                                    # short reads: both forms were run


def test_spans_cut_into_several_heads(monkeypatch, tmp_path):
    monkeypatch.setenv("DUT_HEAD_SPAN", "37")
    rec = synth.long_read_contig(30_000, 6, 17)
    run_contigs([("chrL", 2, 30_000, synth.make_reference(30_000, 3), rec)], None, tmp_path,
                lambda name, length, extent: [("designed", designed_ref(extent, 3))], [(100, 4), (1024, 0)])


# ---- 6. invariants ----
def test_invariants_interleaving_and_the_run_left_alone(tmp_path):
    L = 3 * T + 100
    rec = synth.short_read_contig(L, 12, 31)
    cref = synth.make_reference(L, 32)
    opt = CallableOptions()
    with Engine(opt, 0) as eng:
        eng.contig_begin(0, L, cref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_upload()
        eng.contig_run()
        extent = L
        ref = clean_ref(extent, 1)
        # before the contig is collected
        first = eng.gc_bias(ref, 1, 0)
        before = eng.contig_collect()
        s = before.summary
        assert int(s.extent) == extent == first.extent
        # no invalid base, ref_len == extent, W == 1: every position is in bin 0 or 100, and the sums are the summary's
        assert first.n_skipped == 0 and int(first.positions[0]) + int(first.positions[100]) == extent
        assert int(first.positions[100]) == int(gc_ref.IS_GC[ref].sum())
        assert int(first.sum_raw.sum()) == s.summed_coverage and int(first.sum_qc.sum()) == s.quality_bases
        assert extent - int(first.zero_raw.sum()) == s.n_covered_bases
        # two calls return the same bytes, with other calls between them
        d_raw, d_qc, _, _ = eng.debug_depths(extent)
        nref = designed_ref(extent, 2)
        a = eng.gc_bias(nref, 100, 4)
        prof = eng.depth_profile(1001, 0)
        b = eng.gc_bias(nref, 100, 4)
        tg = eng.target_stats([0, 100], [extent, 5000])
        order = eng.target_order([0], [extent])
        runs = eng.depth_runs("raw")
        c = eng.gc_bias(nref, 100, 4)
        eng.contig_run()
        d = eng.gc_bias(nref, 100, 4)
        assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()
        gc_ref.same(a, gc_ref.profile(d_raw, d_qc, nref, 100, 4), "interleaved")
        assert prof.sum_raw == int(tg.sum_raw[0]) == s.summed_coverage and int(order.len[0]) == extent and runs.extent == extent
        assert eng.depth_profile(1001, 0).hist_raw.tobytes() == prof.hist_raw.tobytes()
        # K == W - 1: skipped are the positions whose window holds no A/C/G/T; their depths are left out
        for W in (3, 100):
            g = eng.gc_bias(nref, W, W - 1)
            _, v = gc_ref.window_counts(nref, extent, W)
            assert g.n_skipped == int((v == W).sum())
            assert int(g.sum_raw.sum()) == int(d_raw[v < W].astype(np.uint64).sum()) and int(g.sum_qc.sum()) == int(d_qc[v < W].astype(np.uint64).sum())
            assert int(g.zero_raw.sum()) == int((d_raw[v < W] == 0).sum())
        assert int(eng.gc_bias(nref, 1, 0).n_skipped) == int(gc_ref.IS_INVALID[nref].sum()) > 0
        # the calls left the run alone
        after = eng.contig_collect()
        assert after.as_dict() == before.as_dict()
        assert np.array_equal(np.asarray(after.intervals), np.asarray(before.intervals))
        # records add up as dut_gc_bias_add has it
        gc_ref.same(a + a, gc_ref.add(gc_ref.add(None, a), a), "a + a")
        # the kernel's time is measured while profiling is on, the upload's always
        assert a.kernel_ms == 0.0 and a.upload_ms > 0.0
        eng.set_profiling(True)
        assert eng.gc_bias(nref, 100, 4).kernel_ms > 0.0


# ---- 7. refusals: a status and a message, the context usable afterwards ----
def test_refusals(monkeypatch):
    L = 3000
    rec = synth.short_read_contig(L, 10, 5)
    cref = synth.make_reference(L, 6)
    ref = designed_ref(L, 4)
    with Engine(CallableOptions(), 0) as eng:
        lib, h = eng._lib, eng._h

        def refused(text, *args, status=-1):
            with pytest.raises(EngineError) as e:
                eng.gc_bias(*args)
            assert e.value.status == status and text in str(e.value), str(e.value)
        refused("has been run", ref, 100, 4)                       # nothing resident
        eng.contig_begin(0, L, cref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        refused("has been run", ref, 100, 4)                       # begun, not run
        eng.contig_upload()
        refused("has been run", ref, 100, 4)                       # uploaded, not run
        eng.contig_run()
        good = eng.gc_bias(ref, 100, 4)
        refused("window", ref, 0, 0)
        assert eng.gc_bias(ref, 100, 4).tobytes() == good.tobytes()
        refused("window", ref, 1025, 4)
        refused("max_invalid", ref, 100, 100)
        refused("max_invalid", ref, 1, 1)
        out = _lib.cl_gc_bias()
        assert lib.cl_contig_gc_bias(h, None, 5, 100, 4, C.byref(out)) == -1 and b"null reference" in lib.cl_last_error(h)
        assert lib.cl_contig_gc_bias(h, ref.ctypes.data, ref.size, 100, 4, None) == -1 and b"null result" in lib.cl_last_error(h)
        assert lib.cl_contig_gc_bias(h, None, 0, 100, 4, C.byref(out)) == 0 and out.n_skipped == L
        assert eng.gc_bias(ref, 100, 4).tobytes() == good.tobytes()
        eng.contig_collect()
        assert eng.gc_bias(ref, 100, 4).tobytes() == good.tobytes()
    monkeypatch.setenv("DUT_QUAL_FORM", "bytes")
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, L, cref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        with pytest.raises(EngineError) as e:
            eng.gc_bias(ref, 100, 4)
        assert e.value.status == -1 and "pass-bit form only" in str(e.value)


# ---- 8. from files ----
def test_gc_files_one_device_several_contexts_and_the_tool(tmp_path):
    names = ["chr1", "chrM"]
    lens = [9000, 5000]
    recs = {0: synth.short_read_contig(lens[0], 20, 900, read_len=100), 1: synth.adversarial_contig(lens[1], 400, 901, overhang=True)}
    refs = [designed_ref(lens[0], 11), designed_ref(lens[1], 12)]
    bam = str(tmp_path / "m.bam"); fa = str(tmp_path / "m.fa")
    write_bam(bam, list(zip(names, lens)), recs, block_every=300)
    write_fasta(fa, list(zip(names, refs)))
    contigs = [(n, t, lens[t], refs[t], recs[t]) for t, n in enumerate(names)]
    o_res, o_bed = oracle_run(contigs, make_options({}), str(tmp_path / "o.bed"), dump=True)
    W, K = 50, 3
    exp = []
    for name, _, length, ref, _ in contigs:
        ro, qo, _, _, eo = o_res[name]["dumps"]
        ext = max(eo, length)
        exp.append((name, gc_ref.profile(depth_ref.pad(ro, ext), depth_ref.pad(qo, ext), ref, W, K)))
    assert exp[1][1]["extent"] > lens[1]                            # the second contig's reads overhang: ref_len < extent
    texts = dict(b=gc_ref.bias_text(exp), s=gc_ref.summary_text(exp))
    tols = dict(b=gc_ref.BIAS_TOL, s=gc_ref.SUMMARY_TOL)
    plain = tmp_path / "plain"; plain.mkdir()
    coverage_files(bam, fa, str(plain / "g.bed"), str(plain / "s.json"), CallableOptions())
    assert open(plain / "g.bed").read() == o_bed
    first = {}
    for devs in (None, [0, 0]):
        d = tmp_path / ("dev%d" % len(devs or [0])); d.mkdir()
        coverage_files(bam, fa, str(d / "g.bed"), str(d / "s.json"), CallableOptions(), devices=devs, gc_bias=str(d / "b.tsv"),
                       gc_summary=str(d / "s.tsv"), gc_window=W, gc_max_invalid=K)
        for k in "bs":
            got = open(d / f"{k}.tsv").read()
            gc_ref.same_text(got, texts[k], tols[k], (devs, k))
            assert first.setdefault(k, got) == got, (devs, k)      # one device and two contexts: the same bytes
        assert open(d / "g.bed").read() == o_bed
        a, b = json.load(open(plain / "s.json")), json.load(open(d / "s.json"))
        a["files"] = b["files"] = None                              # (the paths differ)
        assert a == b
    assert "\ntotal\t" in first["b"] and first["s"].count("\n") == 4
    # through the tool (it writes ./summary.json), with the other families' flags, and the same run without any
    for sub, extra in (("cli", ["--gc-bias", "b.tsv", "--gc-summary", "s.tsv", "--gc-window", str(W), "--gc-max-n", str(K),
                               "--depth-summary", "ds.tsv", "--depth-bed", "p.bed", "--devices", "0,0"]),
                       ("cli0", ["--depth-summary", "ds.tsv", "--depth-bed", "p.bed"]), ("cli00", [])):
        d = tmp_path / sub; d.mkdir()
        r = subprocess.run([_b.CLI, "coverage", bam, "-r", fa, "-o", "g.bed", "-s", "r.html"] + extra, cwd=str(d), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    for k in "bs":
        assert open(tmp_path / "cli" / f"{k}.tsv").read() == first[k]
    for f in ("g.bed", "summary.json", "r.html", "ds.tsv", "p.bed"):
        assert open(tmp_path / "cli0" / f).read() == open(tmp_path / "cli" / f).read(), f
    for f in ("g.bed", "summary.json", "r.html"):
        assert open(tmp_path / "cli00" / f).read() == open(tmp_path / "cli" / f).read(), f
    assert open(tmp_path / "cli00" / "g.bed").read() == o_bed and not (tmp_path / "cli00" / "b.tsv").exists()
    # only one of the files, the defaults W = 100 and K = 4
    d = tmp_path / "only"; d.mkdir()
    coverage_files(bam, fa, str(d / "g.bed"), None, CallableOptions(), gc_summary=str(d / "s.tsv"))
    line = open(d / "s.tsv").read().split("\n")[1].split("\t")
    assert line[:3] == ["chr1", "100", "4"] and sorted(p for p in os.listdir(d) if p.endswith(".tsv")) == ["s.tsv"]
