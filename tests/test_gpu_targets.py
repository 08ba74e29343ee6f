"""Per-target summaries on the device (-m gpu): cl_contig_targets against tests/targets_ref.py applied to the CPU oracle's
per-position raw_depth / qc_depth / state, and to the engine's own cl_debug_depths.  Counts: everything is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import depth_contigs
import depth_ref
import targets_ref
from bamio import write_bam, write_fasta
from helpers import contig_inputs, load_kats, make_options, oracle_run
from decodingustools_amd import (CallableOptions, CallableProfiler, ContigProfiler, Engine, EngineError, build as _b,
                                 process_single_contig, synth, write_target_stats, TargetStats)
from decodingustools_amd.bam import coverage_files
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu
KATS = load_kats()
T = 2048
DEFAULT_THR = (1, 10, 20, 30)
EIGHT = (1, 2, 3, 5, 8, 13, 21, 4_000_000_000)      # the last one lies above every depth
THRESHOLDS = ((), (1,), DEFAULT_THR, EIGHT)


def _opts(d):
    o = make_options(d)
    return CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                           o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def target_sets(extent, extra=()):
    """(label, starts, ends): what the issue lists, for a contig of `extent` positions (targets beyond it are clipped)"""
    E = extent
    rng = np.random.default_rng(1234 + E)
    sets = [("edges", [0, 0, 0, max(E - 1, 0), E, 5], [0, 1, E, E, E + 5, E + 100]),
            ("seams", [2047, 2048, 2047], [2049, 4096, 2048]),
            ("one thread's block", [32 + i for i in range(16)], [33 + i for i in range(16)]),
            ("two blocks", [40 + i for i in range(17)], [41 + i for i in range(17)]),
            ("a full window", list(range(2048)), list(range(1, 2049))),
            ("the second window, full", list(range(2048, 4096)), list(range(2049, 4097))),
            ("points in one window only", [100, 150], [200, 151])]
    # nested, overlapping and duplicate targets in shuffled order
    s = [10, 10, 10, 20, 20, 0, 300, 300, 2000, 2000, 1, 4000, 4000]
    e = [500, 500, 11, 30, 3000, E, 301, 2100, 2100, 6000, E + 7, 4001, 4000]
    order = rng.permutation(len(s))
    sets.append(("nested", [s[i] for i in order], [e[i] for i in order]))
    a = rng.integers(0, E + 50, 5000)
    b = a + np.where(rng.random(5000) < 0.7, rng.integers(0, 400, 5000), rng.integers(0, E + 50, 5000))
    sets.append(("random", a.tolist(), b.tolist()))
    return sets + list(extra)


def union(sets, seed=7):
    s = np.concatenate([np.asarray(x[1], np.int64) for x in sets])
    e = np.concatenate([np.asarray(x[2], np.int64) for x in sets])
    order = np.random.default_rng(seed).permutation(len(s))
    return s[order], e[order]


def same_bytes(a: TargetStats, b: TargetStats):
    return a.records().tobytes() == b.records().tobytes()


def check(contigs, opt_dict, tmp_path, o_res=None, thresholds=THRESHOLDS, extra_sets=(), sets_of=target_sets):
    """every contig through the product path on one engine; while it is resident: every target set with the default
    thresholds and their union with every threshold set, against the oracle's arrays and the engine's own dump; the
    invariants against the summary and the depth profile; the call repeated; the run repeated."""
    opt = _opts(opt_dict)
    if o_res is None:
        o_res, _ = oracle_run(contigs, make_options(opt_dict), str(tmp_path / "o.bed"), dump=True)
    with Engine(opt, 0) as eng:
        counter = CallableProfiler(str(tmp_path / "g.bed"))
        for name, tid, length, ref, rec in contigs:
            process_single_contig(eng, counter, ContigProfiler(name, length), opt, tid, rec, ref)
            before = eng.contig_collect()
            s = before.summary
            extent = int(s.extent)
            ro, qo, _, so, eo = o_res[name]["dumps"]
            assert extent == max(eo, length)
            d_raw, d_qc, _, d_state = eng.debug_depths(extent)
            o_raw, o_qc = depth_ref.pad(ro, extent), depth_ref.pad(qo, extent)
            # the oracle's states end at its last column: behind it the engine's own, held against the oracle's counts
            o_state = np.concatenate((np.asarray(so, np.uint8), np.asarray(d_state[eo:extent], np.uint8)))
            assert np.array_equal(o_state[:eo], d_state[:eo])
            assert np.bincount(o_state, minlength=6).tolist() == [int(v) for v in o_res[name]["state_counts"]]
            sets = sets_of(extent, extra_sets) if sets_of is target_sets else sets_of(extent)
            calls = [(lab, np.asarray(a, np.int64), np.asarray(b, np.int64), DEFAULT_THR) for lab, a, b in sets]
            ua, ub = union(sets)
            calls += [("union", ua, ub, thr) for thr in thresholds]
            for lab, a, b, thr in calls:
                got = eng.target_stats(a, b, thr)
                what = (name, lab, thr)
                targets_ref.same(got, targets_ref.target_stats(o_raw, o_qc, o_state, a, b, thr), what + ("oracle",))
                targets_ref.same(got, targets_ref.target_stats(d_raw, d_qc, d_state, a, b, thr), what + ("debug_depths",))
                assert np.array_equal(got.state.sum(axis=1), got.len), what
                assert same_bytes(got, eng.target_stats(a, b, thr)), what
            # the whole contig as one target: what ties it to the contig's summary and to the depth profile
            whole = eng.target_stats([0], [extent], EIGHT)
            assert int(whole.len[0]) == extent
            assert int(whole.sum_raw[0]) == s.summed_coverage and int(whole.sum_qc[0]) == s.quality_bases
            assert whole.state[0].tolist() == [int(v) for v in s.state_counts]
            assert extent - int(whole.ge_raw[0, 0]) == extent - s.n_covered_bases
            p = eng.depth_profile(4096, 0)
            for k, t in enumerate(EIGHT):
                if t <= 4095:                                   # (the last bin is "4095 or more": its tail sum is exact too)
                    assert int(whole.ge_raw[0, k]) == int(p.hist_raw[t:].sum()), (name, t)
                    assert int(whole.ge_qc[0, k]) == int(p.hist_qc[t:].sum()), (name, t)
                else:
                    assert int(whole.ge_raw[0, k]) == 0 and int(whole.ge_qc[0, k]) == 0
            # interleaved with the siblings, and the run repeated: the same summary and intervals as before
            eng.depth_runs("qc")
            assert same_bytes(whole, eng.target_stats([0], [extent], EIGHT))
            eng.contig_run()
            with pytest.raises(EngineError) as err:                # run, not collected: the intervals are not settled
                eng.target_stats([0], [extent])
            assert err.value.status == -1 and "collected" in str(err.value)
            after = eng.contig_collect()
            assert after.as_dict() == before.as_dict()
            assert np.array_equal(np.asarray(after.intervals), np.asarray(before.intervals))
            assert same_bytes(whole, eng.target_stats([0], [extent], EIGHT))
        counter.close()


@pytest.mark.parametrize("case", KATS["cases"], ids=[c["name"] for c in KATS["cases"]])
def test_kats(case, tmp_path):
    opt = {**KATS["default_options"], **case.get("options", {})}
    contigs = []
    for i, c in enumerate(case["contigs"]):
        rec, ref = contig_inputs(c)
        contigs.append((c["name"], c.get("tid", i), c["len"], ref, rec))
    check(contigs, opt, tmp_path, thresholds=(DEFAULT_THR,))


@pytest.mark.parametrize("L", [1, 300, 2048, 2049, 4096, 6143])
@pytest.mark.parametrize("deep,overhang", [(False, False), (True, False), (False, True), (True, True)])
def test_adversarial_contigs(L, deep, overhang, tmp_path):
    n = {1: 5, 300: 2000, 2048: 500, 2049: 500, 4096: 900, 6143: 700}[L]
    rec = synth.adversarial_contig(L, n, 2000 + L, max_len=min(300, max(2, L)), deep=deep, overhang=overhang)
    ref = synth.make_reference(L, 60 + L % 7, lowercase=(L % 2 == 0))
    thr = THRESHOLDS + (((255, 256), (32767, 32768)) if deep else ())
    check([("chrA", L % 3, L, ref, rec)], dict(min_depth=2, min_depth_for_low_mapq=3), tmp_path, thresholds=thr)


@pytest.mark.parametrize("depth,planes", [(300, 16), (66_000, 32)])
def test_deep_piles_select_the_16_and_32_plane_kernels(depth, planes, tmp_path):
    contig, o_res, _, _ = depth_contigs.deep_pile(depth)
    _, tid, L, ref, rec = contig
    check([contig], depth_contigs.DEEP_OPTIONS, tmp_path, o_res=o_res, thresholds=(DEFAULT_THR, (255, 256), (32767, 32768), (65_999, 66_000, 66_001)))
    with Engine(_opts(depth_contigs.DEEP_OPTIONS), 0) as eng:
        eng.contig_begin(tid, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        assert eng.contig_layout()["counter_planes"] == planes


def test_past_one_scan_step_and_the_grid(tmp_path):
    """3078 windows: four steps of k_target_scan, and workgroups 0..1029 of k_target_depth take two windows.  Targets
    across the step boundaries, at them, and a window with points between many without."""
    contig, o_res, extent, depths = depth_contigs.scan_steps()
    assert extent == depth_contigs.SCAN_L and -(-extent // T) == 2048 + 1030

    def sets(E):
        out = [("edges", [0, 0, E - 1, E, 5], [0, E, E, E + 5, E + 100])]
        s, e = [], []
        for B in depth_contigs.SCAN_B + (2048 * T,):
            s += [B - 700, B - 1, B, B - 1, B - T, B + 3, B - 600, 0, B]
            e += [B + 700, B + 1, B + 1, B, B + T, B + 3 * T + 5, B + 100, B, E]
        out.append(("boundaries", s, e))
        out.append(("one window in the middle", [1500 * T + 5, 1500 * T + 7], [1500 * T + 900, 1500 * T + 8]))
        rng = np.random.default_rng(99)
        a = rng.integers(0, E, 5000)
        out.append(("random", a.tolist(), (a + rng.integers(0, 300_000, 5000)).tolist()))
        return out
    check([contig], {}, tmp_path, o_res=o_res, thresholds=(DEFAULT_THR,), sets_of=sets)


def test_empty_contigs_and_no_targets(tmp_path):
    check([("e1", 0, 0, None, ContigRecords.empty()), ("e2", 1, 5000, None, ContigRecords.empty()),
           ("e3", 2, 4096, synth.make_reference(4096, 3), ContigRecords.empty())], dict(), tmp_path, thresholds=(DEFAULT_THR,))
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, 5000, None)
        eng.contig_finish()
        r = eng.target_stats([], [])
        assert r.len.shape == (0,) and r.state.shape == (0, 6) and r.ge_raw.shape == (0, 4)
        r = eng.target_stats([7, 5000, 9000], [7, 5001, 9001], ())
        assert r.len.tolist() == [0, 0, 0] and r.start.tolist() == [7, 5000, 5000] and r.end.tolist() == [7, 5000, 5000]
        assert not r.state.any() and r.ge_raw.shape == (3, 0)


def test_refusals(monkeypatch):
    L = 3000
    rec = synth.short_read_contig(L, 10, 5)
    ref = synth.make_reference(L, 6)
    with Engine(CallableOptions(), 0) as eng:
        def refused(text, starts=(0,), ends=(10,), thr=DEFAULT_THR):
            with pytest.raises(EngineError) as e:
                eng.target_stats(starts, ends, thr)
            assert e.value.status == -1 and text in str(e.value), str(e.value)

        def good():
            r = eng.target_stats([0, 5], [L, 6])
            assert int(r.sum_raw[0]) == s.summed_coverage and int(r.len[1]) == 1
        refused("collected")                                       # nothing resident
        eng.contig_begin(0, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        refused("collected")                                       # begun
        eng.contig_upload()
        refused("collected")                                       # uploaded
        eng.contig_run()
        refused("collected")                                       # run, not collected
        s = eng.contig_collect().summary
        good()
        for text, kw in (("start > end", dict(starts=(3, 9), ends=(5, 8))),
                         ("more than 8 thresholds", dict(thr=tuple(range(1, 10)))),
                         ("strictly ascending", dict(thr=(1, 5, 5))),
                         ("strictly ascending", dict(thr=(10, 5))),
                         ("first threshold is 0", dict(thr=(0, 5)))):
            refused(text, **kw)
            good()
        # the ABI's own refusals: null result, null arrays with n > 0, too many targets
        import ctypes as C
        from decodingustools_amd import _lib
        lib, h = eng._lib, eng._h
        out = C.POINTER(_lib.cl_target_stats)()
        one = (C.c_uint32 * 1)(0)
        thr = (C.c_uint32 * 1)(1)
        for args, text in (((one, one, 1, thr, 1, None), "null result"),
                           ((None, one, 1, thr, 1, C.byref(out)), "null starts or ends"),
                           ((one, None, 1, thr, 1, C.byref(out)), "null starts or ends"),
                           ((one, one, 1, None, 1, C.byref(out)), "null thresholds"),
                           ((one, one, (1 << 24) + 1, thr, 1, C.byref(out)), "2^24")):
            assert lib.cl_contig_targets(h, *args) == -1
            assert text in lib.cl_last_error(h).decode()
            good()
        assert lib.cl_contig_targets(h, None, None, 0, None, 0, C.byref(out)) == 0 and not out
    monkeypatch.setenv("DUT_QUAL_FORM", "bytes")
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        with pytest.raises(EngineError) as e:
            eng.target_stats([0], [10])
        assert e.value.status == -1 and "pass-bit form only" in str(e.value)


def test_target_files_devices_flags_and_the_tool(tmp_path):
    names = ["chr1", "chr2"]
    lens = [30_000, 9_000]
    # (a last read that overhangs the contig's end: the oracle's per-position states then cover the whole contig)
    tails = [ContigRecords.from_reads([(l - 50, "100M", 60, 30, 0, f"tail{i}")]) for i, l in enumerate(lens)]
    recs = {0: depth_contigs.merge(synth.short_read_contig(lens[0], 25, 910), tails[0]),
            1: depth_contigs.merge(synth.adversarial_contig(lens[1], 1500, 911, deep=True), tails[1])}
    refs = [synth.make_reference(l, 960 + i, lowercase=(i == 1)) for i, l in enumerate(lens)]
    bam = str(tmp_path / "m.bam"); fa = str(tmp_path / "m.fa")
    write_bam(bam, list(zip(names, lens)), recs, block_every=800)
    write_fasta(fa, list(zip(names, refs)))
    contigs = [(n, t, lens[t], refs[t], recs[t]) for t, n in enumerate(names)]
    o_res, o_bed = oracle_run(contigs, make_options({}), str(tmp_path / "o.bed"), dump=True)
    # the regions: chr2 first in the file (the table follows the BED output's order, chr1 first), overlapping, one beyond the end
    regions = [("chr2", 100, 900, "b1"), ("chr1", 0, 2048, "a1"), ("chr1", 2047, 2049, None), ("chr2", 8_000, 20_000, "b2"),
               ("chr1", 29_000, 31_000, "a3"), ("chr1", 500, 700, "a4"), ("chr2", 50_000, 50_010, "beyond"), ("chr1", 600, 600, "empty")]
    bed = str(tmp_path / "t.bed")
    with open(bed, "w") as f:
        f.write("track name=t\n# a comment\n")
        for c, s, e, nm in regions:
            f.write("\t".join([c, str(s), str(e)] + ([nm] if nm else [])) + "\n")
    thr = (1, 10, 25)

    def expected(which):
        out = []
        for name, _, length, _, _ in contigs:
            if name not in which:
                continue
            ro, qo, _, so, eo = o_res[name]["dumps"]
            assert eo >= length                                     # (these contigs: the oracle walks all of them)
            mine = [r for r in regions if r[0] == name]
            st = targets_ref.target_stats(ro, qo, so, [r[1] for r in mine], [r[2] for r in mine], thr)
            out.append((name, st, [r[3] or "." for r in mine]))
        return targets_ref.table_text(out, thr), out
    text_all, exp_all = expected(names)
    text_1, _ = expected(["chr1"])
    assert "\tNA\tNA\t" in text_all and text_all.splitlines()[-1].startswith("total\t.\t.\t.\t")
    # write_target_stats of the reference gives the same text
    ref_path = str(tmp_path / "ref.tsv")
    write_target_stats(ref_path, [(n, TargetStats(thresholds=np.asarray(thr, np.uint32), **{k: st[k] for k in targets_ref.FIELDS}), nm)
                                  for n, st, nm in exp_all], thr)
    assert open(ref_path).read() == text_all

    plain = tmp_path / "plain"; plain.mkdir()
    coverage_files(bam, fa, str(plain / "g.bed"), str(plain / "s.json"), CallableOptions())
    assert open(plain / "g.bed").read() == o_bed

    def same_json(a, b):
        a, b = json.load(open(a)), json.load(open(b))
        a["files"] = b["files"] = None                              # (the paths differ)
        return a == b
    for devs in (None, [0, 0]):
        d = tmp_path / ("dev%d" % len(devs or [0])); d.mkdir()
        coverage_files(bam, fa, str(d / "g.bed"), str(d / "s.json"), CallableOptions(), devices=devs, targets=bed, target_out=str(d / "t.tsv"),
                       target_thresholds=thr)
        assert open(d / "t.tsv").read() == text_all, devs
        assert open(d / "g.bed").read() == o_bed and same_json(plain / "s.json", d / "s.json"), devs
    # a selection that leaves chr2 out: its targets are skipped
    d = tmp_path / "sel"; d.mkdir()
    coverage_files(bam, fa, str(d / "g.bed"), None, CallableOptions(), contigs=["chr1"], targets=bed, target_out=str(d / "t.tsv"), target_thresholds=thr)
    assert open(d / "t.tsv").read() == text_1
    # together with the depth summary and the depth BED: every file as the single flags give it
    single = tmp_path / "single"; single.mkdir()
    coverage_files(bam, fa, str(single / "g.bed"), None, CallableOptions(), depth_summary=str(single / "s.tsv"), depth_cap=40)
    coverage_files(bam, fa, str(single / "g2.bed"), None, CallableOptions(), depth_bed=str(single / "d.bed"), quantize="1:10")
    d = tmp_path / "all"; d.mkdir()
    coverage_files(bam, fa, str(d / "g.bed"), str(d / "s.json"), CallableOptions(), devices=[0, 0], depth_summary=str(d / "s.tsv"), depth_cap=40,
                   depth_bed=str(d / "d.bed"), quantize="1:10", targets=bed, target_out=str(d / "t.tsv"), target_thresholds=thr)
    assert open(d / "t.tsv").read() == text_all and open(d / "g.bed").read() == o_bed
    assert open(d / "s.tsv").read() == open(single / "s.tsv").read() and open(d / "d.bed").read() == open(single / "d.bed").read()
    # through the tool (it writes ./summary.json): with the flags, without them, and a target on a contig the BAM lacks
    for sub, extra in (("cli", ["--targets", bed, "--target-out", "t.tsv", "--target-thresholds", "1,10,25"]), ("cli0", [])):
        d = tmp_path / sub; d.mkdir()
        r = subprocess.run([_b.CLI, "coverage", bam, "-r", fa, "-o", "g.bed", "-s", "r.html"] + extra, cwd=str(d), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert open(tmp_path / "cli" / "t.tsv").read() == text_all
    assert open(tmp_path / "cli0" / "g.bed").read() == open(tmp_path / "cli" / "g.bed").read() == o_bed
    assert open(tmp_path / "cli0" / "summary.json").read() == open(tmp_path / "cli" / "summary.json").read()
    assert same_json(tmp_path / "cli0" / "summary.json", plain / "s.json")
    assert not (tmp_path / "cli0" / "t.tsv").exists()
    unknown = str(tmp_path / "u.bed")
    with open(unknown, "w") as f:
        f.write("chr1\t0\t10\nchrZ\t5\t9\n")
    d = tmp_path / "cliu"; d.mkdir()
    r = subprocess.run([_b.CLI, "coverage", bam, "-r", fa, "-o", "g.bed", "--targets", unknown, "--target-out", "t.tsv"], cwd=str(d),
                       capture_output=True, text=True)
    assert r.returncode == 1 and "line 2" in r.stderr and "chrZ" in r.stderr, r.stderr
