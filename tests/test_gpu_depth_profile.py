"""The depth profile on the device (-m gpu): cl_contig_depth_profile against tests/depth_ref.py applied to the CPU
oracle's per-position raw_depth / qc_depth, and to the engine's own cl_debug_depths.  Counts: everything is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import depth_contigs
import depth_ref
from bamio import write_bam, write_fasta
from helpers import contig_inputs, load_kats, make_options, oracle_run
from decodingustools_amd import (CallableOptions, CallableProfiler, ContigProfiler, Engine, EngineError, build as _b,
                                 depth_stats, process_single_contig, synth)
from decodingustools_amd.bam import coverage_files
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu
KATS = load_kats()
N_BINS = (2, 17, 1001, 4096)                       # 2 and 17 force saturation


def windows_for(extent):
    return (0, 16, 100, 500, 2048, 2049, 5000, extent + 1)


def _opts(d):
    o = make_options(d)
    return CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                           o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def same_profile(got, exp, what):
    assert (got.n_bins, got.window, got.n_windows, got.extent) == (exp["n_bins"], exp["window"], exp["n_windows"], exp["extent"]), what
    assert (got.sum_raw, got.sum_qc) == (exp["sum_raw"], exp["sum_qc"]), what
    assert np.array_equal(got.hist_raw, exp["hist_raw"]), (what, "hist_raw")
    assert np.array_equal(got.hist_qc, exp["hist_qc"]), (what, "hist_qc")
    if exp["window"]:
        assert np.array_equal(got.win_raw, exp["win_raw"]), (what, "win_raw")
        assert np.array_equal(got.win_qc, exp["win_qc"]), (what, "win_qc")
    else:
        assert got.win_raw is None and got.win_qc is None


def check(contigs, opt_dict, tmp_path, n_bins=N_BINS, windows=None, o_res=None):
    """every contig through the product path on one engine; while it is resident: the profile for every (n_bins, S)
    against the oracle's depths and the engine's own dump, the invariants against the summary, and the run repeated.
    o_res: what oracle_run gave for these contigs and options, where a case has it already."""
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
            ro, qo, _, _, eo = o_res[name]["dumps"]
            assert extent == max(eo, length)
            o_raw, o_qc = depth_ref.pad(ro, extent), depth_ref.pad(qo, extent)
            d_raw, d_qc, _, _ = eng.debug_depths(extent)
            for nb in n_bins:
                for S in (windows or windows_for(extent)):
                    if 0 < S < 16:                                  # extent + 1 of a tiny contig: the contract refuses it
                        with pytest.raises(EngineError) as e:
                            eng.depth_profile(nb, S)
                        assert e.value.status == -1
                        continue
                    got = eng.depth_profile(nb, S)
                    same_profile(got, depth_ref.profile(o_raw, o_qc, nb, S), (name, nb, S, "oracle"))
                    same_profile(got, depth_ref.profile(d_raw, d_qc, nb, S), (name, nb, S, "debug_depths"))
                    # what ties it to the contig's summary
                    assert int(got.hist_raw.sum()) == int(got.hist_qc.sum()) == extent
                    assert extent - int(got.hist_raw[0]) == s.n_covered_bases
                    assert got.sum_raw == s.summed_coverage and got.sum_qc == s.quality_bases
                    if S:
                        assert int(got.win_raw.sum()) == got.sum_raw and int(got.win_qc.sum()) == got.sum_qc
                    if got.hist_raw[-1] == 0:
                        assert int((got.hist_raw * np.arange(nb, dtype=np.uint64)).sum()) == got.sum_raw
                    if got.hist_qc[-1] == 0:
                        assert int((got.hist_qc * np.arange(nb, dtype=np.uint64)).sum()) == got.sum_qc
            # the profile left the run's results alone, and the contig runs again as before
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
    L = [777, 2048, 2049, 4096, 5000, 6143, 1, 300][seed]
    n = [200, 500, 500, 900, 1200, 700, 5, 2000][seed]
    rec = synth.adversarial_contig(L, n, 1000 + seed, max_len=min(300, max(2, L)), deep=(seed in (3, 7)), overhang=(seed in (1, 4, 6)))
    ref = synth.make_reference(L, 50 + seed, lowercase=(seed % 2 == 0))
    check([("chrA", seed % 3, L, ref, rec)], dict(min_depth=2, min_depth_for_low_mapq=3), tmp_path)


def test_short_reads_2mb_30x(tmp_path):
    L = 2_000_000
    rec = synth.short_read_contig(L, 30, synth.seed_for(2, 20))
    check([("chr21", 20, L, synth.make_reference(L, synth.seed_for(2, 20)), rec)], dict(), tmp_path)


def test_two_windows_per_workgroup(tmp_path):
    """3078 windows on a grid of 2048: workgroups 0..1029 of k_depth_profile take windows w and w + 2048, with both in
    their LDS histograms and register sums, and with another first window slot (kW) per trip"""
    contig, o_res, extent, depths = depth_contigs.scan_steps()
    T, B2 = depth_contigs.T, depth_contigs.SCAN_B[1]
    assert extent == depth_contigs.SCAN_L and -(-extent // T) == 2048 + 1030
    # from the reference alone: most of these workgroups see depth of both kinds in both of their windows, and other
    # depths in the second than in the first
    for kind in ("raw", "qc"):
        first = depths[kind][:1030 * T].reshape(1030, T)
        second = depth_ref.pad(depths[kind][B2:], 1030 * T).reshape(1030, T)
        assert int((first.any(axis=1) & second.any(axis=1)).sum()) > 900, kind
        assert int((first.sum(axis=1) != second.sum(axis=1)).sum()) > 900, kind
    check([contig], {}, tmp_path, n_bins=(17, 1001), windows=(0, 16, 2049, 100_000), o_res=o_res)


def test_windows_that_only_the_wide_list_covers(tmp_path):
    contig, o_res, extent, depths = depth_contigs.wide_list()
    assert extent == depth_contigs.WIDE_L
    depth_contigs.assert_wide_only_windows(contig[4], depths)
    check([contig], depth_contigs.WIDE_OPTIONS, tmp_path, o_res=o_res)


def test_long_reads_indel_rich(tmp_path):
    L = 300_000
    rec = synth.long_read_contig(L, 50, synth.seed_for(3, 23))
    check([("chrY", 23, L, synth.make_reference(L, synth.seed_for(3, 23)), rec)], dict(), tmp_path)


@pytest.mark.parametrize("depth,planes", [(300, 16), (66_000, 32)])
def test_deep_piles_select_the_16_and_32_plane_kernels(depth, planes, tmp_path):
    contig, o_res, _, _ = depth_contigs.deep_pile(depth)
    _, tid, L, ref, rec = contig
    check([contig], depth_contigs.DEEP_OPTIONS, tmp_path, o_res=o_res)
    with Engine(_opts(depth_contigs.DEEP_OPTIONS), 0) as eng:
        eng.contig_begin(tid, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        s = eng.contig_finish().summary
        assert eng.contig_layout()["counter_planes"] == planes
        p = eng.depth_profile(4096, 0)
        assert p.sum_raw == s.summed_coverage and (p.hist_raw[-1] > 0) == (s.max_raw_depth >= 4095)


def test_candidates_beyond_32767_in_a_window(tmp_path):
    """the 32-bit difference words of the classifier's DEEP form: here every window has them"""
    L = 5000
    rng = np.random.default_rng(5)
    reads = [(int(p), "30M", 60, 30, 0, f"r{i}") for i, p in enumerate(np.sort(rng.integers(100, 1900, 40_000)))]
    check([("chrP", 0, L, synth.make_reference(L, 9), ContigRecords.from_reads(reads))], dict(max_depth=1_000_000), tmp_path)


@pytest.mark.parametrize("head_span", ["37", "1000"])
def test_spans_cut_into_several_heads(head_span, tmp_path, monkeypatch):
    monkeypatch.setenv("DUT_HEAD_SPAN", head_span)
    rec = synth.long_read_contig(60_000, 8, 17)
    check([("chrL", 2, 60_000, synth.make_reference(60_000, 3), rec)], None, tmp_path)


def test_empty_contigs(tmp_path):
    check([("e1", 0, 0, None, ContigRecords.empty()), ("e2", 1, 5000, None, ContigRecords.empty()),
           ("e3", 2, 4096, synth.make_reference(4096, 3), ContigRecords.empty())], dict(), tmp_path)
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, 5000, None)
        eng.contig_finish()
        p = eng.depth_profile(10, 16)
        assert p.hist_raw[0] == p.hist_qc[0] == 5000 and p.sum_raw == 0 and p.n_windows == 313 and not p.win_raw.any()
        eng.contig_begin(1, 0, None)
        eng.contig_finish()
        p = eng.depth_profile(10, 16)
        assert p.extent == 0 and p.n_windows == 0 and not p.hist_raw.any() and p.win_raw.shape == (0,)


def test_refusals(monkeypatch):
    L = 3000
    rec = synth.short_read_contig(L, 10, 5)
    ref = synth.make_reference(L, 6)
    with Engine(CallableOptions(), 0) as eng:
        def refused(nb, S, text):
            with pytest.raises(EngineError) as e:
                eng.depth_profile(nb, S)
            assert e.value.status == -1 and text in str(e.value), str(e.value)
        refused(1001, 500, "has been run")                         # nothing resident
        eng.contig_begin(0, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        refused(1001, 500, "has been run")                         # begun, not run
        eng.contig_upload()
        refused(1001, 500, "has been run")                         # uploaded, not run
        eng.contig_run()
        s = eng.contig_collect().summary
        refused(1, 0, "n_bins")
        refused(4097, 0, "n_bins")
        refused(1001, 7, "window")
        refused(1001, 15, "window")
        assert eng.depth_profile(1001, 16).sum_raw == s.summed_coverage
    monkeypatch.setenv("DUT_QUAL_FORM", "bytes")
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        with pytest.raises(EngineError) as e:
            eng.depth_profile(1001, 500)
        assert e.value.status == -1 and "pass-bit form only" in str(e.value)


def test_depth_files_one_device_several_contexts_and_the_tool(tmp_path):
    names = ["chr1", "chr2", "chr3", "chrX", "chrM"]
    lens = [150_000, 60_000, 90_000, 30_000, 16_569]
    recs = {0: synth.short_read_contig(lens[0], 30, 900), 1: synth.adversarial_contig(lens[1], 3000, 901, deep=True),
            2: synth.long_read_contig(lens[2], 20, 902), 4: synth.short_read_contig(lens[4], 20, 905)}
    refs = [synth.make_reference(l, 950 + i, lowercase=(i == 4)) for i, l in enumerate(lens)]
    bam = str(tmp_path / "m.bam"); fa = str(tmp_path / "m.fa")
    write_bam(bam, list(zip(names, lens)), recs, block_every=800)
    write_fasta(fa, list(zip(names, refs)))
    contigs = [(n, t, lens[t], refs[t], recs.get(t, ContigRecords.empty())) for t, n in enumerate(names)]
    o_res, o_bed = oracle_run(contigs, make_options({}), str(tmp_path / "o.bed"), dump=True)
    cap, S = 40, 500                                               # a cap that saturates in the 30x contig
    exp = []
    for name, _, length, _, _ in contigs:
        ro, qo, _, _, eo = o_res[name]["dumps"]
        ext = max(eo, length)
        exp.append((name, depth_ref.profile(depth_ref.pad(ro, ext), depth_ref.pad(qo, ext), cap + 1, S)))
    texts = dict(d=depth_ref.dist_text(exp), w=depth_ref.windows_text(exp), s=depth_ref.summary_text(exp))
    assert "\t40+\t" in texts["d"]
    plain = tmp_path / "plain"; plain.mkdir()
    coverage_files(bam, fa, str(plain / "g.bed"), str(plain / "s.json"), CallableOptions())
    assert open(plain / "g.bed").read() == o_bed

    def same_outputs(d, how):
        for k in "dws":
            assert open(d / f"{k}.tsv").read() == texts[k], (how, k)
        assert open(d / "g.bed").read() == o_bed, how
        a, b = json.load(open(plain / "s.json")), json.load(open(d / "s.json"))
        a["files"] = b["files"] = None                              # (the paths differ)
        assert a == b, how

    for devs in (None, [0, 0], [0, 0, 0]):
        d = tmp_path / ("dev%d" % len(devs or [0])); d.mkdir()
        coverage_files(bam, fa, str(d / "g.bed"), str(d / "s.json"), CallableOptions(), devices=devs, depth_dist=str(d / "d.tsv"),
                       depth_windows=str(d / "w.tsv"), depth_summary=str(d / "s.tsv"), depth_cap=cap, window=S)
        same_outputs(d, devs)
    # through the tool (it writes ./summary.json), and the same run without the flags
    for sub, extra in (("cli", ["--depth-dist", "d.tsv", "--depth-windows", "w.tsv", "--window", str(S), "--depth-summary", "s.tsv",
                               "--depth-cap", str(cap)]), ("cli0", [])):
        d = tmp_path / sub; d.mkdir()
        r = subprocess.run([_b.CLI, "coverage", bam, "-r", fa, "-o", "g.bed", "-s", "r.html"] + extra, cwd=str(d), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        os.rename(d / "summary.json", d / "s.json")
    same_outputs(tmp_path / "cli", "cli")
    assert open(tmp_path / "cli0" / "g.bed").read() == o_bed
    assert open(tmp_path / "cli0" / "s.json").read() == open(tmp_path / "cli" / "s.json").read()
    assert open(tmp_path / "cli0" / "r.html").read() == open(tmp_path / "cli" / "r.html").read()
    assert not (tmp_path / "cli0" / "d.tsv").exists()
    # only one of the files, no window table asked
    d = tmp_path / "only"; d.mkdir()
    coverage_files(bam, fa, str(d / "g.bed"), None, CallableOptions(), depth_summary=str(d / "s.tsv"), depth_cap=cap)
    assert open(d / "s.tsv").read() == texts["s"] and sorted(p for p in os.listdir(d) if p.endswith(".tsv")) == ["s.tsv"]
    # the summary's numbers are dut_depth_stats of the histograms
    st = depth_stats(exp[0][1]["hist_raw"], exp[0][1]["sum_raw"])
    assert 25 <= st["median"][0] <= 35 and st["frac_at_least"][50] is None
