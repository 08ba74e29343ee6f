"""Per-target order statistics on the device (-m gpu): cl_contig_target_order against tests/order_ref.py applied to the CPU
oracle's per-position raw_depth / qc_depth, and to the engine's own cl_debug_depths.  Whole numbers: everything is exact."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import depth_contigs
import depth_ref
import order_ref
import targets_ref
from bamio import write_bam, write_fasta
from helpers import contig_inputs, load_kats, make_options, oracle_run
from test_gpu_targets import target_sets, union
from decodingustools_amd import (CallableOptions, CallableProfiler, ContigProfiler, Engine, EngineError, TargetOrder, _lib, build as _b,
                                 depth_stats, process_single_contig, synth)
from decodingustools_amd.bam import coverage_files
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu
KATS = load_kats()
T = 2048
THR = (1, 10, 20, 30)


def _opts(d):
    o = make_options(d)
    return CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                           o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def same_bytes(a: TargetOrder, b: TargetOrder):
    return a.records().tobytes() == b.records().tobytes()


def invariants(got, what):
    for five in (got.raw, got.qc):
        assert (five[:, :-1] <= five[:, 1:]).all(), what             # min <= q1 <= median <= q3 <= max
    assert (got.qc <= got.raw).all(), what
    empty = got.len == 0
    assert not got.raw[empty].any() and not got.qc[empty].any(), what
    one = got.len == 1
    assert (got.raw[one] == got.raw[one][:, :1]).all() and (got.qc[one] == got.qc[one][:, :1]).all(), what


def check(contigs, opt_dict, tmp_path, o_res=None, sets_of=target_sets):
    """every contig through the product path on one engine; while it is resident: every target set and their union,
    against the oracle's arrays and the engine's own dump; the invariants, also against target_stats and the depth
    profile; the call repeated, behind its siblings, and behind a run that is not collected."""
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
            o_raw, o_qc = depth_ref.pad(ro, extent), depth_ref.pad(qo, extent)
            # (the engine's dump is the oracle's: one reference serves both; where it is not, each gets its own)
            dump_is_oracle = np.array_equal(np.asarray(d_raw, np.uint64), o_raw) and np.array_equal(np.asarray(d_qc, np.uint64), o_qc)
            assert dump_is_oracle, name
            rounds = int(o_raw.max()).bit_length() if extent else 0
            sets = sets_of(extent)
            ua, ub = union(sets)
            calls = [(lab, np.asarray(a, np.int64), np.asarray(b, np.int64)) for lab, a, b in sets] + [("union", ua, ub)]
            for lab, a, b in calls:
                got = eng.target_order(a, b)
                what = (name, lab)
                order_ref.same(got, order_ref.target_order(o_raw, o_qc, a, b), what)
                invariants(got, what)
                assert same_bytes(got, eng.target_order(a, b)), what
                # the bit rounds: the bit length of the largest raw depth of any target
                ca, cb = targets_ref.clip(a, b, extent)
                assert got.n_rounds == (int(got.raw[:, 4].max()).bit_length() if len(a) else 0), what
                if ((ca == 0) & (cb == extent)).any():
                    assert got.n_rounds == rounds, what
            # against the counts of cl_contig_targets: max >= t iff some position is, min >= t iff every position is
            got, st = eng.target_order(ua, ub), eng.target_stats(ua, ub, THR)
            live = got.len > 0
            for k, t in enumerate(THR):
                assert np.array_equal(got.raw[live, 4] >= t, st.ge_raw[live, k] > 0) and np.array_equal(got.raw[live, 0] >= t, st.ge_raw[live, k] == st.len[live])
                assert np.array_equal(got.qc[live, 4] >= t, st.ge_qc[live, k] > 0) and np.array_equal(got.qc[live, 0] >= t, st.ge_qc[live, k] == st.len[live])
            # the whole contig as one target: its quartiles are the depth profile's
            whole = eng.target_order([0], [extent])
            assert int(whole.len[0]) == extent
            if extent:
                p = eng.depth_profile(4096, 0)
                for five, hist, total in ((whole.raw[0], p.hist_raw, p.sum_raw), (whole.qc[0], p.hist_qc, p.sum_qc)):
                    ds = depth_stats(hist, total)
                    for j, q in ((1, "q1"), (2, "median"), (3, "q3")):
                        if not ds[q][1]:                            # (not in the histogram's last, saturating bin)
                            assert int(five[j]) == ds[q][0], (name, q)
                assert whole.n_rounds == rounds
            # interleaved with the siblings; and behind a run that has not been collected, where cl_contig_targets refuses
            eng.depth_runs("qc")
            assert same_bytes(whole, eng.target_order([0], [extent]))
            eng.target_stats([0], [extent])
            assert same_bytes(whole, eng.target_order([0], [extent]))
            eng.contig_run()
            with pytest.raises(EngineError) as err:
                eng.target_stats([0], [extent])
            assert err.value.status == -1 and "collected" in str(err.value)
            assert same_bytes(whole, eng.target_order([0], [extent]))
            assert same_bytes(got, eng.target_order(ua, ub))
            after = eng.contig_collect()
            assert after.as_dict() == before.as_dict()
            assert np.array_equal(np.asarray(after.intervals), np.asarray(before.intervals))
            assert same_bytes(whole, eng.target_order([0], [extent]))
        counter.close()


@pytest.mark.parametrize("case", KATS["cases"], ids=[c["name"] for c in KATS["cases"]])
def test_kats(case, tmp_path):
    opt = {**KATS["default_options"], **case.get("options", {})}
    contigs = []
    for i, c in enumerate(case["contigs"]):
        rec, ref = contig_inputs(c)
        contigs.append((c["name"], c.get("tid", i), c["len"], ref, rec))
    check(contigs, opt, tmp_path)


@pytest.mark.parametrize("L", [1, 300, 2048, 2049, 4096, 6143])
@pytest.mark.parametrize("deep,overhang", [(False, False), (True, False), (False, True), (True, True)])
def test_adversarial_contigs(L, deep, overhang, tmp_path):
    n = {1: 5, 300: 2000, 2048: 500, 2049: 500, 4096: 900, 6143: 700}[L]
    rec = synth.adversarial_contig(L, n, 2000 + L, max_len=min(300, max(2, L)), deep=deep, overhang=overhang)
    ref = synth.make_reference(L, 60 + L % 7, lowercase=(L % 2 == 0))
    check([("chrA", L % 3, L, ref, rec)], dict(min_depth=2, min_depth_for_low_mapq=3), tmp_path)


@pytest.mark.parametrize("depth,planes,rounds", [(300, 16, 9), (66_000, 32, 17)])
def test_deep_piles_select_the_16_and_32_plane_kernels(depth, planes, rounds, tmp_path):
    contig, o_res, _, _ = depth_contigs.deep_pile(depth)
    _, tid, L, ref, rec = contig
    check([contig], depth_contigs.DEEP_OPTIONS, tmp_path, o_res=o_res)
    with Engine(_opts(depth_contigs.DEEP_OPTIONS), 0) as eng:
        eng.contig_begin(tid, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        assert eng.contig_layout()["counter_planes"] == planes
        whole = eng.target_order([0, 2100], [L, 2101])
        assert whole.n_rounds == rounds == int(whole.raw[0, 4]).bit_length() and int(whole.raw[0, 4]) == depth
        assert whole.raw[1].tolist() == [int(whole.raw[1, 0])] * 5


def test_many_windows_and_the_grid(tmp_path):
    """3078 windows: workgroups 0..1029 of k_target_order take two windows.  Targets across the boundaries of the scan
    steps (windows 1024, 2048, 3072) and of the grid (window 2048), the whole contig, and a window with pieces between
    many without."""
    contig, o_res, extent, depths = depth_contigs.scan_steps()
    assert extent == depth_contigs.SCAN_L and -(-extent // T) == 2048 + 1030

    def sets(E):
        out = [("edges", [0, 0, E - 1, E, 5], [0, E, E, E + 5, E + 100])]
        s, e = [], []
        for B in depth_contigs.SCAN_B + (2048 * T,):
            s += [B - 700, B - 1, B, B - 1, B - T, B + 3, B - 600]
            e += [B + 700, B + 1, B + 1, B, B + T, B + 3 * T + 5, B + 100]
        out.append(("boundaries", s, e))
        out.append(("one window in the middle", [1500 * T + 5, 1500 * T + 7], [1500 * T + 900, 1500 * T + 8]))
        rng = np.random.default_rng(99)
        a = rng.integers(0, E, 2000)
        b = a + np.where(np.arange(2000) < 40, rng.integers(0, 300_000, 2000), rng.integers(0, 400, 2000))
        out.append(("random", a.tolist(), b.tolist()))
        return out
    check([contig], {}, tmp_path, o_res=o_res, sets_of=sets)


def test_empty_contigs_no_targets_and_a_contig_without_reads(tmp_path):
    check([("e1", 0, 0, None, ContigRecords.empty()), ("e2", 1, 5000, None, ContigRecords.empty()),
           ("e3", 2, 4096, synth.make_reference(4096, 3), ContigRecords.empty())], dict(), tmp_path)
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, 5000, None)
        eng.contig_finish()
        r = eng.target_order([], [])
        assert r.len.shape == (0,) and r.raw.shape == (0, 5) and r.qc.shape == (0, 5) and r.n_rounds == 0
        r = eng.target_order([7, 5000, 9000], [7, 5001, 9001])
        assert r.len.tolist() == [0, 0, 0] and r.start.tolist() == [7, 5000, 5000] and r.end.tolist() == [7, 5000, 5000]
        assert not r.raw.any() and not r.qc.any() and r.n_rounds == 0
        # no read: no round, every value 0
        r = eng.target_order([0, 100, 2047], [5000, 101, 2049])
        assert r.len.tolist() == [5000, 1, 2] and not r.raw.any() and not r.qc.any() and r.n_rounds == 0


def test_refusals(monkeypatch):
    L = 5 * T - 7                                                  # five windows
    rec = synth.short_read_contig(L, 10, 5)
    ref = synth.make_reference(L, 6)
    with Engine(CallableOptions(), 0) as eng:
        def refused(text, starts=(0,), ends=(10,)):
            with pytest.raises(EngineError) as e:
                eng.target_order(starts, ends)
            assert e.value.status == -1 and text in str(e.value), str(e.value)

        def good():
            r = eng.target_order([0, 5], [L, 6])
            assert int(r.len[0]) == L and int(r.len[1]) == 1 and int(r.raw[0, 4]) == max_raw and r.raw[1].tolist() == [int(r.raw[1, 0])] * 5
        refused("has been run")                                    # nothing resident
        eng.contig_begin(0, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        refused("has been run")                                    # begun
        eng.contig_upload()
        refused("has been run")                                    # uploaded
        eng.contig_run()
        max_raw = int(eng.target_order([0], [L]).raw[0, 4])        # run, not collected: served
        extent = int(eng.contig_collect().summary.extent)
        assert max_raw == int(np.asarray(eng.debug_depths(extent)[0])[:L].max()) > 0
        good()
        refused("target 1 has start > end", starts=(3, 9), ends=(5, 8))
        good()
        # the piece cap: 2^24 whole-contig targets over five windows, refused on the host with the count and the limit
        n = 1 << 24
        refused(f"{5 * n} pieces", starts=np.zeros(n, np.uint32), ends=np.full(n, L, np.uint32))
        refused(str(1 << 26), starts=np.zeros(n, np.uint32), ends=np.full(n, 0xFFFFFFFF, np.uint32))
        good()
        # the ABI's own refusals: null result, null arrays with n > 0, too many targets
        lib, h = eng._lib, eng._h
        out = C.POINTER(_lib.cl_target_order)()
        one = (C.c_uint32 * 1)(0)
        for args, text in (((one, one, 1, None), "null result"),
                           ((None, one, 1, C.byref(out)), "null starts or ends"),
                           ((one, None, 1, C.byref(out)), "null starts or ends"),
                           ((one, one, (1 << 24) + 1, C.byref(out)), "2^24")):
            assert lib.cl_contig_target_order(h, *args) == -1
            assert text in lib.cl_last_error(h).decode()
            good()
        assert lib.cl_contig_target_order(h, None, None, 0, C.byref(out)) == 0 and not out
        ms, rounds = C.c_double(), C.c_uint32(7)
        assert lib.cl_contig_target_order_ms(h, C.byref(ms), C.byref(rounds)) == 0 and rounds.value == 0
        assert lib.cl_contig_target_order_ms(h, None, None) == -1
        good()
    monkeypatch.setenv("DUT_QUAL_FORM", "bytes")
    with Engine(CallableOptions(), 0) as eng:
        eng.contig_begin(0, L, ref)
        eng.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        eng.contig_finish()
        with pytest.raises(EngineError) as e:
            eng.target_order([0], [10])
        assert e.value.status == -1 and "pass-bit form only" in str(e.value)


def test_target_files_with_quantiles_devices_and_the_tool(tmp_path):
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
    regions = [("chr2", 100, 900, "b1"), ("chr1", 0, 2048, "a1"), ("chr1", 2047, 2049, None), ("chr2", 8_000, 20_000, "b2"),
               ("chr1", 29_000, 31_000, "a3"), ("chr1", 500, 700, "a4"), ("chr2", 50_000, 50_010, "beyond"), ("chr1", 600, 600, "empty")]
    bed = str(tmp_path / "t.bed")
    with open(bed, "w") as f:
        f.write("track name=t\n# a comment\n")
        for c, s, e, nm in regions:
            f.write("\t".join([c, str(s), str(e)] + ([nm] if nm else [])) + "\n")
    thr = (1, 10, 25)
    exp = []
    for name, _, length, _, _ in contigs:
        ro, qo, _, so, eo = o_res[name]["dumps"]
        assert eo >= length
        mine = [r for r in regions if r[0] == name]
        a, b = [r[1] for r in mine], [r[2] for r in mine]
        exp.append((name, targets_ref.target_stats(ro, qo, so, a, b, thr), [r[3] or "." for r in mine], order_ref.target_order(ro, qo, a, b)))
    text_q = order_ref.table_text(exp, thr)
    text_plain = targets_ref.table_text([x[:3] for x in exp], thr)
    assert "\tNA" * 10 + "\n" in text_q and text_q != text_plain

    def same_json(a, b):
        a, b = json.load(open(a)), json.load(open(b))
        a["files"] = b["files"] = None                              # (the paths differ)
        return a == b
    plain = tmp_path / "plain"; plain.mkdir()
    coverage_files(bam, fa, str(plain / "g.bed"), str(plain / "s.json"), CallableOptions(), targets=bed, target_out=str(plain / "t.tsv"), target_thresholds=thr)
    assert open(plain / "t.tsv").read() == text_plain and open(plain / "g.bed").read() == o_bed
    for devs in (None, [0, 0]):
        d = tmp_path / ("dev%d" % len(devs or [0])); d.mkdir()
        coverage_files(bam, fa, str(d / "g.bed"), str(d / "s.json"), CallableOptions(), devices=devs, targets=bed, target_out=str(d / "t.tsv"),
                       target_thresholds=thr, target_quantiles=True)
        assert open(d / "t.tsv").read() == text_q, devs
        assert open(d / "g.bed").read() == o_bed and same_json(plain / "s.json", d / "s.json"), devs
    # through the tool (it writes ./summary.json): with the flag and without it
    base = ["--targets", bed, "--target-out", "t.tsv", "--target-thresholds", "1,10,25"]
    for sub, extra in (("cliq", base + ["--target-quantiles"]), ("cli", base)):
        d = tmp_path / sub; d.mkdir()
        r = subprocess.run([_b.CLI, "coverage", bam, "-r", fa, "-o", "g.bed", "-s", "r.html"] + extra, cwd=str(d), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert open(tmp_path / "cliq" / "t.tsv").read() == text_q and open(tmp_path / "cli" / "t.tsv").read() == text_plain
    assert open(tmp_path / "cliq" / "g.bed").read() == open(tmp_path / "cli" / "g.bed").read() == o_bed
    assert open(tmp_path / "cliq" / "summary.json").read() == open(tmp_path / "cli" / "summary.json").read()
