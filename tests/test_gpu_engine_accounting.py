"""GPU test (-m gpu): the absolute figures of cl_contig_bytes and cl_contig_layout -- what bench.py's roofline is computed
from -- against the formulas in the comment of cl_contig_bytes, for every form of the pileup: the pass-bit form with
4-byte heads, with 8-byte heads and with a wide list, and the two byte forms (records, run table).  The expected values
are computed here from the layout's own element counts, the collected extent and the unit sizes of the kernels' headers
(kernels.hip.h: a 32-byte window record; pass_rows.h: a 128-byte row unit; pileup_bytes.hip.h: a 16-byte record).  Each
case holds the BED against the oracle, so none passes on a contig that did not run."""
import numpy as np
import pytest

from helpers import make_options, oracle_run
from decodingustools_amd import CallableOptions, CallableProfiler, ContigProfiler, Engine, process_single_contig, synth
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu

T = 2048                 # positions per window (callable_loci.hip: CL_WINDOW)
WIN, UNIT, REC = 32, 128, 16
WIDE = 16384             # engine_limits.h: kWideSpan
L = 3 * T + 156          # 3 windows and a part


def _short_reads(length, n=300, seed=1):
    rng = np.random.default_rng(seed)
    return [[int(p), "100M", int(rng.choice([5, 30, 60, 60])), int(rng.choice([10, 25, 40])), 0, f"s{i}"]
            for i, p in enumerate(np.sort(rng.integers(0, length - 100, n)))]


def _long_reads(length, n=40, seed=2):
    rng = np.random.default_rng(seed)
    reads = [[int(p), "20M1I20M1D20M1I20M1D20M", int(rng.choice([5, 60])), int(rng.choice([10, 30])), 0, f"l{i}"]
             for i, p in enumerate(np.sort(rng.integers(0, length - 300, n)))]
    reads[n // 2][1] = "5M1I5M1D" * 20 + "10M"          # 81 operations: beyond the 64 of a CIGAR checkpoint
    return reads


CASES = {
    # name: (environment, contig length, reads, form, bytes per head)
    "a_bits_heads4": ({}, L, _short_reads(L), 3, 4),
    "b_bits_heads8": ({"DUT_HEADS8": "1"}, L, _short_reads(L), 3, 8),
    "c_bits_wide_list": ({}, 30_000, sorted(_short_reads(30_000) + [[1000, "20000M", 60, 30, 0, "wide"]], key=lambda r: r[0]), 3, 8),
    "d_bytes_records": ({"DUT_QUAL_FORM": "bytes"}, L, _short_reads(L), 0, 0),
    "e_bytes_run_table": ({"DUT_QUAL_FORM": "bytes"}, L, _long_reads(L), 2, 0),
}


def _n_wide(rec):
    """Reads whose reference span (M D N = X) exceeds kWideSpan: each has one entry in the wide list."""
    op, ln = rec.cigar & 15, (rec.cigar >> 4).astype(np.int64)
    adv = np.where(np.isin(op, (0, 2, 3, 7, 8)), ln, 0)
    csum = np.concatenate([[0], np.cumsum(adv)])
    off = rec.cigar_off.astype(np.int64)
    return int(np.count_nonzero(csum[off[1:]] - csum[off[:-1]] > WIDE))


@pytest.mark.parametrize("case", list(CASES))
def test_contig_bytes_and_layout_are_the_documented_sums(case, tmp_path, monkeypatch):
    env, length, reads, form, head_bytes = CASES[case]
    for k in ("DUT_QUAL_FORM", "DUT_HEADS8", "DUT_HEAD_SPAN", "DUT_ROWS_UNIFORM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rec = ContigRecords.from_reads(reads)
    ref = synth.make_reference(length, 77)
    n_wide = _n_wide(rec)
    assert (n_wide > 0) == (case == "c_bits_wide_list")
    if form == 2:
        n_ops = np.diff(rec.cigar_off.astype(np.int64))
        assert n_ops.min() >= 8 and n_ops.max() > 64
    oo = make_options({})
    opt = CallableOptions(oo.min_depth, oo.max_depth, oo.min_mapping_quality, oo.min_base_quality,
                          oo.min_depth_for_low_mapq, oo.max_low_mapq, oo.max_low_mapq_fraction)
    _, o_bed = oracle_run([("chrA", 1, length, ref, rec)], oo, str(tmp_path / "o.bed"))
    bed = str(tmp_path / "g.bed")
    with Engine(opt, 0) as eng:
        counter = CallableProfiler(bed)
        process_single_contig(eng, counter, ContigProfiler("chrA", length), opt, 1, rec, ref)
        counter.close()
        res = eng.contig_collect()
        lay = eng.contig_layout()
        in_bytes, out_bytes = eng.contig_bytes()
        # a second, smaller contig on the same context: the context keeps what it holds
        eng.contig_begin(2, length, ref)
        half = rec.slice(0, rec.n // 2)
        eng.push_reads(half.pos, half.mapq, half.cigar_off, half.cigar, half.qual_off, half.qual)
        eng.contig_finish()
        lay2 = eng.contig_layout()
    assert open(bed).read() == o_bed and o_bed

    extent, n_iv = int(res.summary.extent), int(res.intervals.shape[0])
    n_win, n_rec, n_reads, n_qual = lay["n_windows"], lay["n_records"], lay["n_reads"], lay["n_qual"]
    groups, runtab = lay["row_groups"], lay["run_table_entries"]
    print(case, dict(lay), in_bytes, out_bytes, extent, n_iv, n_wide)
    assert lay["form"] == form and extent == length and n_win == (extent + T - 1) // T
    assert n_reads == rec.n and n_qual == rec.qual.shape[0] and n_iv > 0
    padded = n_win * T
    if form == 3:
        assert n_rec == n_reads and groups >= lay["max_groups"] > 0 and runtab == 0
        want_in = (extent + 7) // 8 + WIN * n_win + UNIT * groups + head_bytes * n_rec + 4 * n_wide
        want_h2d = padded // 8 + WIN * n_win + 4 * n_wide + UNIT * groups + (n_rec + 1) * head_bytes
        want_planes = 8 if lay["max_groups"] <= 63 else 16 if lay["max_groups"] <= 16383 else 32
    elif form == 0:
        assert n_rec >= n_reads and groups == 0 and runtab == 0
        want_in = extent + WIN * n_win + n_qual + REC * n_rec + 4 * n_wide
        want_h2d = padded + 16 + WIN * n_win + 4 * n_wide + n_qual + (n_rec + 1) * REC
        want_planes = 0
    else:
        assert runtab > 0 and groups == 0
        want_in = extent + WIN * n_win + n_qual + 8 * runtab + 9 * n_reads + 4 * n_wide
        want_h2d = padded + 16 + WIN * n_win + 4 * n_wide + n_qual + 8 * runtab + 9 * n_reads
        want_planes = 0
    assert in_bytes == want_in, (in_bytes, want_in)
    assert out_bytes == 12 * n_iv
    assert lay["upload_h2d_bytes"] == want_h2d, (lay["upload_h2d_bytes"], want_h2d)
    assert lay["counter_planes"] == want_planes
    assert lay["device_bytes"] > 0 and lay2["device_bytes"] >= lay["device_bytes"]
