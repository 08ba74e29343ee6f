"""The contigs that tests/test_gpu_depth_profile.py and tests/test_gpu_depth_runs.py share, each built once per session
with its reference: the launch constants of cl_contig_depth_profile (2048 workgroups), cl_contig_depth_runs (65536) and
k_depth_runs_scan (1024 windows per step) decide which code a contig reaches, and these reach what lies beyond them."""
import functools
import os
import tempfile

import numpy as np

import depth_ref
from helpers import make_options, oracle_run
from decodingustools_amd import synth
from decodingustools_amd.records import ContigRecords

T = 2048                                           # positions per window of the depth kernels
SCAN_STEP = 1024 * T                               # positions per step of k_depth_runs_scan
WIDE_SPAN = 16384                                  # kWideSpan: a longer reference span goes to the wide list
REF_OPS = (0, 2, 3, 7, 8)                          # M D N = X consume the reference


def ref_spans(rec):
    """reference positions every read spans"""
    ln = np.where(np.isin(rec.cigar & np.uint32(15), REF_OPS), rec.cigar >> np.uint32(4), 0).astype(np.int64)
    return np.diff(np.concatenate(([0], np.cumsum(ln)))[rec.cigar_off.astype(np.int64)])


def _gather(off, data, idx):
    off = off.astype(np.int64)
    ln = (off[1:] - off[:-1])[idx]
    new = np.concatenate(([0], np.cumsum(ln)))
    src = np.repeat(off[:-1][idx] - new[:-1], ln) + np.arange(new[-1])
    return new, np.ascontiguousarray(data[src])


def take(rec, idx):
    """the reads idx of rec, in that order"""
    idx = np.asarray(idx, np.int64)
    co, c = _gather(rec.cigar_off, rec.cigar, idx)
    qo, q = _gather(rec.qual_off, rec.qual, idx)
    no, n = _gather(rec.qname_off, rec.qname, idx)
    return ContigRecords(pos=np.ascontiguousarray(rec.pos[idx]), flag=np.ascontiguousarray(rec.flag[idx]),
                         mapq=np.ascontiguousarray(rec.mapq[idx]), cigar_off=co.astype(np.uint32), cigar=c,
                         qual_off=qo.astype(np.uint64), qual=q, qname_off=no.astype(np.uint32), qname=n).validate()


def merge(a, b):
    """the reads of a and b in coordinate order (a's first where they start together)"""
    both = ContigRecords(pos=np.concatenate((a.pos, b.pos)), flag=np.concatenate((a.flag, b.flag)), mapq=np.concatenate((a.mapq, b.mapq)),
                         cigar_off=np.concatenate((a.cigar_off, b.cigar_off[1:] + a.cigar_off[-1])), cigar=np.concatenate((a.cigar, b.cigar)),
                         qual_off=np.concatenate((a.qual_off, b.qual_off[1:] + a.qual_off[-1])), qual=np.concatenate((a.qual, b.qual)),
                         qname_off=np.concatenate((a.qname_off, b.qname_off[1:] + a.qname_off[-1])), qname=np.concatenate((a.qname, b.qname)))
    return take(both, np.argsort(both.pos, kind="stable"))


def _with_oracle(contig, opt_dict):
    """(contig, what helpers.oracle_run gives for it with the depths dumped, its extent, its depths padded to the extent)"""
    name, _, length, _, _ = contig
    with tempfile.TemporaryDirectory() as d:
        o_res, _ = oracle_run([contig], make_options(opt_dict), os.path.join(d, "o.bed"), dump=True)
    ro, qo, _, _, eo = o_res[name]["dumps"]
    extent = max(eo, length)
    depths = {"raw": depth_ref.pad(ro, extent), "qc": depth_ref.pad(qo, extent)}
    for a in depths.values():
        a.setflags(write=False)
    return contig, o_res, extent, depths


# ---- past one step of the scan, and past one window per workgroup of k_depth_profile ----
SCAN_L = 3 * SCAN_STEP + 5 * T + 17                # 3078 windows: four steps; workgroups 0..1029 of k_depth_profile take two
SCAN_B = (SCAN_STEP, 2 * SCAN_STEP, 3 * SCAN_STEP)  # the first positions of windows 1024, 2048, 3072
SCAN_CLEAR = 3000                                  # no background read touches [B - 3000, B + 3000)
SCAN_PLANTED = [(SCAN_B[0] - 500, "1000M"),                                                   # one read across B_1
                # (nothing at B_2: depth 0 goes on across it)
                (SCAN_B[2] - 500, "500M"), (SCAN_B[2] - 200, "200M"), (SCAN_B[2], "500M")]     # 1, 2 | 1 at B_3


@functools.lru_cache(maxsize=None)
def scan_steps():
    base = synth.short_read_contig(SCAN_L, 3, 11)
    end = base.pos.astype(np.int64) + ref_spans(base)
    touches = np.zeros(base.n, bool)
    for B in SCAN_B:
        touches |= (base.pos < B + SCAN_CLEAR) & (end > B - SCAN_CLEAR)
    assert 0 < int(touches.sum()) < base.n // 100
    planted = ContigRecords.from_reads([(p, cig, 60, 30, 0, f"h{i}") for i, (p, cig) in enumerate(SCAN_PLANTED)])
    rec = merge(take(base, np.flatnonzero(~touches)), planted)
    return _with_oracle(("chrS", 4, SCAN_L, synth.make_reference(SCAN_L, 12), rec), {})


# ---- windows that only reads of the wide list cover, among short reads ----
WIDE_L = 300_000
WIDE_OPTIONS = dict(min_depth=2, min_depth_for_low_mapq=3)


@functools.lru_cache(maxsize=None)
def wide_list():
    """short reads at 12x over the first third; ten reads with a gap of 20,000 to 250,000 positions that start among them,
    and one read that spans the contig: behind the short reads, the windows inside the gaps have raw depth from the wide
    list alone"""
    L = WIDE_L
    base = synth.short_read_contig(L, 12, 555)
    short = base.slice(0, base.n // 3)
    rng = np.random.default_rng(557)
    extra = [(10, f"10M{L - 100}N10M", 60, 30, 0, "span_all")]
    for i, gap in enumerate([20_000, 250_000, 70_000, 120_000, 200_000, 20_000, 250_000, 160_000, 70_000, 230_000]):
        p = int(rng.integers(100, 40_000))
        extra.append((p, f"60M{gap}{'N' if i % 2 else 'D'}40M5S", int(rng.choice([0, 30, 60])), 35, 0, f"w{i}"))
    rec = merge(short, ContigRecords.from_reads(sorted(extra, key=lambda r: r[0])))
    return _with_oracle(("chrW", 5, L, synth.make_reference(L, 556), rec), WIDE_OPTIONS)


def assert_wide_only_windows(rec, depths):
    """from the reads and the oracle alone: some spans go to the wide list, and at least one whole window has raw depth
    everywhere, no qc depth anywhere and no read that starts in it or within WIDE_SPAN positions before it"""
    span = ref_spans(rec)
    assert int((span > WIDE_SPAN).sum()) >= 10 and int((span <= WIDE_SPAN).sum()) > 1000
    pos = np.sort(rec.pos.astype(np.int64))
    found = []
    for w in range(len(depths["raw"]) // T):
        lo, hi = w * T, (w + 1) * T
        n_start = np.searchsorted(pos, hi) - np.searchsorted(pos, lo - WIDE_SPAN)
        if n_start == 0 and depths["raw"][lo:hi].min() >= 1 and depths["qc"][lo:hi].max() == 0:
            found.append(w)
    assert found, "no window that the wide list alone covers"
    return found


# ---- more wide candidates in a window than a workgroup of the depth kernels has threads ----
PILE_L = 60_000
PILE_OPTIONS = dict(max_depth=1_000_000)           # admission drops nothing
DEPTH_BLOCK = 128                                  # kDepthBlock: the stride of wd_scatter's loop over a window's candidates


@functools.lru_cache(maxsize=None)
def wide_pile(n_wide, n_deep=0):
    """short reads at 12x; n_wide reads with a gap of 17,000 or 20,000 positions that start 5 positions apart from 0 on, of
    every mapq (0 / 30 / 60) and base quality (10 / 30), so that raw, low-mapq and qc depth all differ; 20 reads with a gap
    of 30,000 from window 3 on.  The first windows have more than 128 candidates from the wide list and the short reads
    behind them: the candidate loop takes a second trip inside the wide part, and one trip straddles the two parts.
    n_deep passing reads of 120 positions on 60 positions of window 1: beyond 252 of them a segment's stack of rows is
    higher than 63 units, and the contig takes 16 counter planes."""
    L = PILE_L
    base = synth.short_read_contig(L, 12, 71)
    extra = [(5 * i, "60M17000D40M" if i % 2 else "100M20000N100M", (0, 30, 60)[i % 3], (10, 30)[(i // 2) % 2], 0, f"w{i}")
             for i in range(n_wide)]
    extra += [(3 * T + 7 * i, "50M30000N50M", (60, 0, 30)[i % 3], 30, 0, f"x{i}") for i in range(20)]
    extra += [(T + 1000 + i % 60, "120M", 60, 10 if i % 5 == 4 else 30, 0, f"d{i}") for i in range(n_deep)]
    rec = merge(base, ContigRecords.from_reads(sorted(extra, key=lambda r: r[0])))
    return _with_oracle(("chrP", 6, L, synth.make_reference(L, 72), rec), PILE_OPTIONS)


def assert_wide_pile_windows(rec, depths):
    """from the reads and the oracle alone: at least one window is overlapped by more spans above WIDE_SPAN than
    DEPTH_BLOCK, short reads start inside that same window, and the three depths differ there"""
    span = ref_spans(rec)
    pos = rec.pos.astype(np.int64)
    wide = span > WIDE_SPAN
    w_pos, w_end = pos[wide], (pos + span)[wide]
    s_pos = np.sort(pos[~wide & (span > 0)])
    found = []
    for w in range(-(-len(depths["raw"]) // T)):
        lo, hi = w * T, (w + 1) * T
        n_wide = int(((w_pos < hi) & (w_end > lo)).sum())
        n_short = int(np.searchsorted(s_pos, hi) - np.searchsorted(s_pos, lo))
        if n_wide > DEPTH_BLOCK and n_short > 0:
            found.append(w)
            raw, qc = depths["raw"][lo:hi], depths["qc"][lo:hi]
            assert 0 < int(qc.max()) < int(raw.max()), w
    assert found, "no window with more than %d wide candidates and short reads behind them" % DEPTH_BLOCK
    return found


# ---- one position deeper than the counter planes of 8 and of 16 bits hold ----
DEEP_L = 7000
DEEP_OPTIONS = dict(max_depth=1_000_000)


@functools.lru_cache(maxsize=None)
def deep_pile(depth):
    """`depth` reads on 60 positions (of 120 bases; 300 of them: 16 counter planes) or on 4 (of 20 bases; 66,000: 32)"""
    L = DEEP_L
    rng = np.random.default_rng(depth)
    reads = [[int(p), "120M" if depth < 1000 else "20M", int(rng.choice([10, 20, 60, 60])), int(rng.choice([10, 20, 40])), 0, f"d{i}"]
             for i, p in enumerate(np.sort(rng.integers(2000, 2060 if depth < 1000 else 2004, depth)))]
    rec = ContigRecords.from_reads([tuple(r) for r in reads])
    return _with_oracle(("chrD", 3, L, synth.make_reference(L, 8), rec), DEEP_OPTIONS)


# ---- past one window per workgroup of k_depth_runs: 65536 is its launch constant ----
RUNS_GRID = 65536
BIG_L = RUNS_GRID * T + 3 * T + 5                  # 65540 windows: workgroups 0..3 of k_depth_runs take a second one
BIG_B = RUNS_GRID * T                              # the first position of window 65536: also a step boundary of the scan
BIG_KINDS = ((60, 30), (60, 10), (5, 30))          # (mapq, base quality): passes both, fails the base quality, fails the mapq


@functools.lru_cache(maxsize=None)
def beyond_the_runs_grid():
    """-> (records, raw, qc): 100-base reads of one M each; raw and qc are the (start, end) of tests/sparse_ref.py, qc by
    the thresholds of make_options({})"""
    L, B = BIG_L, BIG_B
    rng = np.random.default_rng(65536)
    reads = [(int(p), 100, BIG_KINDS[int(k)]) for p, k in zip(rng.integers(0, L - 100, 4000), rng.integers(0, 3, 4000))]
    for k in range(4):
        # a workgroup's first and second window: k + 1 reads in window k, 6 - k in window 65536 + k, elsewhere in the window
        reads += [(k * T + 300 + 130 * k + 40 * j, 100, BIG_KINDS[j % 3]) for j in range(k + 1)]
        if k < 3:
            reads += [(B + k * T + 900 + 70 * k + 55 * j, 100, BIG_KINDS[(j + k) % 3]) for j in range(6 - k)]
    reads += [(B - 50, 100, BIG_KINDS[0]),                                                  # one read across B
              (B - 300, 300, BIG_KINDS[0]), (B, 300, BIG_KINDS[0]),                          # abutting, 2 on both sides of B
              (B + T - 200, 200, BIG_KINDS[0]), (B + T - 100, 100, BIG_KINDS[0]), (B + T, 150, BIG_KINDS[0]),   # 1, 2 | 1
              # window 65539 has 5 positions: two reads that end with the contig
              (L - 100, 100, BIG_KINDS[0]), (L - 3, 3, BIG_KINDS[1])]
    reads.sort(key=lambda r: r[0])
    rec = ContigRecords.from_reads([(p, f"{n}M", mq, q, 0, f"b{i}") for i, (p, n, (mq, q)) in enumerate(reads)])
    o = make_options({})
    start = np.asarray([r[0] for r in reads], np.int64)
    end = start + np.asarray([r[1] for r in reads], np.int64)
    ok = np.asarray([mq >= o.min_mapping_quality and q >= o.min_base_quality for _, _, (mq, q) in reads])
    assert int(end.max()) == L and 1000 < int(ok.sum()) < len(reads) - 2000
    for a in (start, end, ok):
        a.setflags(write=False)
    return rec, (start, end), (start[ok], end[ok])
