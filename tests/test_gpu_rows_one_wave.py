"""k_pileup_rows with one wave per window (-m gpu): a lane counts a block of 32 positions and classifies the same 32 --
rows, candidates, depths, tests, masks, run list and totals with nothing handed between waves.  The cases sit where that
structure can go wrong: the seams between lanes (every 32 positions), a lane whose 32 positions are 32 runs, lanes whose
sum of differences is negative, the head trips of 64 x 8 candidates, the row trips of 12 groups, an extent that ends
inside a lane, and lanes that leave the byte thresholds for the general path.

Every case is a contig of a few windows (T = 2048) in the pass-bit form, held against the oracle as in
test_gpu_rows_depth_path.py (check_against_oracle there; `check` here is the same with the reference and the engine's
environment as parameters): per position (raw, low, qc, state: Engine.debug_depths, the DEBUG instantiation) and as BED
text, state counts and summary fields (the production instantiation)."""
import numpy as np
import pytest

from helpers import make_options, oracle_run
from decodingustools_amd import CallableOptions, CallableProfiler, ContigProfiler, Engine, process_single_contig, synth
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu

T, LANE, S = 2048, 32, 256
SUMS = ("n_covered_bases", "summed_coverage", "summed_baseq", "summed_mapq", "quality_bases", "n_reads")
REF_N, CALLABLE, NO_COVERAGE, LOW_COVERAGE, EXCESSIVE, POOR_MAPQ = range(6)


@pytest.fixture(autouse=True)
def pass_bit_form(monkeypatch):
    for k in ("DUT_QUAL_FORM", "DUT_HEADS8", "DUT_ROWS_UNIFORM", "DUT_HEAD_SPAN"):
        monkeypatch.delenv(k, raising=False)


def _engine_opts(d):
    o = make_options(d)
    return CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                           o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def check(reads, L, tmp_path, opt_dict=None, ref=None, seed=77):
    """reads: (pos, cigar, mapq[, qual]) tuples in any order; ref: the reference bytes (default: synth.make_reference).
    The engine reads its environment (DUT_HEADS8, DUT_ROWS_UNIFORM) when it is made: set it before the call.
    Returns the oracle's dumps (raw, qc, low, state, extent) and the engine's layout record."""
    reads = sorted(reads, key=lambda r: r[0])
    rec = ContigRecords.from_reads([(r[0], r[1], r[2], r[3] if len(r) > 3 else 30, 0, f"q{i}") for i, r in enumerate(reads)])
    if ref is None:
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


def _plain_ref(L):
    return np.full(L, ord("A"), dtype=np.uint8)


def _inner_boundaries(state, w):
    """run boundaries strictly inside window w: what the kernel's run list of that window holds"""
    s = state[w * T:(w + 1) * T]
    return int(np.count_nonzero(s[1:] != s[:-1]))


# ---- a: the seams between lanes ----
def test_state_changes_at_the_lane_seams(tmp_path):
    """In window 1 the state changes exactly at offsets 31, 32 and 33 (the last position of lane 0, the first two of
    lane 1: the state before a lane's first position comes from the lane below), a run of N fills lane 2 exactly, a
    run of CALLABLE lies over all of lanes 5 to 7, and the state changes at offset 2047 (lane 63's last bit).  Window 2
    begins in the state window 1 ended in and window 3 begins inside a read that crosses the seam: lane 0 of either has
    no boundary at its first position (the seam between windows is the tail's)."""
    W = T
    L = 3 * T + 200
    ref = _plain_ref(L)
    ref[W + 2 * LANE:W + 3 * LANE] = ord("N")
    reads = [(W, "31M", 60), (W + 32, "1M", 60), (W + 2 * LANE - 10, "60M", 60),
             (W + 5 * LANE - 7, f"{3 * LANE + 20}M", 60), (W + 2000, "47M", 60),
             (3 * T - 10, "20M", 60), (3 * T + 100, "30M", 60), (40, "100M", 60)]
    (_, _, _, st, _), _ = check(reads, L, tmp_path, dict(min_depth=1), ref=ref)
    assert [int(st[W + i]) for i in (30, 31, 32, 33)] == [CALLABLE, NO_COVERAGE, CALLABLE, NO_COVERAGE]
    assert (st[W + 2 * LANE:W + 3 * LANE] == REF_N).all() and st[W + 2 * LANE - 1] == CALLABLE and st[W + 3 * LANE] == CALLABLE
    assert (st[W + 5 * LANE - 7:W + 8 * LANE + 13] == CALLABLE).all()
    assert st[W + 2046] == CALLABLE and st[W + 2047] == NO_COVERAGE and st[2 * T] == NO_COVERAGE
    assert st[3 * T - 1] == CALLABLE and st[3 * T] == CALLABLE


# ---- b: the run list at its capacity ----
def test_every_position_a_boundary_and_64_and_65_boundaries(tmp_path):
    """Windows 0 and 1 are covered and the reference has N at every other position: every position but the window's
    first is a run boundary -- 32 per lane (31 in lane 0), 2047 entries per window, every lane's offset from the scan
    over the lanes.  Window 2 has exactly 64 boundaries and window 3 exactly 65 (the 64 entries a wave would hold with
    one per lane, and one more), several of them in one lane."""
    L = 4 * T
    ref = _plain_ref(L)
    ref[1:2 * T:2] = ord("N")
    for w in (2, 3):
        ref[w * T + 1:w * T + 65:2] = ord("N")             # 32 single N: 64 boundaries, in lanes 0 to 2
    ref[4 * T - 1] = ord("N")                              # window 3: one more, at its last position
    reads = [(0, f"{2 * T}M", 60), (2 * T, f"{2 * T}M", 60)]
    (_, _, _, st, _), _ = check(reads, L, tmp_path, dict(min_depth=1), ref=ref)
    assert [_inner_boundaries(st, w) for w in range(4)] == [T - 1, T - 1, 64, 65]


# ---- c: lanes whose sums of differences are negative ----
def test_ends_outnumber_starts_in_the_lanes_behind(tmp_path):
    """About 300 mapq-0 reads start inside one lane's 32 positions (lane 2 of window 1) and end 20 to 40 positions on:
    the lanes behind see only ends, so their sums are negative for both counts, packed two positions to a word.  The
    same again from offset 1000 on.  A few mapq-60 reads lie over both stretches, so that raw != low."""
    rng = np.random.default_rng(5)
    W = T
    reads = []
    for base in (2 * LANE, 1000):
        for i in range(300):
            reads.append((W + base + int(rng.integers(0, LANE)), f"{int(rng.integers(20, 41))}M", 0))
        for i in range(5):
            reads.append((W + base - 3 + 2 * i, "80M", 60))
    reads += [(100, "50M", 60), (2 * T + 10, "50M", 60)]
    (raw, _, low, _, _), _ = check(reads, 2 * T + 300, tmp_path)
    for base in (2 * LANE, 1000):
        p = W + base + LANE - 1
        assert raw[p - 6] > 100 and low[p - 6] > 100 and raw[p - 6] == low[p - 6] + 5
        assert raw[p + 41] == 5 and low[p + 41] == 0       # every mapq-0 read has ended: the lanes between took them away


# ---- d: the head trips ----
@pytest.mark.parametrize("heads8", [False, True])
def test_511_512_513_candidates(heads8, tmp_path, monkeypatch):
    """A wave takes 64 x 8 heads per trip: windows 0, 1 and 2 have exactly 511, 512 and 513 candidates (a candidate of
    a window is a read that starts less than the longest ordinary span in front of its end: every read here is 50 long
    and lies well inside its window).  Once in the 4-byte form of the heads; once in the 8-byte form (DUT_HEADS8=1) with
    one wide read (a span beyond 16 384: it reaches over every window, is their first candidate through wide_idx, and
    takes the extent to 9 windows), one ordinary read fewer per window."""
    rng = np.random.default_rng(11)
    L = 3 * T + 100
    reads = []
    for w, n in enumerate((511, 512, 513)):
        for i in range(n - (1 if heads8 else 0)):
            reads.append((w * T + 100 + int(rng.integers(0, 1700)), "50M", 0 if i % 9 == 0 else 60))
    if heads8:
        reads.append((10, "100M17000N100M", 60))
        monkeypatch.setenv("DUT_HEADS8", "1")
    (raw, _, _, _, eo), lay = check(reads, L, tmp_path)
    assert eo == (10 + 17200 if heads8 else L)
    assert lay["counter_planes"] == 8
    for w, n in enumerate((511, 512, 513)):
        # every candidate's whole span lies in its window; the wide read covers every position from 10 on (N included)
        wide = (T - 10 if w == 0 else T) if heads8 else 0
        assert int(raw[w * T:(w + 1) * T].astype(np.int64).sum()) == 50 * (n - (1 if heads8 else 0)) + wide


# ---- e: row trips and heights ----
def _rows_case(name):
    W = T
    if name == "49_rows":
        # 49 rows (13 groups: group 12 is the second trip of the twelve-in-flight loop) in segment 3 of window 1, taken
        # by the 8 lanes of that segment only; 3 rows in its neighbours
        reads = [(W + 3 * S + 40 + i, "100M", 60, 30 if i % 4 else 10) for i in range(49)]
        for s in (2, 4, 7):
            reads += [(W + s * S + 30 + 9 * i, "150M", 60, 30) for i in range(3)]
        reads += [(100 + 30 * i, "150M", 60, 30) for i in range(4)]
        return reads, 2 * T + 100, {}
    # n rows on one stretch of segment 5 of window 1: 252 -- 63 groups, the most that 8 planes count; 255 and 256 --
    # 64 groups: 16 planes, counts that take all 8 bits and a ninth
    n = int(name.split("_")[0])
    reads = [(W + 5 * S + 20 + (i % 8), "64M", 60, 30) for i in range(n)]
    reads += [(W + 6 * S + 1 + 3 * i, "40M", 60, 30) for i in range(5)] + [(50 + 40 * i, "150M", 60, 30) for i in range(6)]
    return reads, 2 * T + 300, dict(max_depth=5000)


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("name", ["49_rows", "252_rows", "255_rows", "256_rows"])
def test_row_trips_and_plane_counts(name, uniform, tmp_path, monkeypatch):
    if uniform:
        monkeypatch.setenv("DUT_ROWS_UNIFORM", "1")        # every segment as high as the window's highest
    reads, L, opts = _rows_case(name)
    (_, qc, _, _, _), lay = check(reads, L, tmp_path, opts)
    if name == "49_rows":
        assert lay["max_groups"] == 13 and lay["counter_planes"] == 8
        assert qc.max() == 36                              # 49 rows, every fourth (13) below the base-quality threshold
    else:
        n = int(name.split("_")[0])
        assert lay["max_groups"] == (n + 3) // 4 and lay["counter_planes"] == (8 if n <= 252 else 16)
        assert qc.max() == n


# ---- f: the extent ----
@pytest.mark.parametrize("L", [T + 1, T + 31, T + 32, T + 33, 2 * T])
def test_extent_ends_inside_a_lane(L, tmp_path):
    """The last window holds 1, 31, 32, 33 or all 2048 positions of the contig: a lane with one valid position, with all
    but one, exactly one whole lane (the mask of valid positions is a shift by 32 there), one lane and a bit, and a full
    window -- with workgroups of the grid beyond the last window in every case (the grid is a multiple of 8)."""
    reads = [(T - 40, f"{L - T + 40}M", 60), (T - 20, f"{L - T + 20}M", 60), (T - 10, f"{L - T + 10}M", 0), (L - 1, "1M", 60),
             (300, "200M", 60), (350, "200M", 60)]
    (raw, _, low, _, eo), _ = check(reads, L, tmp_path, dict(min_depth=2, min_depth_for_low_mapq=2), ref=_plain_ref(L))
    assert eo == L and raw[L - 1] == 4 and low[L - 1] == 1 and raw[T - 1] == 3


# ---- g: the general path ----
@pytest.mark.parametrize("depth, n_low, opts", [(255, 20, {}), (300, 60, {}), (300, 60, dict(max_depth=0)), (40, 2, dict(min_depth=300))])
def test_a_lane_on_the_general_path(depth, n_low, opts, tmp_path):
    """`depth` reads lie inside lane 3 of window 1 (offsets 100 to 120), `n_low` of them at mapq 0; the lanes around it
    stay at depth 12.  At 255 the lane leaves the byte thresholds (255 = never) for the 32-bit table -- 20 low reads of
    255 are not poor, 60 of 300 are --, its neighbours stay on the bytes; the rows stay within 8 planes.  With
    max_depth = 0 that rule is off; min_depth = 300 is a threshold beyond what 8 planes count to: every covered
    position is LOW_COVERAGE."""
    W = T
    reads = [(W + 100, "20M", 0 if i < n_low else 60) for i in range(depth - 12)]
    reads += [(W + 20, "300M", 60)] * 11 + [(W + 20, "300M", 0)]
    reads += [(W + 1100, "700M", 60)] * 10 + [(W + 1100, "700M", 0)] * 2 + [(50, "100M", 60)] * 5
    (raw, qc, low, st, _), lay = check(reads, 2 * T + 100, tmp_path, opts, ref=_plain_ref(2 * T + 100))
    assert lay["counter_planes"] == 8
    assert raw[W + 110] == depth and low[W + 110] == n_low + 1 and raw[W + 99] == 12 and raw[W + 120] == 12
    if opts.get("min_depth") == 300:
        assert st[W + 110] == LOW_COVERAGE and st[W + 60] == LOW_COVERAGE
    else:
        assert st[W + 110] == (POOR_MAPQ if 10 * (n_low + 1) > depth else CALLABLE)
        assert st[W + 60] == CALLABLE and st[W + 1500] == POOR_MAPQ
