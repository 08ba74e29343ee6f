"""k_pileup_rows with one packed difference word per position (raw + (low << 16), the forms without DEEP) and a
carry-save tree over 8 or 16 rows at a time (-m gpu).  The cases sit where those two can go wrong:

  the packed word: lanes whose sums borrow from one field into the other (a negative raw sum beside a positive low sum
  and the reverse), positions with low == raw and with low == 0 < raw, reads that end exactly at a window's end (no
  end scatter) and one position in front of it, a read over two window seams, the byte thresholds at raw depths of 254,
  255 and 256 with the low count one below and at the threshold (the fast path, its exit, and the general path on
  packed words), and the limits of the 16-bit fields: exactly 32 767 candidates over one position, at mapq 60 and at
  mapq 0, and one more, which is DEEP's;

  the tree: segments of 1, 3, 4, 5, 8, 9, 12, 13, 16 and 17 groups (every way a chunk of four group slots can be
  taken: not at all, as 8 rows, as 16), exactly 48 and 49 rows (the second trip), one segment of 13 groups among
  segments of 1, depth steps 127 -> 128 and 254 -> 255 (a carry through every plane), 63 and 64 groups (8 and 16
  planes), and depth thresholds that the top planes decide.

Every case is a contig of 2 to 4 windows (T = 2048) held against the oracle with the `check` of
test_gpu_rows_one_wave.py (copied: per position raw, low, qc and state from Engine.debug_depths, the DEBUG
instantiation; BED text, state counts and summary sums from the production instantiation), once with 4-byte heads
and once with DUT_HEADS8=1; the row cases also with DUT_ROWS_UNIFORM=1."""
import numpy as np
import pytest

from helpers import make_options, oracle_run
from decodingustools_amd import CallableOptions, CallableProfiler, ContigProfiler, Engine, process_single_contig, synth
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu

T, LANE, S = 2048, 32, 256
SUMS = ("n_covered_bases", "summed_coverage", "summed_baseq", "summed_mapq", "quality_bases", "n_reads")
REF_N, CALLABLE, NO_COVERAGE, LOW_COVERAGE, EXCESSIVE, POOR_MAPQ = range(6)


@pytest.fixture(autouse=True, params=[False, True], ids=["heads4", "heads8"])
def head_form(request, monkeypatch):
    for k in ("DUT_QUAL_FORM", "DUT_HEADS8", "DUT_ROWS_UNIFORM", "DUT_HEAD_SPAN"):
        monkeypatch.delenv(k, raising=False)
    if request.param:
        monkeypatch.setenv("DUT_HEADS8", "1")


@pytest.fixture(params=[False, True], ids=["heights", "uniform"])
def uniform(request, monkeypatch, head_form):
    if request.param:
        monkeypatch.setenv("DUT_ROWS_UNIFORM", "1")        # every segment as high as the window's highest
    return request.param


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


def _lane_sum(depth, w, lane):
    """the sum of a count's differences over one lane's 32 positions: what the lane adds up before the scan"""
    p = w * T + lane * LANE
    return int(depth[p + LANE - 1]) - (int(depth[p - 1]) if p else 0)


# ---------------------------------------------------------------- the packed word ----

def test_borrow_between_the_fields(tmp_path):
    """Window 1.  300 mapq-0 reads start in lane 2 and end 20 to 40 positions on, in lanes 2 to 4, while 150 mapq-60
    reads that started in lane 1 end in lanes 3 and 4, where 100 more mapq-0 reads start: lanes whose raw sum is
    negative while their low sum is zero or positive.  From offset 1000 on the reverse: mapq-0 reads end in a lane in
    which more mapq-60 reads start (raw up, low down).  In a packed word the low field's borrow runs through the raw
    field's carry; only the running sum at a position is the two counts again.  Position 70 of the window is covered by
    mapq-0 reads only (low == raw), position 40 by mapq-60 reads only (low == 0 < raw)."""
    rng = np.random.default_rng(23)
    W = T
    reads = []
    for i in range(300):
        reads.append((W + 2 * LANE + int(rng.integers(0, LANE)), f"{int(rng.integers(20, 41))}M", 0))
    for i in range(150):                                   # start in lane 1 behind offset 40, end in lanes 5 and 6
        reads.append((W + 41 + (i % 23), f"{5 * LANE - 41 - (i % 23) + int(rng.integers(0, 2 * LANE))}M", 60))
    for i in range(40):                                    # lane 6: low starts where the mapq-60 reads end
        reads.append((W + 6 * LANE + (i % LANE), "70M", 0))
    for i in range(40):                                    # lane 5: ends of mapq-60 reads and nothing else
        reads.append((W + 3 * LANE + 16 + (i % 16), f"{2 * LANE + (i % LANE) - 16 - (i % 16)}M", 60))
    reads += [(W + 36, "4M", 60)] * 3                      # offsets 36..39: mapq 60 only
    # the reverse from offset 1000 (lane 31) on: 200 mapq-0 reads end in lane 33, where 260 mapq-60 reads start
    for i in range(200):
        reads.append((W + 1000 + (i % 20), f"{33 * LANE - 1000 - (i % 20) + 1 + (i % 31)}M", 0))
    for i in range(260):
        reads.append((W + 33 * LANE + (i % LANE), "90M", 60))
    reads += [(100, "50M", 60), (2 * T + 10, "50M", 0)]
    (raw, _, low, _, _), _ = check(reads, 2 * T + 300, tmp_path)
    sums = {l: (_lane_sum(raw, 1, l), _lane_sum(low, 1, l)) for l in (2, 4, 5, 6, 33)}
    assert sums[5][0] < 0 and sums[5][1] == 0, sums        # raw negative, low zero
    assert sums[6][0] < 0 < sums[6][1], sums               # raw negative, low positive
    assert sums[33][1] < 0 < sums[33][0], sums             # raw positive, low negative
    assert sums[2][0] > 0 and sums[2][1] > 0, sums
    assert raw[W + 38] == 3 and low[W + 38] == 0           # low == 0 < raw
    assert raw[W + 1005] == low[W + 1005] > 0              # low == raw


def test_window_edges(tmp_path):
    """Reads that end exactly at a window's end W + T (no end scatter in that window), one position in front of it
    (the end scatter in the window's last word), one that starts at W, one over two seams (it covers all of window 2:
    no scatter there but the start at offset 0; it ends in lane 0 of window 3), and an extent that ends inside a lane
    (L = 3 T + 45)."""
    W = T
    L = 3 * T + 45
    reads = [(W + T - 50, "50M", 60), (W + T - 50, "50M", 0), (W + T - 60, "59M", 60), (W + T - 60, "59M", 0),
             (W, "40M", 0), (W, "40M", 60), (W - 1, "1M", 60),
             (W + T - 100, f"{T + 120}M", 0), (W + T - 90, f"{T + 120}M", 60), (W + 300, f"{T}M", 60),
             (3 * T + 20, "25M", 60), (3 * T + 30, "15M", 0), (3 * T + 44, "1M", 60), (10, "100M", 60)]
    (raw, _, low, _, eo), _ = check(reads, L, tmp_path, dict(min_depth=1, min_depth_for_low_mapq=2), ref=_plain_ref(L))
    assert eo == L
    assert raw[2 * T - 1] == 5 and low[2 * T - 1] == 2 and raw[2 * T - 2] == 7 and low[2 * T - 2] == 3
    assert raw[2 * T] == 3 and low[2 * T] == 1 and raw[3 * T - 1] == 2 and raw[3 * T] == 2
    assert raw[W] == 2 and low[W] == 1 and raw[W - 1] == 1 and raw[W + 40] == 0
    assert raw[L - 1] == 3 and low[L - 1] == 1


def _stack(at, n_high, n_low, length=1):
    return [(at, f"{length}M", 60)] * n_high + [(at, f"{length}M", 0)] * n_low


@pytest.mark.parametrize("mdl", [10, 255, 300], ids=lambda v: f"min_depth_for_low_mapq_{v}")
def test_threshold_bytes_and_their_exit(mdl, tmp_path):
    """max_low_mapq_fraction = 0.1: at raw depths of 254, 255 and 256 a low count of 26 is "too many" and 25 is not
    (25.4, 25.5, 25.6).  Window 1 has these six (raw, low) pairs at neighbouring positions of ONE lane (lane 3: it
    sees 255 and leaves the byte thresholds for the general path, which splits the packed words), the two pairs of
    254 in lane 8 (the largest depth the bytes serve: the fast path), those of 255 in lane 12 and of 256 in lane 20,
    the lanes between at depth 12 on the fast path.  With min_depth_for_low_mapq at 255 the rule is off at 254 only,
    at 300 at every depth used here."""
    W = T
    pairs = [(254, 25), (254, 26), (255, 25), (255, 26), (256, 25), (256, 26)]
    reads = [(W + 20, "1200M", 60)] * 11 + [(W + 20, "1200M", 0)] + [(60, "100M", 60)] * 5

    def place(at, pp):
        out = []
        for i, (r, l) in enumerate(pp):
            out += _stack(at + i, r - l - 11, l - 1)
        return out
    reads += place(W + 3 * LANE + 4, pairs) + place(W + 8 * LANE + 30, pairs[:2]) + place(W + 12 * LANE, pairs[2:4])
    reads += place(W + 20 * LANE + 15, pairs[4:])
    L = 2 * T + 100
    (raw, _, low, st, _), lay = check(reads, L, tmp_path, dict(min_depth_for_low_mapq=mdl), ref=_plain_ref(L))
    assert lay["counter_planes"] == 8
    for at, pp in ((W + 3 * LANE + 4, pairs), (W + 8 * LANE + 30, pairs[:2]), (W + 12 * LANE, pairs[2:4]), (W + 20 * LANE + 15, pairs[4:])):
        for i, (r, l) in enumerate(pp):
            assert (int(raw[at + i]), int(low[at + i])) == (r, l)
            assert st[at + i] == (POOR_MAPQ if l == 26 and r >= mdl else CALLABLE), (r, l, mdl)
    assert raw[W + 5 * LANE] == 12 and st[W + 5 * LANE] == CALLABLE


@pytest.mark.parametrize("n, mapq", [(32767, 60), (32767, 0), (32768, 60), (32768, 0)])
def test_sixteen_bit_limits(n, mapq, tmp_path):
    """Window 1 has exactly n candidates, all over one position.  32 767 is the most a window without DEEP has: raw =
    0x7FFF, the edge of the sign tests on the packed word ((raw - 1) << 16 must not be negative), and at mapq 0 the
    low field is 0x7FFF as well (the whole word 0x7FFF7FFF).  One read more is DEEP's (two 32-bit arrays): a packed
    word could not hold it.  (The reads of window 0 end far in front of window 1: no candidates of it.)"""
    W = T
    reads = [(W + 500 + (i & 1), "3M", mapq, 30 if i % 3 else 10) for i in range(n)]
    reads += [(100, "3M", 60), (200, "3M", 0), (W + 900, "3M", 60), (W + 900, "3M", 0)][:2]
    L = 2 * T + 10
    # (the pileup drops a read that starts where more than max_depth reads are open: a max_depth above n keeps them all)
    (raw, qc, low, st, _), lay = check(reads, L, tmp_path, dict(max_depth=40000), ref=_plain_ref(L))
    assert raw[W + 501] == n and low[W + 501] == (n if mapq == 0 else 0)
    assert raw[W + 500] == (n + 1) // 2 and raw[W + 499] == 0 and raw[W + 504] == 0
    assert st[W + 501] == (POOR_MAPQ if mapq == 0 else CALLABLE)
    if mapq:
        assert lay["counter_planes"] == 16 and qc[W + 501] == n - (n + 2) // 3


# ---------------------------------------------------------------- the tree ----

def _segment_rows(w, s, n, length=64):
    """n rows in segment s of window w: n reads over one stretch, every fourth below the base-quality threshold"""
    return [(w * T + s * S + 20 + (i % 8), f"{length}M", 60, 30 if i % 4 else 10) for i in range(n)]


@pytest.mark.parametrize("rows", [(1, 9, 13, 20), (32, 33, 48, 49), (64, 65)], ids=lambda r: "rows_" + "_".join(map(str, r)))
def test_segment_heights(rows, uniform, tmp_path):
    """Window w + 1's highest segment has rows[w] rows: 1, 3, 4, 5 / 8, 9, 12, 13 / 16 and 17 groups of 4 -- every way
    the wave's three chunks of four group slots are taken (a chunk with 1 or 2 groups as 8 rows, with 3 or 4 as 16, a
    chunk past the highest segment not at all), exactly 48 rows (12 groups: one trip) and 49 (the second trip).  The
    other segments of the window are lower: one a group lower, one of half the rows, the rest of 2 rows or none."""
    reads = [(50 + 40 * i, "150M", 60) for i in range(6)]
    for w, n in enumerate(rows, start=1):
        top = (w + 2) % 8
        reads += _segment_rows(w, top, n)
        if n > 4:
            reads += _segment_rows(w, (top + 1) % 8, n - 4) + _segment_rows(w, (top + 3) % 8, n // 2, length=100)
        reads += _segment_rows(w, (top + 5) % 8, 2)
    L = (len(rows) + 1) * T + 77
    (_, qc, _, _, _), lay = check(reads, L, tmp_path, dict(max_depth=70))
    assert lay["max_groups"] == (max(rows) + 3) // 4 and lay["counter_planes"] == 8
    for w, n in enumerate(rows, start=1):
        assert qc[w * T:(w + 1) * T].max() == max(n - (n + 3) // 4, 1)     # (1: the segment of 2 rows beside a single row)


def test_one_high_segment_among_low_ones(uniform, tmp_path):
    """Segment 5 of window 1 has 13 groups (49 rows: two trips), every other segment of the window one group; window 2
    has one group everywhere: the heights differ most (the q0 form, or with DUT_ROWS_UNIFORM=1 thirteen everywhere)."""
    reads = []
    for s in range(8):
        reads += _segment_rows(1, s, 49 if s == 5 else 3) + _segment_rows(2, s, 4, length=200)
    reads += [(10, "100M", 60)]
    (_, qc, _, _, _), lay = check(reads, 3 * T + 5, tmp_path)
    assert lay["max_groups"] == 13 and qc.max() == 49 - 13


@pytest.mark.parametrize("opts", [dict(min_depth=128, max_depth=200), dict(min_depth=64, max_depth=254), dict(min_depth=255, max_depth=0)],
                         ids=lambda o: f"min{o['min_depth']}_max{o['max_depth']}")
def test_depth_steps_through_every_plane(opts, uniform, tmp_path):
    """A staircase of qc_depth inside one lane and over a lane's seam (window 1, segment 2): 127, 128, 200, 201, 254,
    255 at neighbouring stretches of 3 positions -- 127 -> 128 and 254 -> 255 change every plane of the count (255 rows
    are 64 groups: 16 planes).  min_depth / max_depth sit at those steps, so that the comparison with them is decided
    by the top planes (and at 255 by all eight).  The pileup keeps at most max_depth + 1 reads open (0: 500), so the
    staircase ends one above max_depth: with max_depth = 200 at 201, on 8 planes."""
    W = T
    at = W + 2 * S + 3 * LANE - 9                          # the last two steps lie in the next lane
    steps = [d for d in (127, 128, 200, 201, 254, 255) if not opts["max_depth"] or d <= opts["max_depth"] + 1]
    reads, have = [], 0
    for i, d in enumerate(steps):
        reads += [(at + 3 * i, f"{3 * (len(steps) - i)}M", 60)] * (d - have)
        have = d
    reads += [(W + 40, "100M", 60)] * 5 + [(30, "100M", 60)] * 4
    L = 2 * T + 9
    (_, qc, _, st, _), lay = check(reads, L, tmp_path, opts, ref=_plain_ref(L))
    assert lay["max_groups"] == (steps[-1] + 3) // 4 and lay["counter_planes"] == (16 if steps[-1] > 252 else 8)
    for i, d in enumerate(steps):
        assert qc[at + 3 * i] == d and qc[at + 3 * i + 2] == d
        want = LOW_COVERAGE if d < opts["min_depth"] else (EXCESSIVE if opts["max_depth"] and d > opts["max_depth"] else CALLABLE)
        assert st[at + 3 * i + 1] == want, (d, opts)


@pytest.mark.parametrize("n", [252, 253])
def test_plane_limit(n, uniform, tmp_path):
    """252 rows are 63 groups, the most that 8 planes are used for (a count of 252 <= 255: the carry out of plane 7
    that the tree drops is zero); 253 rows are 64 groups and take 16 planes.  127 -> 128 is here too, on 8 planes."""
    W = T
    at = W + 5 * S + 20
    reads = [(at, "64M", 60)] * 127 + [(at + 10, "54M", 60)] * (n - 128) + [(at + 12, "52M", 60)]
    reads += [(W + 6 * S + 1 + 3 * i, "40M", 60) for i in range(5)]
    reads += [(50 + 40 * i, "150M", 60) for i in range(6)]
    L = 2 * T + 300
    # (max_depth = n - 1: the pileup keeps n reads open, one more than max_depth, and n is EXCESSIVE_COVERAGE)
    (_, qc, _, st, _), lay = check(reads, L, tmp_path, dict(min_depth=128, max_depth=n - 1), ref=_plain_ref(L))
    assert lay["max_groups"] == (n + 3) // 4 and lay["counter_planes"] == (8 if n <= 252 else 16)
    assert qc[at + 9] == 127 and qc[at + 10] == n - 1 and qc[at + 12] == n and qc.max() == n
    assert st[at + 9] == LOW_COVERAGE and st[at + 10] == CALLABLE and st[at + 12] == EXCESSIVE and st[W + 6 * S + 20] == LOW_COVERAGE
