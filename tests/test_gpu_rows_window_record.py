"""What k_pileup_rows does once per window (-m gpu): the addresses of its row and head loads, the wave's totals and the
32-byte record they leave for k_tail (kernels.hip.h: WinRecord; tail_summary_rows unpacks it).

  row addresses   unit k of a trip takes k x 128 from the load's immediate offset, the lane's part is k < n ? off : none:
                  segments of different heights, a segment without a unit beside one with more than 12 groups (the
                  second trip), heights of exactly 12 and 13 groups; the same with every segment at the highest one's height
  head addresses  a trip of a window without wide candidates reads slot v as head v of the window's descriptor and leaves
                  the validity to the descriptor: candidate counts around one lane row (64), one trip (512) and two, both
                  head widths; a contig with a read wider than 16 384 positions, whose windows take the general trip
                  beside windows that do not
  packed fields   a window that is wholly one state (a 16-bit half holds exactly 2 048), 252 rows over a whole window (the
                  most 8 planes take: n_cov = 2 048 beside the largest sum_qc in one register), 256 rows (16 planes: sum_qc
                  in a word of its own, max_raw from the general path), more than 32 767 candidates (32-bit differences)
  the ragged end  extents of 2 048 + 1, 31, 32, 33 and 2 047
  the tail        1 025 windows (two summary workgroups), repeated runs on a resident contig, the byte form on a second
                  engine (WinPartial, the other instantiation of k_tail), a contig without a window

Every case holds the BED text, the six state counts and the six summary sums against the oracle, exactly."""
import numpy as np
import pytest

from helpers import make_options, oracle_run
from decodingustools_amd import CallableOptions, CallableProfiler, ContigProfiler, Engine, process_single_contig, synth
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu

T = 2048
SUMS = ("n_covered_bases", "summed_coverage", "summed_baseq", "summed_mapq", "quality_bases", "n_reads")
HOOKS = ("DUT_QUAL_FORM", "DUT_HEADS8", "DUT_ROWS_UNIFORM", "DUT_HEAD_SPAN", "DUT_TAIL_CHUNKS")
A, N = ord("A"), ord("N")
# the states' numbers (types.rs:36-43)
REF_N, CALLABLE, NO_COVERAGE, LOW_COVERAGE, EXCESSIVE_COVERAGE, POOR_MAPPING_QUALITY = range(6)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)


def _opts(d=None):
    o = make_options(d or {})
    return o, CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                              o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def records(*groups):
    """groups: (positions, read length, mapq, base quality) -- reads of one M operation, scalars or one value per read;
    the records in coordinate order, built without a loop over the reads"""
    pos, rl, mq, bq = [], [], [], []
    for p, length, mapq, qual in groups:
        p = np.atleast_1d(np.asarray(p, np.int64))
        pos.append(p)
        for dst, v in ((rl, length), (mq, mapq), (bq, qual)):
            dst.append(np.broadcast_to(np.asarray(v, np.int64), p.shape))
    if not pos:
        return ContigRecords.from_reads([])
    pos, rl, mq, bq = (np.concatenate(x) for x in (pos, rl, mq, bq))
    order = np.argsort(pos, kind="stable")
    pos, rl, mq, bq = pos[order], rl[order], mq[order], bq[order]
    n = pos.shape[0]
    return ContigRecords(
        pos=pos.astype(np.int32), flag=np.zeros(n, np.uint16), mapq=mq.astype(np.uint8),
        cigar_off=np.arange(n + 1, dtype=np.uint32), cigar=(rl << 4).astype(np.uint32),
        qual_off=np.concatenate([[0], np.cumsum(rl)]).astype(np.uint64), qual=np.repeat(bq, rl).astype(np.uint8),
        qname_off=(np.arange(n + 1, dtype=np.uint32) * np.uint32(10)), qname=synth._names_fixed(np.arange(n)).reshape(-1)).validate()


def scattered(rng, n, lo, hi, length=50):
    """n reads of `length` positions that start in [lo, hi), their mapq and base quality mixed"""
    return (np.sort(rng.integers(lo, hi, n)), length, rng.choice([0, 5, 30, 60, 60], n), rng.choice([10, 25, 40], n))


def speckled(length, seed, every=97):
    """a reference of A with an N now and then (a few REF_N runs per window)"""
    ref = np.full(length, A, np.uint8)
    ref[np.random.default_rng(seed).integers(0, length, max(1, length // every))] = N
    return ref


def run_and_check(contigs, tmp_path, env=None, monkeypatch=None, opts=None, after=None):
    """contigs: [(name, tid, length, ref, ContigRecords)] through ONE engine, each held against the oracle: BED text,
    state counts and the six sums.  after(engine, last result, oracle results): further checks, the last contig resident."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    oo, opt = _opts(opts)
    o_res, o_bed = oracle_run(contigs, oo, str(tmp_path / "o.bed"))
    bed = str(tmp_path / ("g%s.bed" % "".join(sorted(env or {}))))
    with Engine(opt, 0) as eng:
        counter = CallableProfiler(bed)
        stats = []
        for name, tid, length, ref, rec in contigs:
            st = ContigProfiler(name, length)
            process_single_contig(eng, counter, st, opt, tid, rec, ref)
            stats.append(st)
        counts = [counter.get_contig_counts(name) for name, *_ in contigs]
        counter.close()
        res = eng.contig_collect()
        if after:
            after(eng, res, o_res)
    for (name, *_), st, cnt in zip(contigs, stats, counts):
        for k in SUMS:
            assert getattr(st, k) == o_res[name]["stats"][k], (name, k)
        assert cnt == o_res[name]["state_counts"], name
    assert open(bed).read() == o_bed and o_bed
    return res


# ---- 1. row addresses: the heights of a window's eight segments ----
# d reads of 100 positions on one start inside a segment are d rows of that segment alone: ceil(d / 4) groups
HEIGHTS = {"mixed_13": (4, 0, 52, 8, 48, 1, 20, 30),     # none beside 13 groups (the second trip), 12 beside it
           "top_12": (48, 0, 4, 47, 45, 0, 0, 1),        # the highest segment fills the first trip exactly
           "top_13": (49, 0, 0, 0, 0, 0, 0, 48),         # one row into the second trip
           "all_13": (52,) * 8}


@pytest.mark.parametrize("uniform", (False, True), ids=("own_heights", "uniform"))
@pytest.mark.parametrize("which", sorted(HEIGHTS))
def test_segment_heights(which, uniform, tmp_path, monkeypatch):
    depths = HEIGHTS[which]
    L = 3 * T + 77
    # window 1 carries the stacks; window 0 and 2 a few reads of their own (other heights in the same launch)
    groups = [(np.full(d, T + 256 * s + 10), 100, 60, 30) for s, d in enumerate(depths) if d]
    rng = np.random.default_rng(3)
    groups += [scattered(rng, 40, 0, T - 200), scattered(rng, 90, 2 * T + 60, L - 60)]

    def after(eng, res, o):
        lay = eng.contig_layout()
        assert lay["form"] == 3 and lay["counter_planes"] == 8 and lay["max_groups"] == (max(depths) + 3) // 4

    run_and_check([("chrR", 0, L, speckled(L, 1), records(*groups))], tmp_path,
                  {"DUT_ROWS_UNIFORM": "1"} if uniform else None, monkeypatch, after=after)


# ---- 2. head addresses: candidates per window around a lane row, one trip and two ----
@pytest.mark.parametrize("heads8", (False, True), ids=("heads4", "heads8"))
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 511, 512, 513, 1025))
def test_candidate_counts(n, heads8, tmp_path, monkeypatch):
    """n reads of 50 positions inside window 1, none within 50 of its ends: window 1 has exactly n candidates, its
    neighbours none (window 3 has three of its own)"""
    L = 4 * T
    rng = np.random.default_rng(n)
    groups = [scattered(rng, n, T + 100, 2 * T - 100)] if n else []
    groups.append(([3 * T + 5, 3 * T + 5, 3 * T + 900], 50, 60, 30))
    run_and_check([("chrH", 0, L, speckled(L, 2), records(*groups))], tmp_path, {"DUT_HEADS8": "1"} if heads8 else None, monkeypatch)


def test_wide_read_beside_plain_windows(tmp_path):
    """A read of 20 000 positions (wider than kWideSpan = 16 384) from position 300: windows 0..9 have a wide candidate and
    take the general trip, windows 10..12 have none; a second one starts in window 5.  The contig keeps 8-byte heads."""
    L = 13 * T - 5
    rng = np.random.default_rng(8)
    groups = [([300], 20000, 60, 30), ([5 * T + 9], 16385, 0, 30), scattered(rng, 700, 0, L - 50), scattered(rng, 600, 10 * T + 100, 11 * T - 100)]
    run_and_check([("chrW", 0, L, speckled(L, 3), records(*groups))], tmp_path)


# ---- 3. the packed fields at their ends ----
# (reference base of window 1, the reads' groups, options).  Reads over a whole window start in front of it; the pileup
# admits no more than max_depth reads per START, so the six of EXCESSIVE_COVERAGE take six starts
WHOLE = {REF_N: (N, [], None), NO_COVERAGE: (A, [], None),
         CALLABLE: (A, [(np.full(4, T - 1), T + 1, 60, 30)], None),
         LOW_COVERAGE: (A, [(np.full(2, T - 1), T + 1, 60, 30)], None),
         EXCESSIVE_COVERAGE: (A, [(T - 10 + np.arange(6), T + 10 - np.arange(6), 60, 30)], dict(max_depth=2, min_depth=1)),
         POOR_MAPPING_QUALITY: (A, [(np.full(12, T - 1), T + 1, 0, 30)], None)}


@pytest.mark.parametrize("state", sorted(WHOLE))
def test_window_of_one_state(state, tmp_path):
    """The last window of the contig is wholly `state`: a count of exactly 2 048 in its half of a register"""
    base, groups, opts = WHOLE[state]
    ref = np.full(2 * T, A, np.uint8)
    ref[T:] = base

    def after(eng, res, o):
        assert o["chrS"]["state_counts"][state] >= T

    run_and_check([("chrS", 0, 2 * T, ref, records(*groups))], tmp_path, opts=opts, after=after)


@pytest.mark.parametrize("rows,planes", ((252, 8), (256, 16)))
def test_full_window_of_rows(rows, planes, tmp_path):
    """`rows` passing reads over the whole of window 1 (on four starts in front of it, below the pileup's cap per start):
    n_cov = 2 048 and sum_qc = rows x 2 048 in the window's record"""
    L = 3 * T
    groups = [(np.repeat(T - 4 + np.arange(4), rows // 4), T + 4, 60, 30)]

    def after(eng, res, o):
        lay = eng.contig_layout()
        assert lay["counter_planes"] == planes and lay["max_groups"] == rows // 4
        assert o["chrF"]["stats"]["quality_bases"] == rows * (T + 4) and int(res.summary.max_raw_depth) == rows

    run_and_check([("chrF", 0, L, np.full(L, A, np.uint8), records(*groups))], tmp_path, opts=dict(max_depth=1000), after=after)


def test_more_than_32767_candidates(tmp_path):
    """33 000 reads of 40 positions in one window: the differences take 32-bit words (DEEP), the depths 16 planes"""
    L = 3 * T
    rng = np.random.default_rng(12)
    n = 33_000
    groups = [(np.sort(rng.integers(T + 100, 2 * T - 100, n)), 40, rng.choice([0, 20, 60, 60], n), rng.choice([5, 25, 40], n))]

    def after(eng, res, o):
        assert int(res.summary.max_raw_depth) > 255

    run_and_check([("chrD", 0, L, speckled(L, 4), records(*groups))], tmp_path, opts=dict(max_depth=100000), after=after)


# ---- 4. the ragged end ----
@pytest.mark.parametrize("over", (1, 31, 32, 33, 2047))
def test_ragged_end(over, tmp_path):
    L = T + over
    rng = np.random.default_rng(over)
    groups = [scattered(rng, 200, 0, L - 20, length=20), ([L - 20] * 5, 20, 60, 30)]
    ref = speckled(L, 5, every=40)
    run_and_check([("chrE", 0, L, ref, records(*groups))], tmp_path)


# ---- 5. the record through the tail ----
def _long_contig():
    L = 1024 * T + 33
    rng = np.random.default_rng(21)
    return ("chrL", 0, L, speckled(L, 6, every=700), records(scattered(rng, 3000, 0, L - 100, length=100)))


def test_two_summary_workgroups_repeated_runs_and_the_byte_form(tmp_path, monkeypatch):
    """1 025 windows: the summary takes two workgroups.  Three more runs on the resident contig leave the same bytes; a
    second, short contig follows on the same engine; a second engine in the byte form (WinPartial) agrees with both."""
    long_c = _long_contig()
    rng = np.random.default_rng(22)
    l2 = 2 * T + 700
    short_c = ("chrM", 1, l2, speckled(l2, 7), records(scattered(rng, 150, 0, l2 - 50)))

    def resident(eng, first, o):
        assert eng.contig_layout()["n_windows"] == 1025
        for _ in range(3):
            eng.contig_run()
        again = eng.contig_collect()
        assert again.as_dict() == first.as_dict()
        assert again.intervals.tobytes() == first.intervals.tobytes()

    rows_long = run_and_check([long_c], tmp_path, after=resident)

    def form_is(form):
        def after(eng, res, o):
            assert eng.contig_layout()["form"] == form
        return after

    rows_both = run_and_check([long_c, short_c], tmp_path, after=form_is(3))
    bytes_both = run_and_check([long_c, short_c], tmp_path, {"DUT_QUAL_FORM": "bytes"}, monkeypatch, after=form_is(0))
    assert rows_both.as_dict() == bytes_both.as_dict() and rows_both.intervals.tobytes() == bytes_both.intervals.tobytes()
    assert int(rows_long.summary.extent) == long_c[2] and int(rows_both.summary.extent) == l2


def test_contig_without_a_window(tmp_path):
    _, opt = _opts()
    with Engine(opt, 0) as eng:
        eng.contig_begin(0, 0, None)
        res = eng.contig_finish()
        assert res.intervals.shape[0] == 0 and eng.contig_layout()["n_windows"] == 0
        assert res.as_dict() == dict(state_counts=[0] * 6, n_covered_bases=0, summed_coverage=0, summed_baseq=0, summed_mapq=0,
                                     quality_bases=0, extent=0, max_raw_depth=0, n_intervals=0)
        # ... and a contig with windows behind it on the same engine
        eng.contig_begin(1, T + 5, np.full(T + 5, N, np.uint8))
        res = eng.contig_finish()
        assert res.as_dict()["state_counts"] == [T + 5, 0, 0, 0, 0, 0] and int(res.summary.n_intervals) == 1
