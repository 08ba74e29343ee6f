"""k_tail, the one launch behind the pileup (-m gpu): a workgroup owns a chunk of `wpc` consecutive windows, sums the runs
of every window before its chunk from the windows' packed words (n_inner | first state << 16 | last state << 24) and
writes its windows' intervals; the last chunk stores the number of intervals, and a few workgroups in front of the grid
add the windows' totals to the contig summary with atomics (tail_summary).  The cases sit where that can go
wrong: the chunk borders (the seam run, the run that is closed across the border), window counts around one and two
chunks, wpc > 64 with a ragged last chunk (DUT_TAIL_CHUNKS), run lists beyond the 64 entries a wave requests ahead, an
interval buffer that has to grow (the tail alone runs again: the summary starts over), repeated runs on a resident
contig (the start values are rewritten by every run), a second contig on the same engine, both head forms, the byte
form, and a contig without a window.

The references are built so that the states are known without reads: where N and A alternate every position is a run
(2 047 inner runs and a seam per window), a stretch of A alone has none.  Every case holds the BED text, the state counts
and the six summary fields against the oracle, exactly."""
import numpy as np
import pytest

from helpers import make_options, oracle_run
from decodingustools_amd import CallableOptions, CallableProfiler, ContigProfiler, Engine, process_single_contig
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu

T = 2048
SUMS = ("n_covered_bases", "summed_coverage", "summed_baseq", "summed_mapq", "quality_bases", "n_reads")
HOOKS = ("DUT_QUAL_FORM", "DUT_HEADS8", "DUT_ROWS_UNIFORM", "DUT_HEAD_SPAN", "DUT_TAIL_CHUNKS")
A, N = ord("A"), ord("N")
WAYS = ("seam_no_inner", "same_state", "full_both", "none")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)


def _opts():
    o = make_options({})
    return o, CallableOptions(o.min_depth, o.max_depth, o.min_mapping_quality, o.min_base_quality,
                              o.min_depth_for_low_mapq, o.max_low_mapq, o.max_low_mapq_fraction)


def wpc_of(n_win, max_chunks=512):
    """callable_loci.hip: tail_wpc"""
    if (n_win + 63) // 64 <= max_chunks:
        return 64
    per = (n_win + max_chunks - 1) // max_chunks
    return min((per + 15) // 16 * 16, 4096)


def alternating(n):
    """N at the even offsets, A at the odd ones: a run boundary at every position, the last position (n even) an A"""
    a = np.full(n, A, dtype=np.uint8)
    a[0::2] = N
    return a


def make_ref(n_win, length, borders, way):
    """A reference of `length` positions over n_win windows.  Background: all A, and in window k (k * 7) % 5 single N's
    (two inner runs each), so that the windows' run counts differ.  At every border b in `borders` (between windows
    b - 1 and b) the two windows are laid out `way`:
      seam_no_inner  A...A | N...N       a seam run, no inner run on either side
      same_state     NANA...NA | A...A   no seam (A on both sides), 2 047 inner runs on the left, none on the right
      full_both      NANA...NA | NANA..  a seam and 2 047 inner runs on both sides
      none           A...A | A...A       no seam, no inner run"""
    ref = np.full(n_win * T, A, dtype=np.uint8)
    for k in range(n_win):
        for j in range((k * 7) % 5):
            ref[k * T + 100 + 10 * j] = N
    for b in borders:
        if not 0 < b < n_win:
            continue
        lo, hi = slice((b - 1) * T, b * T), slice(b * T, (b + 1) * T)
        if way == "seam_no_inner":
            ref[lo], ref[hi] = A, N
        elif way == "same_state":
            ref[lo], ref[hi] = alternating(T), A
        elif way == "full_both":
            ref[lo], ref[hi] = alternating(T), alternating(T)
        else:
            ref[lo], ref[hi] = A, A
    return ref[:length].copy()


def make_reads(length, keep_out, n=300, seed=5):
    """A few hundred short reads (states other than REF_N and NO_COVERAGE), none touching a window of `keep_out`"""
    if length < 3 * T:
        return []
    rng = np.random.default_rng(seed)
    reads = []
    for p in np.sort(rng.integers(0, length - 100, n)):
        if int(p) // T in keep_out or (int(p) + 99) // T in keep_out:
            continue
        reads.append((int(p), "100M", int(rng.choice([5, 30, 60, 60])), int(rng.choice([10, 25, 40])), 0, f"s{len(reads)}"))
    return reads


def run_and_check(contigs, tmp_path, env=None, monkeypatch=None, after=None):
    """contigs: [(name, tid, length, ref, reads)] through ONE engine, each held against the oracle: BED text, state counts
    and the six sums.  after(engine, last result): further checks on the engine with the last contig resident."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    oo, opt = _opts()
    recs = [(name, tid, length, ref, ContigRecords.from_reads(reads)) for name, tid, length, ref, reads in contigs]
    o_res, o_bed = oracle_run(recs, oo, str(tmp_path / "o.bed"))
    bed = str(tmp_path / "g.bed")
    with Engine(opt, 0) as eng:
        counter = CallableProfiler(bed)
        stats = []
        for name, tid, length, ref, rec in recs:
            st = ContigProfiler(name, length)
            process_single_contig(eng, counter, st, opt, tid, rec, ref)
            stats.append(st)
        counts = [counter.get_contig_counts(name) for name, *_ in recs]
        counter.close()
        res = eng.contig_collect()
        if after:
            after(eng, res)
    for (name, *_), st, cnt in zip(recs, stats, counts):
        for k in SUMS:
            assert getattr(st, k) == o_res[name]["stats"][k], (name, k)
        assert cnt == o_res[name]["state_counts"], name
    assert open(bed).read() == o_bed and o_bed
    return res


def border_case(n_win, length, way, borders, tmp_path, env=None, monkeypatch=None, after=None):
    ref = make_ref(n_win, length, borders, way)
    keep_out = {b - 1 for b in borders} | set(borders)
    return run_and_check([("chrT", 0, length, ref, make_reads(length, keep_out))], tmp_path, env, monkeypatch, after)


def _lengths(n_win):
    """a multiple of the window, and 156 positions past one"""
    return (n_win * T, (n_win - 1) * T + 156)


# ---- 1. window counts around one and two chunks of 64; the chunk borders 63|64 and 127|128 four ways ----
# (the same ways at the window borders 0|1 and 61|62 inside a chunk; the counts without a chunk border get two of them)
CASE1 = [(n, full, way) for n in (65, 128, 129) for full in (True, False) for way in WAYS] + \
        [(n, full, way) for n in (1, 2, 63, 64) for full in (True, False) for way in ("seam_no_inner", "full_both")]


@pytest.mark.parametrize("n_win,full,way", CASE1)
def test_window_counts_and_chunk_borders(n_win, full, way, tmp_path):
    length = _lengths(n_win)[0 if full else 1]
    def after(eng, res):
        lay = eng.contig_layout()
        assert (lay["tail_wpc"], lay["tail_chunks"]) == (64, (n_win + 63) // 64)

    res = border_case(n_win, length, way, (1, 62, 64, 128), tmp_path, after=after)
    assert int(res.summary.extent) == length and wpc_of(n_win) == 64


# ---- 2. wpc > 64 and a ragged last chunk ----
@pytest.mark.parametrize("chunks,n_win,way", [(c, n, way) for c in (2, 3) for n in (200, 201) for way in WAYS])
def test_wide_chunks_under_the_hook(chunks, n_win, way, tmp_path, monkeypatch):
    wpc = wpc_of(n_win, chunks)
    assert wpc == {2: 112, 3: 80}[chunks] and n_win % wpc != 0            # waves loop over 7 or 5 windows; the last chunk is short
    borders = tuple(range(wpc, n_win, wpc))

    def after(eng, res):                                                 # the engine took the hook: what it launches
        lay = eng.contig_layout()
        assert (lay["tail_wpc"], lay["tail_chunks"]) == (wpc, (n_win + wpc - 1) // wpc) and lay["tail_chunks"] == chunks

    border_case(n_win, (n_win - 1) * T + 156, way, borders, tmp_path, {"DUT_TAIL_CHUNKS": str(chunks)}, monkeypatch, after)


# ---- 3. run lists beyond the first 64 entries ----
@pytest.mark.parametrize("k", (65, 128, 2047))
@pytest.mark.parametrize("behind", (False, True))
def test_long_run_lists(k, behind, tmp_path):
    """one window with k inner runs, alone and as the first window of the second chunk behind 64 windows without any"""
    n_win = 65 if behind else 1
    ref = np.full(n_win * T, A, dtype=np.uint8)
    w = ref[(n_win - 1) * T:]
    w[1:k + 1:2] = N                                                     # boundaries at offsets 1 .. k
    if k % 2:
        w[k:] = N
    assert int(np.count_nonzero(w[1:] != w[:-1])) == k
    run_and_check([("chrT", 0, n_win * T, ref, [])], tmp_path)


# ---- 4. more intervals than the interval buffer holds ----
@pytest.mark.parametrize("n_win", (513, 577))
def test_interval_buffer_grows(n_win, tmp_path):
    """513 windows of alternating N: 513 x 2 048 intervals, more than the 2^20 the first buffer is asked for.  The buffer
    is allocated with an eighth and 64 elements of slack (engine_base.hip.h: DevBuf::reserve), which 513 windows do not
    exceed: 577 windows do, cl_contig_collect grows the buffer and launches the tail alone again.  A second collect
    returns the same summary (the tail accumulates: the record started over)."""
    n_iv = n_win * T
    assert n_iv > 1 << 20 and (n_win == 513 or n_iv > (1 << 20) + (1 << 20) // 8 + 64)

    def after(eng, res):
        again = eng.contig_collect()
        assert again.as_dict() == res.as_dict()
        assert np.array_equal(again.intervals, res.intervals)

    res = run_and_check([("chrT", 0, n_iv, alternating(n_iv), [])], tmp_path, after=after)
    assert int(res.summary.n_intervals) == n_iv == res.intervals.shape[0]
    assert np.array_equal(res.intervals[:, 0], np.arange(n_iv)) and np.array_equal(res.intervals[:, 1], np.arange(1, n_iv + 1))


# ---- 5. the start values are rewritten by every run ----
def test_repeated_runs_on_a_resident_contig(tmp_path):
    def after(eng, first):
        for _ in range(3):
            eng.contig_run()
        again = eng.contig_collect()
        assert again.as_dict() == first.as_dict()
        assert np.array_equal(again.intervals, first.intervals)

    border_case(129, 128 * T + 156, "full_both", (64, 128), tmp_path, after=after)


# ---- 6. a second, different contig on the same engine carries its own host sums and extent ----
def test_second_contig_on_the_same_engine(tmp_path):
    l1, l2 = 66 * T + 156, 3 * T + 700
    c1 = ("chrA", 0, l1, make_ref(67, l1, (64,), "full_both"), make_reads(l1, {63, 64}, seed=5))
    c2 = ("chrB", 1, l2, make_ref(4, l2, (1,), "seam_no_inner"), make_reads(l2, {0, 1}, n=120, seed=9))
    res = run_and_check([c1, c2], tmp_path)
    assert int(res.summary.extent) == l2


# ---- 7. the 65-window contig in the byte form and with 8-byte heads ----
@pytest.mark.parametrize("env", ({"DUT_QUAL_FORM": "bytes"}, {"DUT_HEADS8": "1"}), ids=("bytes", "heads8"))
@pytest.mark.parametrize("way", WAYS)
def test_other_pileup_forms(env, way, tmp_path, monkeypatch):
    def after(eng, res):
        assert eng.contig_layout()["form"] == (0 if "DUT_QUAL_FORM" in env else 3)

    border_case(65, 64 * T + 156, way, (1, 63, 64), tmp_path, env, monkeypatch, after)


# ---- 8. a contig without a window ----
def test_zero_length_contig(tmp_path):
    """A contig of length 0 without reads has no window: no pileup is launched and the summary is its start values (the
    engine before the single tail launch returned the same: nothing counted, no interval, extent 0)."""
    _, opt = _opts()
    with Engine(opt, 0) as eng:
        eng.contig_begin(0, 0, None)
        res = eng.contig_finish()
        assert res.intervals.shape[0] == 0
        assert res.as_dict() == dict(state_counts=[0] * 6, n_covered_bases=0, summed_coverage=0, summed_baseq=0, summed_mapq=0,
                                     quality_bases=0, extent=0, max_raw_depth=0, n_intervals=0)
        assert eng.contig_layout()["n_windows"] == 0
        # ... and the engine goes on: a contig with windows behind it
        eng.contig_begin(1, T + 156, alternating(2 * T)[:T + 156])
        res = eng.contig_finish()
        assert int(res.summary.n_intervals) == T + 156 == res.intervals.shape[0] and int(res.summary.extent) == T + 156
