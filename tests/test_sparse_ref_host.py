"""tests/sparse_ref.py against the dense references (no device): the same runs and the same profile as tests/runs_ref.py and
tests/depth_ref.py give for the per-position depth, which is built here one read at a time."""
import numpy as np
import pytest

import depth_ref
import runs_ref
import sparse_ref

EDGE_SETS = (None, [1], [1, 4, 100], [2, 3, 5, 17])


def dense(start, end, extent):
    d = np.zeros(extent, np.uint64)
    for s, e in zip(start, end):
        d[s:min(e, extent)] += np.uint64(1)                        # (an empty slice where s >= extent)
    return d


def reads(seed, L, n, max_len, overhang):
    """random reads with what the breakpoints could get wrong: shared starts, shared ends, abutting pairs (an end that is
    another read's start), nested reads, and with `overhang` reads that end, or lie, beyond L"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, L, n)
    ln = rng.integers(1, max_len + 1, n)
    e = s + ln
    k = n // 5
    s[:k] = e[k:2 * k]                                              # abutting
    e[:k] = s[:k] + ln[:k]
    s[2 * k:3 * k] = s[3 * k:4 * k] + ln[3 * k:4 * k] // 4          # nested
    e[2 * k:3 * k] = np.maximum(s[2 * k:3 * k] + 1, e[3 * k:4 * k] - ln[3 * k:4 * k] // 4)
    if not overhang:
        e = np.minimum(e, L)
        s = np.minimum(s, e - 1)
    keep = rng.random(n) < 0.5                                      # every other read passes: the qc depth differs
    return s, e, keep


def same(s, e, keep, extent, profiles):
    d_raw, d_qc = dense(s, e, extent), dense(s[keep], e[keep], extent)
    for edges in EDGE_SETS:
        for d, (a, b) in ((d_raw, (s, e)), (d_qc, (s[keep], e[keep]))):
            exp_s, exp_v = runs_ref.runs(d, edges)
            got_s, got_v = sparse_ref.runs(a, b, extent, edges)
            assert got_s.dtype == exp_s.dtype and got_v.dtype == exp_v.dtype
            assert np.array_equal(got_s, exp_s) and np.array_equal(got_v, exp_v), (extent, edges)
    for nb, S in profiles:
        exp = depth_ref.profile(d_raw, d_qc, nb, S)
        got = sparse_ref.profile((s, e), (s[keep], e[keep]), extent, nb, S)
        assert sorted(got) == sorted(exp), (nb, S)
        for key, v in exp.items():
            if isinstance(v, np.ndarray):
                assert got[key].dtype == v.dtype and np.array_equal(got[key], v), (extent, nb, S, key)
            else:
                assert got[key] == v and type(got[key]) is type(v), (extent, nb, S, key)


def profiles_for(extent):
    """S of 16, values that do not divide the extent, one that does where there is one, and extent + 1"""
    S = {0, 16, 2049, 500, extent + 1} | ({extent // 5} if extent % 5 == 0 and extent >= 80 else set())
    return [(nb, w) for nb in (2, 17, 1001) for w in sorted(S) if w == 0 or w >= 16]


@pytest.mark.parametrize("seed,L,n,max_len,overhang", [
    (1, 50_000, 3000, 300, False), (2, 50_000, 3000, 300, True), (3, 7777, 4000, 40, True), (4, 4096, 300, 5000, True),
    (5, 100_003, 500, 200, False), (6, 17, 40, 30, True), (7, 1, 5, 3, True)])
def test_random_reads(seed, L, n, max_len, overhang):
    s, e, keep = reads(seed, L, n, max_len, overhang)
    assert np.intersect1d(s, e).size or n < 10                      # abutting reads are among them
    assert not overhang or int(e.max()) > L
    for extent in sorted({L, max(L, int(e.max()))}):                # clipped at the contig's length, and the engine's extent
        same(s, e, keep, extent, profiles_for(extent))


def test_by_hand():
    s, e = np.array([5, 5, 10, 20, 20, 3]), np.array([10, 8, 20, 25, 22, 30])
    keep = np.array([True, False, True, True, False, False])
    #             0  3  5  8  10 20 22 25  30
    pts, d = sparse_ref.depth(s, e, 40)
    assert pts.tolist() == [0, 3, 5, 8, 10, 20, 22, 25, 30] and d.tolist() == [0, 1, 3, 2, 2, 3, 2, 1, 0]
    assert [a.tolist() for a in sparse_ref.runs(s, e, 40)] == [[0, 3, 5, 8, 20, 22, 25, 30], [0, 1, 3, 2, 3, 2, 1, 0]]
    assert [a.tolist() for a in sparse_ref.runs(s, e, 40, [2])] == [[0, 5, 25], [0, 1, 0]]
    assert [a.tolist() for a in sparse_ref.runs(s, e, 21)] == [[0, 3, 5, 8, 20], [0, 1, 3, 2, 3]]   # nothing at or behind the extent
    p = sparse_ref.profile((s, e), (s[keep], e[keep]), 40, 3, 16)
    assert p["hist_raw"].tolist() == [13, 7, 20] and p["sum_raw"] == 2 + 9 + 24 + 6 + 6 + 5 == int(p["win_raw"].sum())
    assert p["win_raw"].tolist() == [2 + 9 + 4 + 12, 8 + 6 + 6 + 5, 0] and p["n_windows"] == 3
    assert p["hist_qc"].tolist() == [20, 20, 0] and p["win_qc"].tolist() == [11, 9, 0]
    same(s, e, keep, 40, profiles_for(40))
    same(s, e, keep, 21, profiles_for(21))


def test_no_reads_and_no_positions():
    none = np.zeros(0, np.int64)
    keep = np.zeros(0, bool)
    for extent in (5000, 16, 1):
        same(none, none, keep, extent, profiles_for(extent))
        assert [a.tolist() for a in sparse_ref.runs(none, none, extent, [1, 4])] == [[0], [0]]
    same(none, none, keep, 0, [(2, 0), (17, 16)])
    assert sparse_ref.runs(none, none, 0)[0].shape == (0,)
    # reads, but none of them below the extent
    same(np.array([10, 12]), np.array([15, 20]), np.array([True, False]), 10, profiles_for(10))
