"""Seeded inputs of the fingerprint-compare tests.  A sketch is (hashes uint64 ascending, counts uint32, ksize, scaled); a
case is (sketches, pairs).  T is the device kernel's tile: the merged sequence of a pair (ties: the first sketch's element
first) is cut every T elements."""
import numpy as np

import fpc_ref

K = 31
U64 = 2 ** 64


def universe(rng, n, top):
    """n distinct ascending hashes in [0, top]."""
    h = np.unique(rng.integers(0, top, size=n + n // 8 + 16, dtype=np.uint64, endpoint=True))
    while h.size < n:
        h = np.unique(np.concatenate([h, rng.integers(0, top, size=n, dtype=np.uint64, endpoint=True)]))
    return np.sort(rng.choice(h, size=n, replace=False))


def subset(rng, uni, n, scaled=1000, ksize=K, count_hi=50):
    h = np.sort(rng.choice(uni, size=n, replace=False)) if n else np.zeros(0, np.uint64)
    return (h.astype(np.uint64), rng.integers(1, count_hi, size=n, dtype=np.uint32, endpoint=True), ksize, scaled)


def two_of(rng, na, nb, scaled=1000):
    """Two sketches of na and nb entries out of one universe of about na + nb hashes, so that many are shared."""
    uni = universe(rng, max(na + nb - min(na, nb) // 2, 1), fpc_ref.max_hash(scaled))
    return [subset(rng, uni, na, scaled), subset(rng, uni, nb, scaled)]


def merged_layout(rng, total, common_at):
    """Two sketches whose merged sequence (first sketch's element first on a tie) has `total` elements and a common hash
    exactly at the positions p, p + 1 for every p of common_at: the first sketch's element at p, the second's at p + 1."""
    ha, hb = [], []
    v, pos = int(rng.integers(1, 1000)), 0
    starts = set(common_at)
    assert all(p + 1 not in starts and 0 <= p < total - 1 for p in starts)
    while pos < total:
        if pos in starts:
            ha.append(v), hb.append(v)
            pos += 2
        else:
            (ha if rng.random() < 0.5 else hb).append(v)
            pos += 1
        v += int(rng.integers(1, 1 << 40))
    mk = lambda h: (np.array(h, np.uint64), rng.integers(1, 9, size=len(h), dtype=np.uint32, endpoint=True), K, 1000)  # noqa: E731
    return [mk(ha), mk(hb)]


def both_ways(n=2):
    return [(i, j) for i in range(n) for j in range(n)]


def cases(T, seed=29):
    """name -> (sketches, pairs)"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in (T - 1, T, T + 1, 2 * T + 1):
        out[f"both_{n}"] = (two_of(rng, n, n), both_ways())
    out["mixed_3T+5_7"] = (two_of(rng, 3 * T + 5, 7), both_ways())
    out["mixed_T+1_2T-1"] = (two_of(rng, T + 1, 2 * T - 1), both_ways())
    uni = universe(rng, 4 * T, fpc_ref.max_hash(1000))
    empty = subset(rng, uni, 0)
    out["empty_empty"] = ([empty, subset(rng, uni, 0)], both_ways())
    out["empty_T+1"] = ([empty, subset(rng, uni, T + 1)], both_ways())
    one = (np.array([12345], np.uint64), np.array([3], np.uint32), K, 1000)
    out["one_equal"] = ([one, (np.array([12345], np.uint64), np.array([7], np.uint32), K, 1000)], both_ways())
    out["one_unequal"] = ([one, (np.array([12346], np.uint64), np.array([7], np.uint32), K, 1000)], both_ways())
    # seams: a common hash across every boundary of a 4-tile pair (the first sketch's element last in its tile), the same one
    # element earlier and one later, and all three places at once; (1, 0) is the mirror image, the seams at the same places
    for shift in (0, -1, 1):
        out[f"seam_{shift}"] = (merged_layout(rng, 4 * T, [d - 1 + shift for d in (T, 2 * T, 3 * T)]), both_ways())
    out["seam_dense"] = (merged_layout(rng, 4 * T, [d - 1 + s for d in (T, 2 * T, 3 * T) for s in (-2, 0, 2)] + list(range(10, T - 10, 7))),
                         both_ways())
    same = subset(rng, uni, 2 * T + 1)
    out["identical_2T+1"] = ([same, (same[0].copy(), same[1].copy(), K, 1000)], both_ways())
    lowhigh = np.sort(uni)
    below = (lowhigh[:T + 3].copy(), rng.integers(1, 9, size=T + 3, dtype=np.uint32), K, 1000)
    above = (lowhigh[T + 3:3 * T + 4].copy(), rng.integers(1, 9, size=2 * T + 1, dtype=np.uint32), K, 1000)
    out["all_below"] = ([below, above], both_ways())
    ev = np.arange(0, 2 * (T + 5), 2, dtype=np.uint64)
    out["even_odd"] = ([(ev, np.ones(ev.size, np.uint32), K, 1000), (ev + np.uint64(1), np.full(ev.size, 2, np.uint32), K, 1000)], both_ways())
    # unsigned order
    edge = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], np.uint64)
    out["unsigned_edges"] = ([(edge, np.array([1, 2, 3, 4, 5], np.uint32), K, 1), (edge.copy(), np.array([5, 4, 3, 2, 1], np.uint32), K, 1),
                              (edge[[0, 3]].copy(), np.array([9, 9], np.uint32), K, 1), (edge[[2, 4]].copy(), np.array([1, 1], np.uint32), K, 0)],
                             both_ways(4))
    wide = universe(rng, 3 * T, U64 - 1)
    assert (wide >= np.uint64(2 ** 63)).sum() > T // 2
    out["unsigned_random"] = ([subset(rng, wide, T + 700, scaled=1), subset(rng, wide, 2 * T - 3, scaled=1)], both_ways())
    # the cut: two `scaled` values, entries on both sides of the coarser max_hash and one equal to it
    for fine, coarse in ((1000, 3000), (1, 7)):
        mc = fpc_ref.max_hash(coarse)
        u2 = np.unique(np.concatenate([universe(rng, 2 * T, fpc_ref.max_hash(fine)), universe(rng, T, mc), np.array([mc, mc - 1, mc + 1], np.uint64)]))
        pick = lambda n, keep: np.unique(np.concatenate([rng.choice(u2, size=n, replace=False), np.array(keep, np.uint64)]))  # noqa: E731
        a = pick(T + 50, [mc, mc + 1])
        b = pick(T // 2, [mc])
        b = b[b <= np.uint64(mc)]
        c = pick(T, [mc - 1, mc + 1])
        cnt = lambda h: rng.integers(1, 30, size=h.size, dtype=np.uint32)  # noqa: E731
        sk = [(a, cnt(a), K, fine), (b, cnt(b), K, coarse), (c, cnt(c), K, fine)]
        assert (a > np.uint64(mc)).sum() > 10 and (c > np.uint64(mc)).sum() > 10
        out[f"cut_{fine}_{coarse}"] = (sk, both_ways(3))
    # counts at the top of 32 bits on both sides of many common hashes: the sums pass 2^32
    big = subset(rng, uni, T + 100)
    full = np.full(T + 100, 2 ** 32 - 1, np.uint32)
    out["counts_max"] = ([(big[0], full, K, 1000), (big[0].copy(), full.copy(), K, 1000), (big[0][::2].copy(), full[::2].copy(), K, 1000)],
                         both_ways(3))
    return out


def many(T, seed=31, n=40):
    """n small sketches of seeded sizes 0 .. 3T out of one universe: pairs of very different tile counts side by side."""
    rng = np.random.default_rng(seed)
    uni = universe(rng, 4 * T, fpc_ref.max_hash(1000))
    sizes = rng.integers(0, 3 * T, size=n, endpoint=True)
    sizes[:4] = (0, 3 * T, 1, T)
    return [subset(rng, uni, int(s)) for s in sizes]
