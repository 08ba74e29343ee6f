"""The sparse site pileup on the device (-m gpu): k_site_pileup with site_prepare, site_filter, cl_site_upload,
cl_site_run and cl_site_pileup, on the tiles where such a kernel goes wrong -- unsorted tiles (the wrapped LDS slot and the
global-atomic path), reads of one to six CIGAR operations (the four-word preload and its filler), the SiteRec escapes at
their edges, reads with fewer bases than their CIGAR spends, overhangs, ref_len < contig_len, odd nibble offsets in the
filtered tile, sites at the edges of the 256-position buckets, duplicated sites -- and one tile whose base offsets pass
2^32, through the sparse kernel, the dense scan and the filtered scan.

Every histogram is compared exactly with BOTH tests/site_ref.py (numpy, read by read) and oracle.site_pileup, over three
routes: site_upload + site_run, the one-call site_pileup (which sends only the reads that can count), and the one-call
form with DUT_SITE_FILTER=0 in a child process (the variable is read once per process).  What a case needs of its own
input -- hits below the workgroup's first site, hits beyond the LDS slots, hits in the fifth operation, kept reads at odd
nibbles -- is asserted from site_ref alone before the device is asked, so that no case passes by being empty."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import scan_ref
import site_ref as S
from decodingustools_amd import CallableOptions, Engine, synth

pytestmark = pytest.mark.gpu
QUALITIES = (0, 10, 61)
TESTS = os.path.dirname(os.path.abspath(__file__))


class Case:
    def __init__(self, L, rec, lists, whole=False):
        self.L, self.rec, self.lists, self.whole = L, rec, lists, whole      # whole: the one-call form cannot filter this tile
        self.ref_lens = (L, L - 300)


def _adversarial(i):
    seed, L, n, overhang = S.ADVERSARIAL[i]
    rec = S.adversarial_tile(seed, L, n, overhang)
    return Case(L, rec, S.site_lists(L, rec, seed))


def _edges(order):
    L = 4000
    rec = S.edge_tiles(L)[order]
    return Case(L, rec, S.site_lists(L, rec, 9))


def _shuffled():
    L = 200_000
    rec = S.shuffled_short_reads(L, 30, 41)
    lists = S.site_lists(L, rec, 3)
    assert lists["sparse"].shape[0] == 5000
    lists["stretch"] = np.arange(1, 3001, dtype=np.uint32)
    return Case(L, rec, lists)


def _ladder():
    L = 20_000
    rec = S.ladder_tile(L, 4001, 17)
    return Case(L, rec, S.site_lists(L, rec, 5))


def _escapes():
    L = 90_000
    rec = S.escape_tile()
    return Case(L, rec, S.site_lists(L, rec, 6), whole=True)


def _long_reads():
    L = 90_000
    rec = S.with_random_seq(synth.long_read_contig(L, 6, 77), 78, all_codes=False)
    return Case(L, rec, S.site_lists(L, rec, 7), whole=True)


def _pile():
    L = 3000
    rec = S.pile_tile(70_000)
    lists = S.site_lists(L, rec, 8)
    lists["in-and-out"] = np.array([990, 1000, 1001, 1002, 1025, 1050, 1051, 1052, 2000, 1001], np.uint32)
    return Case(L, rec, lists)


def _odd():
    L = 60_000
    rec = S.odd_length_tile(L, 3000, 21)
    lists = S.site_lists(L, rec, 4)
    lists["half"] = S.half_dropping_list(L, rec, 22)
    return Case(L, rec, lists)


CASES = {"adversarial-1": lambda: _adversarial(0), "adversarial-2": lambda: _adversarial(1), "adversarial-3": lambda: _adversarial(2),
         "adversarial-4": lambda: _adversarial(3), "edges-sorted": lambda: _edges("sorted"), "edges-reversed": lambda: _edges("reversed"),
         "edges-rotated": lambda: _edges("rotated"), "shuffled": _shuffled, "ladder": _ladder, "escapes": _escapes,
         "long-reads": _long_reads, "pile": _pile, "odd-lengths": _odd}


def expectations(case):
    """[(ref_len, min_quality, list name, sites, rows)]: site_ref's rows, which the oracle's must equal."""
    out = []
    for ref_len in case.ref_lens:
        ref = np.full(ref_len, ord("A"), np.uint8)
        for mq in QUALITIES:
            both = S.hist_all(case.L, ref_len, case.rec, mq)
            for name, sites in case.lists.items():
                want = S.rows(both, case.L, ref_len, sites)
                orc = oracle.site_pileup(1, mq, case.L, ref, case.rec, sites)["hist"]
                assert np.array_equal(want, orc), ("the two references differ", ref_len, mq, name)
                out.append((ref_len, mq, name, sites, want))
    return out


def same(got, want, sites, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (what, int(bad.size), int(sites[bad[0]]), got[bad[0]].tolist(), want[bad[0]].tolist())


def tile_bytes(rec):
    """What a whole tile adds to site_pileup_stats' bytes: 4-bit bases, one 16-byte record per read, the CIGAR words."""
    return (int(rec.seq_off[-1]) + 1) // 2 + rec.n * 16 + int(rec.cigar_off[-1]) * 4


def travelled(eng, sites):
    """The bytes of the tile the last site_pileup ran over: its algorithmic bytes less those of the site list."""
    _, nbytes = eng.site_pileup_stats()
    return nbytes - 8 * int(np.count_nonzero(sites)) - 64 * int(sites.shape[0])


def check(case, routes, name=""):
    exp = expectations(case)
    with Engine(CallableOptions(), 0) as eng:
        if "run" in routes:
            last = None
            for ref_len, mq, lname, sites, want in exp:
                if ref_len != last:
                    eng.site_upload(case.L, ref_len, case.rec)
                    last = ref_len
                same(eng.site_run(mq, sites), want, sites, (name, "site_run", ref_len, mq, lname))
        if "call" in routes or "whole" in routes:
            for k, (ref_len, mq, lname, sites, want) in enumerate(exp):
                same(eng.site_pileup(mq, case.L, ref_len, case.rec, sites), want, sites, (name, "site_pileup", ref_len, mq, lname))
                if (case.whole or "whole" in routes) and np.count_nonzero(sites):
                    assert travelled(eng, sites) >= tile_bytes(case.rec), (name, lname, "the whole tile was to travel")
                if "whole" in routes and sites.shape[0]:
                    # DUT_SITE_FILTER=0: the tile that stays behind serves any other list
                    _, _, oname, other, owant = exp[k - 1 if exp[k - 1][:2] == (ref_len, mq) else k + 1]
                    same(eng.site_run(mq, other), owant, other, (name, "site_run after site_pileup", ref_len, mq, lname, oname))


def whole_tile_route(name):
    """The case once more in a child process with DUT_SITE_FILTER=0: the one-call form sends the whole tile."""
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_site_pileup as T\nT.check(T.CASES[%r](), ('whole',), %r)\nprint('WHOLE_TILE_OK')"
            % (TESTS, os.path.dirname(TESTS), name, name))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DUT_SITE_FILTER="0"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "WHOLE_TILE_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])


def duplicated_sites_with_counts(case):
    sites = case.lists["duplicates"]
    h = S.hist_at_sites(case.L, case.L, case.rec, 0, sites)
    vals, cnt = np.unique(sites, return_counts=True)
    return sum(1 for v in vals[cnt > 1].tolist() if h[np.flatnonzero(sites == v)[0]].any())


def input_conditions(name, case):
    """From the reference alone, before the device is asked."""
    L, rec, lists = case.L, case.rec, case.lists
    assert {"every", "sparse", "shuffled", "duplicates", "bucket-edges", "beyond", "ends", "empty"} <= set(lists)
    assert lists["every"].tolist() == list(range(1, L + 51)) and lists["ends"].tolist() == [0, L, L + 1, 2**31]
    assert lists["empty"].shape[0] == 0 and not S.hist_at_sites(L, L, rec, 0, lists["beyond"]).any()
    assert sorted(lists["shuffled"].tolist()) == lists["sparse"].tolist() and lists["shuffled"].tolist() != lists["sparse"].tolist()
    pos0 = lists["bucket-edges"].astype(np.int64) - 1
    assert all(np.isin([256 * b - 1, 256 * b, 256 * b + 1], pos0 + 1).all() for b in range(1, L // 256 + 1)) and 0 in lists["bucket-edges"]
    assert duplicated_sites_with_counts(case) >= 50
    if name.startswith("adversarial"):
        assert S.slot_stats(L, L, rec, 0, lists["every"])["widest"] > S.LDS_SITES
        assert len(set(scan_ref.unpack_seq4(rec.seq4, int(rec.seq_off[-1])).tolist())) == 16
    if name in ("edges-reversed", "edges-rotated"):
        assert S.slot_stats(L, L, rec, 0, lists["every"])["wrapped"] > 0
    if name == "shuffled":
        for lname in ("sparse", "stretch"):
            st = S.slot_stats(L, L, rec, 0, lists[lname])
            assert st["wrapped"] > 0, (lname, st)
        st = S.slot_stats(L, L, rec, 0, lists["sparse"])
        assert st["far"] >= st["groups"] == (rec.n + 255) // 256, st
    if name == "ladder":
        r, _, op = S.hits(L, L, rec, 0, lists["sparse"])
        nops = np.diff(rec.cigar_off.astype(np.int64))
        assert int((op == 4).sum()) > 0 and int((op == 5).sum()) > 0 and set(np.unique(nops).tolist()) == {1, 2, 3, 4, 5, 6}
        assert nops[-1] == 1 and S.hits(L, L, rec, 0, lists["every"])[0].max() == rec.n - 1   # the last read has a hit
    if name == "escapes":
        nops = np.diff(rec.cigar_off.astype(np.int64)); nb = np.diff(rec.seq_off.astype(np.int64))
        assert {254, 255, 300} <= set(nops.tolist()) and {65534, 65535, 70000} <= set(nb.tolist())
    if case.whole:
        assert not S.no_escape(rec) and not S.kept(L, rec, 0, lists["ends"]).all()      # a filter would have dropped reads
    else:
        assert S.no_escape(rec)
    if name == "pile":
        h = S.hist_at_sites(L, L, rec, 0, lists["in-and-out"])
        assert h.sum(1).tolist() == [0, 0, 70_000, 70_000, 70_000, 70_000, 0, 0, 0, 70_000]
    if name == "odd-lengths":
        keep = S.kept(L, rec, 0, lists["half"])
        ln = np.diff(rec.seq_off.astype(np.int64))
        assert int((keep & ((rec.seq_off[:-1] & np.uint64(1)) == 1)).sum()) >= 100
        assert int((keep[1:] & ~keep[:-1] & (ln[:-1] % 2 == 1)).sum()) >= 100
        assert int((ln == 0).sum()) >= 100 and 0.3 * rec.n < int(keep.sum()) < 0.7 * rec.n


@pytest.mark.parametrize("name", list(CASES))
def test_site_pileup_three_routes(name):
    case = CASES[name]()
    input_conditions(name, case)
    check(case, ("run", "call"), name)
    if name == "odd-lengths":
        # the contrast of the whole-tile assertion: here the one-call form leaves half of the reads behind
        with Engine(CallableOptions(), 0) as eng:
            eng.site_pileup(0, case.L, case.L, case.rec, case.lists["half"])
            assert travelled(eng, case.lists["half"]) < 0.8 * tile_bytes(case.rec)
    whole_tile_route(name)


# ---- one tile past 2^32 bases -----------------------------------------------------------------------------------------
def same_scan(got, exp, what):
    assert (got.low_depth, got.mixed, got.uncomparable, got.match, got.variant) == \
        (exp["low_depth"], exp["mixed"], exp["uncomparable"], exp["match"], exp["variant"]), what
    c = got.candidates
    have = [(int(r["pos"]), chr(r["ref"]), chr(r["alt"]), int(r["a"]), int(r["c"]), int(r["g"]), int(r["t"]), int(r["depth"])) for r in c]
    assert have == [tuple(x[:8]) for x in exp["candidates"]], what


def counts5(both):
    return np.concatenate([both[:, [1, 2, 4, 8]], both.sum(1, dtype=np.uint64)[:, None].astype(np.uint32)], axis=1)


class PastTheMark:
    """The input of the test below and everything the reference says about it; the conditions on the input are asserted
    here, from the reference alone."""
    MARK = 1 << 32

    def __init__(self):
        MARK = self.MARK
        L = self.L = 200_000
        ref = self.ref = synth.make_reference(L, 61)
        sample = ref.copy()
        rng = np.random.default_rng(62)
        for p in rng.choice(L, 400, replace=False):
            sample[p] = rng.choice(list(b"ACGT"))
        short = synth.short_read_contig(L, 30, 63, with_seq=True, ref=sample)
        adv = S.adversarial_tile(2, 5000, 1500, True)
        half = short.n // 2
        it = self.it = S.concat([short.slice(0, half), adv, short.slice(half, short.n)])
        ln = np.diff(it.seq_off.astype(np.int64))
        cross = half + adv.n // 2 + int(np.argmax(ln[half + adv.n // 2:] >= 4))
        B = S.ballast_bases(it, cross, MARK)
        buf = S.ballast_buffer(it, B, 64)
        tile, nb = self.tile, self.nb = S.ballast_tile(it, buf, S.ballast_lengths(B, 1_000_000, seed=65), 100_000, 66)
        lists = self.lists = {"sparse": np.sort(rng.choice(np.arange(1, L + 50), 5000, replace=False)).astype(np.uint32),
                              "stretch": np.arange(1, 3001, dtype=np.uint32)}
        lists["shuffled, with duplicates"] = rng.permutation(np.concatenate([lists["sparse"], lists["sparse"][::9]]))
        # a read whose bases lie across the mark, a thousand reads with hits on either side of it
        assert int(tile.seq_off[nb + cross]) < MARK <= int(tile.seq_off[nb + cross + 1]) and 4000 < nb < 4600
        assert int(tile.seq_off[-1]) > MARK + 2_000_000 and int(tile.qual_off[nb]) == 0 and (tile.mapq[:nb] == 5).all()
        hit_reads = np.unique(np.concatenate([S.hits(L, L, it, 10, s)[0] for s in lists.values()]))
        assert int((hit_reads > cross).sum()) >= 1000 and int((hit_reads < cross).sum()) >= 1000
        p_cross = int(it.pos[cross])
        self.ranges = [(0, 2048 + 17), (max(0, p_cross - 700), min(L, p_cross + 900)), (L - 2500, L)]
        assert self.ranges[1][0] <= p_cross < self.ranges[1][1] and adv.n // 2 <= cross - half < adv.n
        self.both = {mq: S.hist_all(L, L, it, mq) for mq in (0, 10)}
        self.filt = {mq: scan_ref.stranded_hist(L, L, it, mq, 0x704, 20) for mq in (0, 10)}
        assert all(int(self.filt[mq].sum()) < int(self.both[mq].sum()) for mq in (0, 10))
        self.share = {a: S.ballast_share(tile, nb, L, L, np.arange(a, b)) for a, b in self.ranges}
        assert all(int(v.sum(1).max()) > 50 for v in self.share.values())                  # the ballast lies over every range
        assert int(self.share[self.ranges[2][0]].sum(1).min()) > 4000
        # the same bases under a ballast of 60 000-base reads, which site_filter gathers: with the ballast kept
        # (min_quality 0) the gathered offsets pass the mark, without it (10) the offsets gathered from do
        tile2, nb2 = self.tile2, self.nb2 = S.ballast_tile(it, buf, S.ballast_lengths(B, 60_000, fixed=True), 100_000, 67)
        sites = self.sites2 = np.sort(rng.choice(np.arange(1, L + 1), 1500, replace=False)).astype(np.uint32)
        assert S.no_escape(tile2) and int(tile2.seq_off[nb2]) == B and nb2 > 70_000
        for mq in (0, 10):
            keep = S.kept(L, tile2, mq, sites)
            s0, s1 = tile2.seq_off[:-1].astype(np.int64), tile2.seq_off[1:].astype(np.int64)
            gathered = np.concatenate([[0], np.cumsum(np.where(keep, ((s1 + 1) >> 1) - (s0 >> 1), 0))]) * 2
            k_it = np.flatnonzero(keep[nb2:])
            assert k_it.shape[0] < it.n and int((s0[nb2:][k_it] >= MARK).sum()) >= 1000 and int((s0[nb2:][k_it] < MARK).sum()) >= 1000
            if mq == 0:
                assert keep[:nb2].all() and int((gathered[nb2:-1][k_it] >= MARK).sum()) >= 1000
            else:
                assert not keep[:nb2].any() and int(gathered[-1]) < MARK // 64

    def rows(self, mq, tile, n_ballast, sites):
        w = S.rows(self.both[mq], self.L, self.L, sites)
        return w + S.ballast_share(tile, n_ballast, self.L, self.L, sites.astype(np.int64) - 1) if mq <= 5 else w


def test_one_tile_past_2_32_bases_through_all_three_kernels():
    """All three kernels address a base as the 64-bit base offset of a group of 256 reads plus a 32-bit difference, and the
    pass bits by bi >> 6.  A ballast of about 4 300 single-M reads of a million random bases each (mapq 5, no quality
    values) puts the offsets of an adversarial contig and a short-read contig around 2^32; min_quality 10 leaves the
    ballast out, 0 counts it.  The reference: site_ref / scan_ref over the interesting reads as a tile of their own, plus
    the ballast's share (site_ref.ballast_share); the oracle over the whole tile agrees with it at the site lists."""
    I = PastTheMark()
    L, ref, tile, nb, lists, ranges, both, filt, share = I.L, I.ref, I.tile, I.nb, I.lists, I.ranges, I.both, I.filt, I.share
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, tile)
        for mq in (0, 10):
            for lname, sites in lists.items():
                want = I.rows(mq, tile, nb, sites)
                assert np.array_equal(want, oracle.site_pileup(1, mq, L, ref, tile, sites)["hist"]), ("the two references differ", mq, lname)
                same(eng.site_run(mq, sites), want, sites, ("site_run", mq, lname))
            for a, b in ranges:
                tot = both[mq][a:b] + (share[a] if mq <= 5 else 0)
                got = eng.site_scan_counts(mq, a, b)
                bad = np.nonzero((got != counts5(tot)).any(1))[0]
                assert bad.size == 0, ("site_scan_counts", mq, (a, b), int(a + bad[0]), got[bad[0]].tolist(), counts5(tot)[bad[0]].tolist())
                h2 = np.zeros((2, L, 16), np.uint32)
                h2[0, a:b] = tot
                for md in (10, 3000):
                    same_scan(eng.site_scan(mq, md, ref, a, b), scan_ref.reduce(h2, ref, L, md, a, b), ("site_scan", mq, md, (a, b)))
        exp10 = scan_ref.reduce(np.stack([both[10], np.zeros_like(both[10])]), ref, L, 10, 0, L)
        assert exp10["variant"] > 100 and exp10["match"] > L // 2                         # the scan has something to call
        same_scan(eng.site_scan(10, 10, ref), exp10, "site_scan, whole contig")
        eng.site_attach_quals(tile, 20)
        for mq in (0, 10):
            for a, b in ranges:
                h2 = filt[mq][:, a:b].copy()
                if mq <= 5:
                    h2[0] += share[a]                                                      # flag 0: forward; no quality value: passes
                got = eng.site_scan_counts_ex(mq, a, b, 0x704, True)
                want = scan_ref.counts9(h2)
                bad = np.nonzero((got != want).any(1))[0]
                assert bad.size == 0, ("site_scan_counts_ex", mq, (a, b), int(a + bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
        # the one-call form: a read of 65 535 bases and more, so the whole tile travels
        for mq in (0, 10):
            sites = lists["sparse"]
            same(eng.site_pileup(mq, L, L, tile, sites), I.rows(mq, tile, nb, sites), sites, ("site_pileup, whole tile", mq))
            assert travelled(eng, sites) >= tile_bytes(tile)
        # ... and the gathered one
        tile2, nb2, sites = I.tile2, I.nb2, I.sites2
        for mq in (0, 10):
            want = I.rows(mq, tile2, nb2, sites)
            assert np.array_equal(want, oracle.site_pileup(1, mq, L, ref, tile2, sites)["hist"]), ("the two references differ", mq)
            same(eng.site_pileup(mq, L, L, tile2, sites), want, sites, ("site_pileup, gathered", mq))
            assert travelled(eng, sites) < tile_bytes(tile2) - (0 if mq == 0 else I.MARK // 4)


# ---- the statistics of the caller's own site pileup survive a scan that runs one ------------------------------------------
class SettledByThePileup:
    """A small tile for site_pileup and the same reads with an ambiguity code (R) planted in every plain read over three
    positions, which the unfiltered scan can only settle through the site pileup's 16-code histogram; what the references
    say of both.  The conditions on the input are asserted here, from the references alone."""

    def __init__(self):
        L = self.L = 4000
        ref = self.ref = synth.make_reference(L, 71)
        rec = self.rec = synth.short_read_contig(L, 15, 72, with_seq=True, ref=ref)
        assert 200 <= rec.n <= 600 and S.no_escape(rec) and not (rec.seq_off & np.uint64(1)).any()
        self.sites = np.array([0, 7, 300, 301, 1024, 1999, 2000, 2500, 3100, 3500, 3990, L + 5], np.uint32)
        keep = S.kept(L, rec, 0, self.sites)
        assert 0 < int(keep.sum()) < rec.n
        # (whole bytes per read: what the one-call form gathers is the tile of the kept reads)
        self.bytes = tile_bytes(S.permuted(rec, np.flatnonzero(keep))) + 8 * int(np.count_nonzero(self.sites)) + 64 * self.sites.shape[0]
        self.want = S.hist_at_sites(L, L, rec, 0, self.sites)
        assert np.array_equal(self.want, oracle.site_pileup(1, 0, L, ref, rec, self.sites)["hist"]) and self.want.any()
        # the planted tile
        planted = self.planted = np.array([700, 1800, 2900])
        codes = scan_ref.unpack_seq4(rec.seq4, int(rec.seq_off[-1])).copy()
        plain = (np.diff(rec.cigar_off.astype(np.int64)) == 1) & ((rec.cigar[rec.cigar_off[:-1]] & 15) == 0)
        for p in planted:
            r = np.flatnonzero(plain & (rec.pos <= p) & (p < rec.pos.astype(np.int64) + 150))
            codes[rec.seq_off[r].astype(np.int64) + (p - rec.pos[r])] = 5
        amb = self.amb = S.permuted(rec, np.arange(rec.n))
        amb.seq4 = S.pack_seq4(codes)
        h = oracle.site_pileup(1, 0, L, ref, amb, (planted + 1).astype(np.uint32))["hist"].astype(np.int64)
        depth = h.sum(1)
        assert (depth >= 5).all() and (10 * h[:, 5] >= 7 * depth).all(), h.tolist()    # R holds 7/10: neither A, C, G, T nor N
        self.exp = scan_ref.reduce(np.stack([S.hist_all(L, L, amb, 0), np.zeros((L, 16), np.uint32)]), ref, L, 1, 0, L)
        clean = scan_ref.reduce(np.stack([S.hist_all(L, L, rec, 0), np.zeros((L, 16), np.uint32)]), ref, L, 1, 0, L)
        assert self.exp["uncomparable"] == clean["uncomparable"] + planted.shape[0]


def test_a_scan_settled_by_the_site_pileup_leaves_the_callers_pileup_stats():
    """cl_site_scan settles the positions its counter planes cannot classify with a run of the site pileup of its own
    (site_scan_hist16).  site_pileup_stats keeps speaking of the caller's last site_pileup all the same -- its kernel time
    and its algorithmic bytes, both exactly -- and site_scan_stats of the scan."""
    I = SettledByThePileup()
    with Engine(CallableOptions(), 0) as eng:
        same(eng.site_pileup(0, I.L, I.L, I.rec, I.sites), I.want, I.sites, "site_pileup")
        ms0, bytes0 = eng.site_pileup_stats()
        assert ms0 > 0 and bytes0 == I.bytes, (ms0, bytes0, I.bytes)
        eng.site_upload(I.L, I.L, I.amb)
        res = eng.site_scan(0, 1, I.ref)
        same_scan(res, I.exp, "site_scan over the planted tile")
        assert res.uncomparable + res.mixed > 0 and res.uncomparable >= I.planted.shape[0]     # the settling path was taken
        assert eng.site_pileup_stats() == (ms0, bytes0)
        assert eng.site_scan_stats()[0] > 0
