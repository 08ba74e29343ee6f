"""tests/site_ref.py tied to the committed oracle, without a device: hist_at_sites against oracle.site_pileup on every
tile shape and site list of tests/test_gpu_site_pileup.py at small size and on the site KATs, the oracle's own contract on
duplicated and far-away sites, and the conditions the device tests put on their inputs (a case must not pass by being
empty), computed from the reference alone."""
import numpy as np
import pytest

import oracle
import site_ref as S
from helpers import load_kats
from decodingustools_amd import synth
from decodingustools_amd.records import ContigRecords

KATS = load_kats()


def tie(L, rec, lists, qualities=(0, 10, 61), ref_lens=None, what=""):
    for ref_len in (ref_lens or (L, L - 300)):
        ref = np.full(ref_len, ord("A"), np.uint8)
        for mq in qualities:
            both = S.hist_all(L, ref_len, rec, mq)
            for name, sites in lists.items():
                want = oracle.site_pileup(1, mq, L, ref, rec, sites)["hist"]
                got = S.rows(both, L, ref_len, sites)
                bad = np.nonzero((got != want).any(1))[0]
                assert bad.size == 0, (what, ref_len, mq, name, int(sites[bad[0]]), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("case", KATS["site_cases"], ids=[c["name"] for c in KATS["site_cases"]])
def test_reference_equals_the_oracle_on_site_kats(case):
    rec = ContigRecords.from_reads([tuple(r) for r in case["reads"]])
    L = case["contig_len"]
    sites = np.asarray(case["sites"], np.uint32)
    tie(L, rec, {"kat": sites, "kat twice": np.concatenate([sites, sites[::-1]])}, (0, case["min_quality"], 61), (len(case["ref"]),), case["name"])


@pytest.mark.parametrize("seed,L,n,overhang", S.ADVERSARIAL)
def test_adversarial_tiles(seed, L, n, overhang):
    rec = S.adversarial_tile(seed, L, n, overhang)
    lists = S.site_lists(L, rec, seed)
    tie(L, rec, lists, what=("adversarial", seed))
    # the every-position list makes some workgroup hit more sites than it keeps in LDS
    assert S.slot_stats(L, L, rec, 0, lists["every"])["widest"] > S.LDS_SITES
    dup_ok(L, rec, lists["duplicates"])


def dup_ok(L, rec, sites, mq=0):
    """>= 50 sites entered more than once whose row is not zero, every entry with the same row."""
    h = S.hist_at_sites(L, L, rec, mq, sites)
    vals, cnt = np.unique(sites, return_counts=True)
    twice = vals[cnt > 1]
    nz = [v for v in twice.tolist() if h[np.flatnonzero(sites == v)[0]].any()]
    assert len(nz) >= 50, len(nz)
    for v in nz:
        i = np.flatnonzero(sites == v)
        assert (h[i] == h[i[0]]).all()


@pytest.mark.parametrize("order", ["sorted", "reversed", "rotated"])
def test_edge_reads(order):
    L = 4000
    rec = S.edge_tiles(L)[order]
    lists = S.site_lists(L, rec, 9)
    tie(L, rec, lists, (0, 20, 61), (L, L - 100), ("edges", order))
    st = S.slot_stats(L, L, rec, 0, lists["every"])
    assert (st["wrapped"] > 0) == (order != "sorted"), st
    dup_ok(L, rec, lists["duplicates"])


def test_shuffled_short_reads():
    L = 20_000
    rec = S.shuffled_short_reads(L, 30, 41)
    lists = S.site_lists(L, rec, 3)
    lists["stretch"] = np.arange(1, 3001, dtype=np.uint32)
    tie(L, rec, lists, (0, 20), what="shuffled")
    st = S.slot_stats(L, L, rec, 0, lists["sparse"])
    assert st["wrapped"] > 0 and st["far"] >= st["groups"], st


def test_ladder_of_operation_counts():
    L = 6000
    rec = S.ladder_tile(L, 1200, 17)
    lists = S.site_lists(L, rec, 5)
    tie(L, rec, lists, what="ladder")
    _, _, op = S.hits(L, L, rec, 0, lists["sparse"])
    assert int((op >= 4).sum()) > 0 and int((op == 5).sum()) > 0 and int((op == 0).sum()) > 0
    # the reads of two, three and four operations have no reference span: nothing of theirs counts
    r, _, _ = S.hits(L, L, rec, 0, lists["every"])
    nops = np.diff(rec.cigar_off.astype(np.int64))
    assert set(np.unique(nops[r]).tolist()) == {1, 5, 6}


def test_escape_shapes_at_small_size():
    rec = S.escape_tile(scale=0.02)
    L = 3000
    lists = S.site_lists(L, rec, 6)
    tie(L, rec, lists, (0, 40), what="escapes")
    assert int(np.diff(rec.cigar_off.astype(np.int64)).max()) == 300 and not S.no_escape(rec)
    L = 9000
    lr = S.with_random_seq(synth.long_read_contig(L, 6, 77), 78, all_codes=False)
    tie(L, lr, S.site_lists(L, lr, 7), (0, 20), what="long reads")


def test_deep_pile_at_small_size():
    L = 3000
    rec = S.pile_tile(700)
    lists = S.site_lists(L, rec, 8)
    tie(L, rec, lists, (20,), what="pile")
    h = S.hist_at_sites(L, L, rec, 20, np.array([1000, 1001, 1050, 1051], np.uint32))
    assert h.sum(1).tolist() == [0, 700, 700, 0]
    dup_ok(L, rec, lists["duplicates"])


def odd_conditions(L, rec, sites, mq):
    """(kept reads with an odd base offset, kept reads that directly follow a dropped read of odd length)."""
    keep = S.kept(L, rec, mq, sites)
    ln = np.diff(rec.seq_off.astype(np.int64))
    odd_off = keep & ((rec.seq_off[:-1] & np.uint64(1)) == 1)
    after = keep[1:] & ~keep[:-1] & (ln[:-1] % 2 == 1)
    return int(odd_off.sum()), int(after.sum()), int(keep.sum())


def test_odd_length_mix():
    L = 60_000
    rec = S.odd_length_tile(L, 3000, 21)
    lists = S.site_lists(L, rec, 4)
    lists["half"] = S.half_dropping_list(L, rec, 22)
    tie(L, rec, lists, what="odd lengths")
    n_odd, n_after, n_kept = odd_conditions(L, rec, lists["half"], 0)
    assert n_odd >= 100 and n_after >= 100 and 0.3 * rec.n < n_kept < 0.7 * rec.n, (n_odd, n_after, n_kept, rec.n)
    assert int((np.diff(rec.seq_off.astype(np.int64)) == 0).sum()) >= 100


def test_kept_reads_hold_every_hit():
    """site_ref.kept against the hits: a read that has a hit is kept, and the kept reads alone give the rows of the
    whole tile."""
    L = 5000
    rec = S.adversarial_tile(2, L, 1500, True)
    sites = S.site_lists(L, rec, 2)["sparse"]
    for mq in (0, 10):
        keep = S.kept(L, rec, mq, sites)
        r, _, _ = S.hits(L, L, rec, mq, sites)
        assert keep[np.unique(r)].all() and 0 < int(keep.sum()) < rec.n
        only = S.permuted(rec, np.flatnonzero(keep))
        assert np.array_equal(S.hist_at_sites(L, L, only, mq, sites), S.hist_at_sites(L, L, rec, mq, sites))


def test_hits_add_up_to_the_rows():
    L = 3000
    rec = S.adversarial_tile(1, L, 600, False)
    sites = S.site_lists(L, rec, 1)["duplicates"]
    pos0, order = S.sorted_sites(sites)
    for mq in (0, 10):
        _, lo, _ = S.hits(L, L - 300, rec, mq, sites)
        per_entry = np.zeros(sites.shape[0], np.int64)
        per_entry[order] = np.bincount(lo, minlength=order.shape[0])
        assert np.array_equal(per_entry, S.hist_at_sites(L, L - 300, rec, mq, sites).sum(1))


def test_oracle_rows_do_not_depend_on_the_rest_of_the_list():
    """Every entry gets its row (duplicates included), and a site of 2**31 or 2**32 - 1 costs no memory."""
    L = 5000
    rec = S.adversarial_tile(2, L, 1500, True)
    ref = np.full(L, ord("A"), np.uint8)
    covered = np.flatnonzero(S.hist_all(L, L, rec, 0).sum(1) > 0) + 1
    a = covered[:60].astype(np.uint32)
    sites = np.concatenate([a, np.array([2**31, 2**32 - 1, 0], np.uint32), a[::-1], a[:7]])
    out = oracle.site_pileup(1, 0, L, ref, rec, sites)
    one = oracle.site_pileup(1, 0, L, ref, rec, a)
    assert one["hist"].sum(1).min() > 0
    assert np.array_equal(out["hist"][:60], one["hist"]) and np.array_equal(out["hist"][63:123], one["hist"][::-1])
    assert np.array_equal(out["hist"][123:], one["hist"][:7]) and not out["hist"][60:63].any()
    for k in ("total", "count", "base", "called", "freq"):
        assert np.array_equal(out[k][:60], one[k]) and np.array_equal(out[k][63:123], one[k][::-1]), k
    assert oracle.site_pileup(1, 0, L, ref, rec, np.zeros(0, np.uint32))["hist"].shape == (0, 16)


def test_ballast_share_and_the_whole_tile_at_small_size():
    """The past-2^32 tile of the device test with its mark at 2^20 bases: the reference of the interesting reads plus
    the ballast's share equals the oracle over the whole tile."""
    L = 20_000
    it = S.concat([S.adversarial_tile(2, 5000, 1500, True), synth.short_read_contig(L, 10, 5, with_seq=True)])
    cross = 900
    B = S.ballast_bases(it, cross, 1 << 20)
    buf = S.ballast_buffer(it, B, 1)
    ref = np.full(L, ord("A"), np.uint8)
    sites = S.site_lists(L, it, 3)
    for lens in (S.ballast_lengths(B, 40_000, seed=2), S.ballast_lengths(B, 6000, fixed=True)):
        tile, nb = S.ballast_tile(it, buf, lens, 8000, 4)
        assert int(tile.seq_off[nb + cross]) < (1 << 20) <= int(tile.seq_off[nb + cross + 1]) and int(tile.seq_off[nb]) == B
        mine = tile.slice(nb, tile.n)
        for mq in (0, 10):
            both = S.hist_all(L, L, mine, mq)
            assert np.array_equal(both, S.hist_all(L, L, it, mq))
            for name, s in sites.items():
                want = oracle.site_pileup(1, mq, L, ref, tile, s)["hist"]
                got = S.rows(both, L, L, s)
                if mq <= 5:
                    got = got + S.ballast_share(tile, nb, L, L, s.astype(np.int64) - 1)
                assert np.array_equal(got, want), (name, mq)
            if mq == 0:
                assert int(S.ballast_share(tile, nb, L, L, np.arange(L)).sum()) > 10 * L
