"""The deletion scan on the device (-m gpu): cl_site_scan_dels in both forms and find-deletions; counts, classes and the
full candidate list compared exactly with the independent reference tests/dels_ref.py (a plain Python walk written from the
rule) -- never with the engine's own other calls, except where the invariant between two calls is what is tested."""
import ctypes as C
import random
import subprocess

import numpy as np
import pytest

import dels_ref as D
from bamio import write_bam, write_fasta
from helpers import load_kats
from test_gpu_filtered_scan import requal
from decodingustools_amd import CallableOptions, Engine, EngineError, _lib, build as _b, synth, variants as V
from decodingustools_amd.callable_loci import HostStage
from decodingustools_amd.records import ContigRecords, pack_seq4

pytestmark = pytest.mark.gpu
KATS = load_kats()
W = 1024                                            # the kernel's window
PARAMS = [(1, 1, 1), (2, 1, 2500), (10, 3, 7000)]   # (min_depth, min_del_count, min_del_per_10k)
FILTERS = [(0, False), (0x704, False), (0x704, True), (0xFFFF, True)]
FIELDS = ("pos", "ref", "del", "depth", "del_fwd", "del_rev", "depth_fwd", "depth_rev")


def rows(cand):
    return [(int(r["pos"]), chr(r["ref"])) + tuple(int(r[f]) for f in FIELDS[2:]) for r in cand]


def same_dels(got, exp, what):
    assert (got.low_depth, got.kept, got.deleted) == (exp["low_depth"], exp["kept"], exp["deleted"]), what
    assert got.low_depth + got.kept + got.deleted == got.end - got.start, what
    have = rows(got.candidates)
    if have != exp["candidates"]:
        bad = next((i for i, (x, y) in enumerate(zip(have, exp["candidates"])) if x != y), min(len(have), len(exp["candidates"])))
        assert False, (what, bad, have[bad:bad + 2], exp["candidates"][bad:bad + 2])


def check_dels(eng, L, ref, rec, mq, mbq, filters=FILTERS, params=PARAMS, ranges=None, what=""):
    """The resident tile of `eng` is `rec` (attachment at mbq): both forms, every filter, parameter triple and range.
    Returns the number of candidates seen."""
    ref_len = ref.shape[0]
    seen = 0
    for flt in [None] + list(filters):
        if flt is None:
            depth, dels = D.walk(L, ref_len, rec, mq)
        else:
            depth, dels = D.walk(L, ref_len, rec, mq, flt[0], mbq if flt[1] else None)
        for md, cnt, per in params:
            for a, b in (ranges or [(0, L)]):
                exp = D.reduce(depth, dels, ref, L, md, cnt, per, a, b, stranded=flt is not None)
                got = eng.site_scan_dels(mq, md, cnt, per, ref, a, b, filter=flt)
                assert (got.start, got.end) == (a, b)
                same_dels(got, exp, (what, mq, mbq, flt, (md, cnt, per), (a, b)))
                seen += got.deleted
    return seen


@pytest.mark.parametrize("case", KATS["site_cases"], ids=[c["name"] for c in KATS["site_cases"]])
def test_del_scan_site_kats(case):
    rec = requal(ContigRecords.from_reads([tuple(r) for r in case["reads"]]), 5)
    ref = np.frombuffer(case["ref"].encode(), dtype=np.uint8).copy()
    L = case["contig_len"]
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, ref.shape[0], rec)
        eng.site_attach_quals(rec, 20)
        for mq in (0, case["min_quality"]):
            check_dels(eng, L, ref, rec, mq, 20, ranges=[(0, L), (0, 0), (L // 2, L)], what=case["name"])


def random_reads(L, n, seed, codes="ACGTACGTACGTNRY="):
    """Reads with every CIGAR operation at random places -- a deletion in two of three, some directly behind an insertion,
    a clip or the read's start, some beside an N skip -- some hanging over the contig's end, some with fewer bases than the
    CIGAR consumes or none at all."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ops, q = [], 0
        k = rng.random()
        if k < 0.25:
            l = rng.randint(1, 9); ops.append(f"{l}S"); q += l
        if k < 0.05 or k > 0.97:
            ops.append(f"{rng.randint(1, 9)}D")
        for _ in range(rng.randint(1, 4)):
            l = rng.randint(3, 90); ops.append(f"{l}{rng.choice('MMM=X')}"); q += l
            k = rng.random()
            if k < 0.2:
                l = rng.randint(1, 6); ops.append(f"{l}I"); q += l
                if k < 0.1:
                    ops.append(f"{rng.randint(1, 20)}D")
            elif k < 0.7:
                ops.append(f"{rng.randint(1, 60)}D")
                if k < 0.3:
                    ops.append(f"{rng.randint(5, 200)}N")
            elif k < 0.8:
                ops.append(f"{rng.randint(5, 200)}N")
                if k < 0.75:
                    ops.append(f"{rng.randint(1, 20)}D")
        l = rng.randint(2, 40); ops.append(f"{l}M"); q += l
        if rng.random() < 0.3:
            l = rng.randint(1, 9); ops.append(f"{l}S"); q += l
        k = rng.random()
        q = 0 if k < 0.03 else rng.randint(1, q) if k < 0.1 else q
        seq = "".join(rng.choice(codes) for _ in range(q))
        out.append((rng.randint(0, L - 1), "".join(ops), rng.choice([0, 5, 19, 20, 40, 60]), 30, 0x10 * (i & 1), f"r{i}", seq))
    return out


PLANT_L = 3 * W + 17
S40 = "ACGT" * 10


def planted_reads(L=PLANT_L, short=PLANT_L - 100):
    """(reads, the positions every one of which some planted deletion covers under no filter)."""
    q10 = [30] * 10
    reads = [
        # window borders
        (W - 21, "10M11D10M", 60, 30, 0, "ends-at-1023", S40[:20]),
        (W - 10, "10M8D10M", 60, 30, 0x10, "starts-at-1024", S40[:20]),
        (290, "10M2500D10M", 60, 30, 0, "over-a-whole-window", S40[:20]),
        (291, "9M2501D10M", 60, 30, 0x10, "over-a-whole-window-rev", S40[:19]),
        (L - 20, "10M30D5M", 60, 30, 0, "past-the-contig", S40[:15]),
        (short - 15, "10M20D5M", 60, 30, 0x10, "past-a-shorter-reference", S40[:15]),
        # the rule's corners
        (50, "5D10M", 60, 30, 0, "leading", S40[:10]),
        (60, "5M2I3D5M", 60, 30, 0x10, "behind-i", S40[:12]),
        (80, "4S3D6M", 60, 30, 0, "behind-s", S40[:10]),
        (2 * W - 30, "40M5D10M", 60, 30, 0, "bases-ran-out", "T" * 33),
        (2 * W - 60, "20M5D10M", 60, 30, 0x10, "at-l-seq", "G" * 20),
        (100, "10M5D10M", 60, None, 0, "no-bases", ""),
        (120, "5M3N2D5M", 60, 30, 0, "n-then-d", S40[:10]),
        (140, "5M2D3N5M", 60, 30, 0x10, "d-then-n", S40[:10]),
        (160, "3=2X4D3=", 60, 30, 0, "eq-x", S40[:8]),
        (200, "5M4D5M", 60, [30, 30, 30, 30, 19, 30, 30, 30, 30, 30], 0, "carrier-below", S40[:10]),
        (200, "5M4D5M", 60, [10, 10, 10, 10, 20, 10, 10, 10, 10, 10], 0x10, "carrier-at", S40[:10]),
        (220, "5M4D5M", 60, [10, 10, 10], 0, "carrier-without-a-value", S40[:10]),
        (220, "5M4D5M", 60, [], 0x10, "no-values", S40[:10]),
        (240, "5M4D5M", 60, q10, 0x400, "duplicate", S40[:10]),
        (240, "5M4D5M", 19, q10, 0, "mapq-19", S40[:10]),
        (240, "5M4D5M", 20, q10, 0x10, "mapq-20", S40[:10]),
        (L + 5, "5M4D5M", 60, q10, 0, "starts-beyond-the-contig", S40[:10]),
    ]
    reads += random_reads(L, 300, 3)
    reads.sort(key=lambda r: r[0])
    return reads


def test_del_scan_planted_deletions_at_window_borders_and_the_rules_corners():
    L, short = PLANT_L, PLANT_L - 100
    rec = ContigRecords.from_reads(planted_reads())
    ref = synth.make_reference(L, 5, lowercase=True)
    ranges = [(0, L), (1000, 1030), (W + 5, W + 300), (W - 1, W), (7, 7)]
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        seen = check_dels(eng, L, ref, rec, 20, 20, ranges=ranges, what="planted")
        assert seen > 1000
        check_dels(eng, L, ref, rec, 0, 20, filters=[(0, True)], params=[(1, 1, 1)], what="planted, every mapq")
        # what the planted reads say by themselves, whatever the reference walk does: under (1, 1, 1) every position with a
        # counted deletion is listed with its counts
        reads = [r for r in planted_reads() if not r[5].startswith("r")]
        only = ContigRecords.from_reads(reads)
        eng.site_upload(L, L, only)
        eng.site_attach_quals(only, 20)
        got = {r[0] - 1: r for r in rows(eng.site_scan_dels(20, 1, 1, 1, ref).candidates)}
        for p in range(W - 11, W):
            assert p in got, p                                          # ends at 1023 ...
        assert got[W - 1][2] == 3 and got[W][2] == 3 and got[W + 7][2] == 3 and got[W + 8][2] == 2      # ... starts at 1024, both over the long ones
        assert all(got[p][2:4] == (2, 0) for p in range(W + 18, 2 * W - 60))          # the middle window: deletions only
        assert got[2799][2] == 2 and got[2800][2] == 1 and 2801 not in got
        assert got[L - 1][2:4] == (1, 0) and max(got) == L - 1
        assert not any(p in got for p in range(50, 55))                # leading D
        assert all(got[p][2:4] == (1, 0) for p in (65, 66, 67, 80, 81, 82))            # behind I, behind S
        assert all(got[p][2] == 2 for p in range(2 * W + 10, 2 * W + 15))                # the bases ran out: the two long ones only
        assert all(got[p][2] == 3 for p in range(2 * W - 40, 2 * W - 35))               # y == l_seq (and the two long ones)
        assert not any(p in got for p in range(110, 115))              # l_seq == 0
        assert sorted(p for p in got if 120 <= p < 160) == [128, 129, 145, 146]         # N is no deletion
        assert all(got[p][2:4] == (1, 0) for p in range(165, 169))                     # = X
        assert all(got[p][2] == 2 for p in range(205, 209)) and all(got[p][2] == 2 for p in range(225, 229))
        assert all(got[p][2] == 2 for p in range(245, 249))            # mapq 20 and the duplicate; not mapq 19
        flt = {r[0] - 1: r for r in rows(eng.site_scan_dels(20, 1, 1, 1, ref, filter=(0x400, True)).candidates)}
        assert all(flt[p][2:6] == (1, 0, 0, 1) for p in range(205, 209))               # the carrier at 20 passes, the one at 19 does not
        assert all(flt[p][2:6] == (2, 0, 1, 1) for p in range(225, 229))               # a carrier without a value passes
        assert all(flt[p][2:6] == (1, 0, 0, 1) for p in range(245, 249))
        # ref_len < contig_len: nothing counts at or beyond it
        for r in (rec, only):
            eng.site_upload(L, short, r)
            eng.site_attach_quals(r, 20)
            check_dels(eng, L, ref[:short], r, 20, 20, filters=[(0, False), (0x704, True)], ranges=[(0, L), (short - 5, short + 5), (short, L)],
                       what="short reference")
        got = {r[0] - 1: r for r in rows(eng.site_scan_dels(20, 1, 1, 1, ref[:short]).candidates)}
        assert all(got[p][2:4] == (1, 0) for p in range(short - 5, short)) and max(got) == short - 1
        tail = eng.site_scan_dels(0, 1, 1, 1, ref[:short], short, L)
        assert (tail.low_depth, tail.kept, tail.deleted) == (L - short, 0, 0)


def test_del_scan_of_random_reads_and_of_an_unsorted_copy():
    L = PLANT_L
    reads = sorted(random_reads(L, 500, 11), key=lambda r: r[0])
    shuffled = list(reads)
    random.Random(4).shuffle(shuffled)
    ref = synth.make_reference(L, 5)
    ranges = [(0, L), (W - 3, W + 3), (2 * W + 1, 3 * W - 1), (L - 1, L), (L, L)]
    results = []
    for k, order in enumerate((reads, shuffled)):
        rec = requal(ContigRecords.from_reads(order), 17, ragged=True)
        with Engine(CallableOptions(), 0) as eng:
            eng.site_upload(L, L, rec)
            eng.site_attach_quals(rec, 20)
            if k == 0:
                assert check_dels(eng, L, ref, rec, 10, 20, ranges=ranges, what="random") > 1000
        # the same qualities and flags on both orders: attached by name
        plain = ContigRecords.from_reads([r[:3] + ([20 + (int(r[5][1:]) * 7) % 25] * max(0, len(r[6]) - int(r[5][1:]) % 4),
                                                   [0, 0x10, 0x400, 0x10][int(r[5][1:]) % 4]) + r[5:] for r in order])
        with Engine(CallableOptions(), 0) as eng:
            eng.site_upload(L, L, plain)
            eng.site_attach_quals(plain, 30)
            check_dels(eng, L, ref, plain, 10, 30, filters=[(0x704, True)], params=[(2, 1, 2500)], ranges=[(0, L), (W - 3, W + 3)], what=f"order {k}")
            results.append([eng.site_scan_dels(10, 1, 1, 1, ref, filter=f) for f in (None, (0x704, True))])
    for a, b in zip(*results):
        assert (a.low_depth, a.kept, a.deleted) == (b.low_depth, b.kept, b.deleted) and np.array_equal(a.candidates, b.candidates) and a.deleted > 500


def column(p, n_del, n_base, name):
    """n_del reads that delete p and n_base reads with a base there; strands alternate."""
    return [(p - 1, "1M1D1M" if i < n_del else "3M", 60, 30, 0x10 * (i & 1), f"{name}{i}", "AC" if i < n_del else "ACG") for i in range(n_del + n_base)]


def test_del_scan_threshold_edges():
    L = 2 * W + 100
    ref = synth.make_reference(L, 9)
    cols = {10: (7, 3),            # 7 / 10: exactly 0.7
            20: (6, 4),            # one read below it
            30: (3, 0),            # exactly min_del_count 3
            40: (2, 1),            # one below
            W - 1: (7, 3), W + 2: (6, 3),                              # span 10 == min_depth, span 9: low_depth
            W + 50: (1, 9)}                                  # 1 of 10 at 1000 per 10 000
    reads = sorted((r for p, (d, b) in cols.items() for r in column(p, d, b, f"c{p}_")), key=lambda r: r[0])
    rec = ContigRecords.from_reads(reads)
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        check_dels(eng, L, ref, rec, 20, 20, filters=[(0, False), (0x10, False)], params=[(1, 1, 1), (1, 1, 7000), (1, 3, 1), (10, 1, 1), (10, 3, 7000), (1, 1, 1000), (1, 1, 1001)],
                   ranges=[(0, L), (W - 1, W + 3)], what="edges")
        for flt in (None, (0, False)):
            def at(*prm):
                return {r[0] - 1 for r in rows(eng.site_scan_dels(20, *prm, ref, filter=flt).candidates)}
            assert at(1, 1, 1) == set(cols)
            assert at(1, 1, 7000) == {10, 30, W - 1}                    # 7 / 10 and 3 / 3; 6 / 10, 2 / 3 and 6 / 9 are below
            assert at(1, 3, 1) == {10, 20, 30, W - 1, W + 2}
            assert at(10, 1, 1) == {10, 20, W - 1, W + 50}
            got = eng.site_scan_dels(20, 10, 1, 1, ref, W + 2, W + 3, filter=flt)
            assert (got.low_depth, got.kept, got.deleted) == (1, 0, 0)
            assert W + 50 in at(1, 1, 1000) and W + 50 not in at(1, 1, 1001)
            assert D.classify(7, 3, 1, 1, 7000) == D.DELETED and D.classify(6, 4, 1, 1, 7000) == D.KEPT


def test_del_scan_one_deep_column_needs_64_bits():
    """2^20 reads over one position, 45 % of them with a deletion there: 10000 * del is past 2^32.  The column is reported
    with exact counts; the same column with one deleting read fewer is not."""
    n = 1 << 20
    d = -(-4500 * n // 10000)                                            # the smallest count with 10000 d >= 4500 n: 471 860
    assert 10000 * d >= 4500 * n > 10000 * (d - 1) and 10000 * d > 1 << 32
    L = 2 * W
    is_del = np.zeros(2 * n, bool)
    is_del[:d] = True                                                    # d at 1000 ...
    is_del[n:n + d - 1] = True                                           # ... d - 1 at 1500
    pos = np.concatenate([np.full(n, 999, np.int32), np.full(n, 1499, np.int32)])
    n_ops = np.where(is_del, 3, 1)
    cigar_off = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.uint32)
    cigar = np.full(int(cigar_off[-1]), (1 << 4) | 0, np.uint32)         # 1M ...
    first = cigar_off[:-1].astype(np.int64)
    cigar[first[~is_del]] = (3 << 4) | 0                                 # 3M
    cigar[first[is_del] + 1] = (1 << 4) | 2                              # 1M 1D 1M
    n_bases = np.where(is_del, 2, 3)
    base_off = np.concatenate([[0], np.cumsum(n_bases)]).astype(np.uint64)
    flag = ((np.arange(2 * n) % 3 == 0).astype(np.uint16) << np.uint16(4))
    rec = ContigRecords(pos=pos, flag=flag, mapq=np.full(2 * n, 60, np.uint8), cigar_off=cigar_off, cigar=cigar, qual_off=base_off,
                        qual=np.full(int(base_off[-1]), 30, np.uint8), qname_off=np.arange(2 * n + 1, dtype=np.uint32),
                        qname=np.full(2 * n, ord("p"), np.uint8)).validate()
    rec.seq_off = base_off.copy()
    rec.seq4 = pack_seq4(np.full(int(base_off[-1]), 2, np.uint8))
    ref = synth.make_reference(L, 4)
    rev = flag[:n] != 0
    d_rev, b_rev = int(rev[:d].sum()), int(rev[d:].sum())
    assert D.classify(d, n - d, 10, 3, 4500) == D.DELETED and D.classify(d - 1, n - d + 1, 10, 3, 4500) == D.KEPT
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        for flt, strands in ((None, (0, 0, 0, 0)), ((0, False), (d - d_rev, d_rev, n - d - b_rev, b_rev)), ((0, True), (d - d_rev, d_rev, n - d - b_rev, b_rev))):
            got = eng.site_scan_dels(20, 10, 3, 4500, ref, filter=flt)
            assert (got.low_depth, got.kept, got.deleted) == (L - 6, 5, 1), flt
            assert rows(got.candidates) == [(1001, chr(ref[1000] & 0xDF), d, n - d) + strands], flt
            both = rows(eng.site_scan_dels(20, 10, 3, 4499, ref, 900, 1600, filter=flt).candidates)
            assert [r[:4] for r in both] == [(1001, chr(ref[1000] & 0xDF), d, n - d), (1501, chr(ref[1500] & 0xDF), d - 1, n - d + 1)], flt


def test_del_scan_grows_its_candidate_buffer():
    """70 000 deleted positions: more candidates than the buffer's first 65 536 entries (the smallest range that has more
    is one of 65 537 positions; the scan has no hook that shrinks the buffer)."""
    n_del = 70_000
    L = n_del + 2
    reads = [(0, f"1M{n_del}D1M", 60, 30, 0x10 * (i & 1), f"w{i}", "AC") for i in range(4)] + [(5, "20M", 60, 30, 0, "m", "A" * 20)]
    rec = ContigRecords.from_reads(reads)
    ref = synth.make_reference(L, 6)
    depth, dels = D.walk(L, L, rec, 20)
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        for flt in (None, (0, False)):
            exp = D.reduce(depth, dels, ref, L, 1, 1, 1, 0, L, stranded=flt is not None)
            assert exp["deleted"] == n_del
            got = eng.site_scan_dels(20, 1, 1, 1, ref, filter=flt)
            same_dels(got, exp, flt)
            assert np.array_equal(got.candidates["pos"], np.arange(2, L))
            again = eng.site_scan_dels(20, 1, 1, 1, ref, filter=flt)
            assert np.array_equal(again.candidates, got.candidates) and got.kernel_ms > 0
            # one position more than the first buffer holds, then a smaller range: the grown buffer serves it
            same_dels(eng.site_scan_dels(20, 1, 1, 1, ref, 1, 65_538, filter=flt), D.reduce(depth, dels, ref, L, 1, 1, 1, 1, 65_538, stranded=flt is not None), (flt, "65537"))
            same_dels(eng.site_scan_dels(20, 1, 1, 1, ref, 100, 1100, filter=flt), D.reduce(depth, dels, ref, L, 1, 1, 1, 100, 1100, stranded=flt is not None), (flt, "range"))
        assert V.del_events(got.candidates) == [{"start": 2, "end": L - 1, "length": n_del, "q": 2, "del": 4, "span": 4, "del_fwd": 2, "del_rev": 2, "max_del": 4}]


QUALS = [10, 19, 20, 30, 40]
LOCI = [(3000, 9, 60, "both"), (5000, 2, 25, "both"), (8281, 9, 60, "fwd"), (12000, 70, 60, "both")]   # (first deleted position, length, carriers of 60, strands)


def del_sample(L, seed, n=3000, rl=100):
    """Reads of rl bases over a reference, a small deletion in one of ten, an insertion or a clip in a few; at LOCI sixty
    reads each, `carriers` of them with the deletion.  Qualities around 20, strands alternate, a few flagged reads."""
    ref = synth.make_reference(L, seed)
    text = bytes(ref & 0xDF).decode()
    rng = random.Random(seed + 1)
    reads = []

    def add(p, cigar, name, strand):
        k = rng.random()
        flag = (0x10 if strand else 0) | (0x400 if k < 0.03 else 0x100 if k < 0.05 else 0)
        reads.append((p, cigar, rng.choice([60, 60, 60, 30, 5]), rng.choices(QUALS, k=rl), flag, name, text[p:p + rl]))

    for i in range(n):
        p = rng.randint(0, L - rl - 80)
        k = rng.random()
        a = rng.randint(5, rl - 10)
        if k < 0.85:
            cigar = f"{rl}M"
        elif k < 0.95:
            cigar = f"{a}M{rng.randint(1, 12)}D{rl - a}M"
        elif k < 0.98:
            cigar = f"{a}M2I{rl - a - 2}M"
        else:
            cigar = f"{a}S{rl - a}M"
        add(p, cigar, f"s{i}", i & 1)
    for locus, length, carriers, strands in LOCI:
        for i in range(60):
            add(locus - 50, f"50M{length}D50M" if i < carriers else f"{rl}M", f"l{locus}_{i}", 0 if strands == "fwd" and i < carriers else i & 1)
    reads.sort(key=lambda r: r[0])
    return ref, ContigRecords.from_reads(reads)


def test_del_scan_invariants_and_interleaving():
    L = 20_000
    ref, rec = del_sample(L, 40)
    sites = np.sort(np.random.default_rng(8).choice(np.arange(1, L + 1), 2000, replace=False)).astype(np.uint32)
    with Engine(CallableOptions(), 0) as eng:
        lib, h = eng._lib, eng._h
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        refp = ref.ctypes.data
        # the other calls before: their results, and the context-owned candidate arrays of the other scans by their addresses
        run0 = eng.site_run(20, sites)
        scan0, ex0 = eng.site_scan(20, 10, ref), eng.site_scan_ex(20, 10, ref, 0x704, True)
        minor0 = eng.site_scan_minor(20, 10, 3, 500, ref, filter=(0x704, True))
        c5, c9 = eng.site_scan_counts(20, 0, L), eng.site_scan_counts_ex(20, 0, L, 0x704, True)
        r1, r2, r3 = _lib.cl_scan_result(), _lib.cl_scan_result_ex(), _lib.cl_minor_result()
        f704 = _lib.cl_scan_filter(0x704, 1, 0)
        prm = _lib.cl_minor_params(10, 3, 500)
        assert lib.cl_site_scan(h, 20, 10, refp, L, 0, L, C.byref(r1)) == 0
        assert lib.cl_site_scan_ex(h, 20, 10, C.byref(f704), refp, L, 0, L, C.byref(r2)) == 0
        assert lib.cl_site_scan_minor(h, 20, C.byref(f704), C.byref(prm), refp, L, 0, L, C.byref(r3)) == 0
        keep = [C.string_at(r1.candidates, int(r1.n_variant) * 28), C.string_at(r2.candidates, int(r2.n_variant) * 44),
                C.string_at(r3.candidates, int(r3.n_minor) * 44)]
        plain = eng.site_scan_dels(20, 10, 3, 7000, ref)
        off = eng.site_scan_dels(20, 10, 3, 7000, ref, filter=(0, False))
        on = eng.site_scan_dels(20, 10, 3, 7000, ref, filter=(0x704, True))
        every = eng.site_scan_dels(20, 1, 1, 1, ref, filter=(0x704, True))
        every_plain = eng.site_scan_dels(20, 1, 1, 1, ref)
        # the three planted events are 88 positions; one read in ten has a small deletion, of which the mapping quality, the
        # flags and the carrier's quality (two of five values are below 20) leave about 2100 * 0.8 * 0.95 * 0.6 position-reads
        assert plain.deleted >= 80 and every.deleted > 500 and every_plain.deleted > every.deleted
        same_dels(every, D.reduce(*D.walk(L, L, rec, 20, 0x704, 20), ref, L, 1, 1, 1, 0, L), "every")
        assert keep == [C.string_at(r1.candidates, int(r1.n_variant) * 28), C.string_at(r2.candidates, int(r2.n_variant) * 44),
                        C.string_at(r3.candidates, int(r3.n_minor) * 44)]
        # the planted events, by the default rule: the heteroplasmic one at 5000 is not among them
        assert [(e["start"], e["length"]) for e in V.del_events(plain.candidates)] == [(3001, 9), (8282, 9), (12001, 70)]
        # filter {0, 0} and no filter agree in everything but the four strand fields
        assert (plain.low_depth, plain.kept, plain.deleted) == (off.low_depth, off.kept, off.deleted)
        for f in FIELDS[:4]:
            assert np.array_equal(plain.candidates[f], off.candidates[f]), f
        for f in FIELDS[4:]:
            assert not plain.candidates[f].any()
        # the strand counts add up; a candidate's depth is the dense scan's depth there
        for res in (off, on, every):
            c = res.candidates
            assert np.array_equal(c["del_fwd"].astype(np.int64) + c["del_rev"], c["del"]) and np.array_equal(c["depth_fwd"].astype(np.int64) + c["depth_rev"], c["depth"])
            assert res.low_depth + res.kept + res.deleted == L and (np.diff(c["pos"].astype(np.int64)) > 0).all()
        assert np.array_equal(every.candidates["depth"], c9[every.candidates["pos"].astype(np.int64) - 1, 8])
        assert np.array_equal(on.candidates["depth"], c9[on.candidates["pos"].astype(np.int64) - 1, 8])
        assert np.array_equal(every_plain.candidates["depth"], c5[every_plain.candidates["pos"].astype(np.int64) - 1, 4])
        # ... and each equals the reference
        same_dels(on, D.reduce(*D.walk(L, L, rec, 20, 0x704, 20), ref, L, 10, 3, 7000, 0, L), "on")
        same_dels(plain, D.reduce(*D.walk(L, L, rec, 20), ref, L, 10, 3, 7000, 0, L, stranded=False), "plain")
        ms, nbytes = eng.site_scan_stats()
        assert ms > 0 and nbytes > 20 * rec.n + 32 * every_plain.deleted
        # the other calls after: the same results, and the deletion scan's own candidate array stays as it is across them
        r4, dprm = _lib.cl_del_result(), _lib.cl_del_params(10, 3, 7000)
        assert lib.cl_site_scan_dels(h, 20, C.byref(f704), C.byref(dprm), refp, L, 0, L, C.byref(r4)) == 0
        keep_del = C.string_at(r4.candidates, int(r4.n_deleted) * 32)
        assert int(r4.n_deleted) == on.deleted and keep_del == on.candidates.tobytes()
        assert np.array_equal(eng.site_run(20, sites), run0)
        scan1, ex1 = eng.site_scan(20, 10, ref), eng.site_scan_ex(20, 10, ref, 0x704, True)
        for x, y in ((scan0, scan1), (ex0, ex1)):
            assert (x.low_depth, x.mixed, x.uncomparable, x.match, x.variant) == (y.low_depth, y.mixed, y.uncomparable, y.match, y.variant)
            assert np.array_equal(x.candidates, y.candidates)
        minor1 = eng.site_scan_minor(20, 10, 3, 500, ref, filter=(0x704, True))
        assert (minor0.low_depth, minor0.single, minor0.minor) == (minor1.low_depth, minor1.single, minor1.minor) and np.array_equal(minor0.candidates, minor1.candidates)
        assert keep_del == C.string_at(r4.candidates, int(r4.n_deleted) * 32)
        assert np.array_equal(eng.site_scan_counts_ex(20, 0, L, 0x704, True), c9) and np.array_equal(eng.site_scan_counts(20, 0, L), c5)
        again = eng.site_scan_dels(20, 10, 3, 7000, ref, filter=(0x704, True))
        assert np.array_equal(again.candidates, on.candidates)


def test_del_scan_refusals_leave_the_context_usable():
    L = 20_000
    ref, rec = del_sample(L, 50, n=1500)
    sites = np.arange(1, 2000, 7, dtype=np.uint32)

    def refused(*a, **k):
        with pytest.raises(EngineError) as e:
            eng.site_scan_dels(*a, **k)
        assert e.value.status == -1 and len(str(e.value)) > len(" (cl_status -1)") + 10, str(e.value)
        return str(e.value)

    with Engine(CallableOptions(), 0) as eng:
        refused(20, 10, 3, 7000, ref)                                               # nothing resident
        eng.site_pileup(20, L, L, rec, sites)                                      # a tile filtered for its own list
        refused(20, 10, 3, 7000, ref)
        eng.site_upload(L, L, rec)
        assert "attach" in refused(20, 10, 3, 7000, ref, filter=(0, False))         # nothing attached
        ok = eng.site_scan_dels(20, 10, 3, 7000, ref)                              # the unfiltered form needs no attachment
        eng.site_attach_quals(rec, 20)
        for flt in (None, (0x704, True)):
            assert "min_depth" in refused(20, 0, 3, 7000, ref, filter=flt)
            assert "min_del_count" in refused(20, 10, 0, 7000, ref, filter=flt)
            assert "min_del_per_10k" in refused(20, 10, 3, 0, ref, filter=flt)
            assert "min_del_per_10k" in refused(20, 10, 3, 10001, ref, filter=flt)
            refused(20, 10, 3, 7000, ref, 0, L + 1, filter=flt)                     # end > contig_len
            refused(20, 10, 3, 7000, ref, 10, 9, filter=flt)                        # start > end
            refused(20, 10, 3, 7000, ref[:L - 1], 0, L, filter=flt)                 # another ref_len
        out = _lib.cl_del_result()
        st = eng._lib.cl_site_scan_dels(eng._h, 20, None, None, ref.ctypes.data, L, 0, L, C.byref(out))       # null params
        assert st == -1 and b"params" in eng._lib.cl_last_error(eng._h)
        prm = _lib.cl_del_params(10, 3, 7000)
        assert eng._lib.cl_site_scan_dels(eng._h, 20, None, C.byref(prm), ref.ctypes.data, L, 0, L, None) == -1    # null result
        assert eng._lib.cl_site_scan_dels(eng._h, 20, None, C.byref(prm), None, L, 0, L, C.byref(out)) == -1       # null reference
        # the next valid calls succeed and equal the reference
        got = eng.site_scan_dels(20, 10, 3, 7000, ref)
        assert np.array_equal(got.candidates, ok.candidates) and got.deleted > 0
        same_dels(eng.site_scan_dels(20, 10, 3, 10000, ref, filter=(0x704, True)),
                  D.reduce(*D.walk(L, L, rec, 20, 0x704, 20), ref, L, 10, 3, 10000, 0, L), "after the refusals")
        empty = eng.site_scan_dels(20, 10, 3, 7000, ref, 5, 5, filter=(0x704, True))
        assert (empty.low_depth, empty.kept, empty.deleted, empty.candidates.shape[0]) == (0, 0, 0, 0)
    with HostStage(CallableOptions()) as hs:
        with pytest.raises(EngineError) as e:
            hs.site_scan_dels(20, 10, 3, 7000, ref)
        assert e.value.status == -2


def test_find_deletions_on_files_and_cli(tmp_path):
    L = 20_000
    ref, rec = del_sample(L, 60)
    names = ["chr1", "chrM", "chrY"]; lens = [248956422, L, 57227415]
    bam = str(tmp_path / "d.bam"); fa = str(tmp_path / "d.fa")
    write_bam(bam, list(zip(names, lens)), {1: rec}, block_every=5000)
    write_fasta(fa, [("chrM", ref)])

    def want(mq=20, md=10, per=7000, cnt=3, mbq=None, ex=0, k=0, a=0, b=L):
        exp = D.reduce(*D.walk(L, L, rec, mq, ex, mbq), ref, L, md, cnt, per, a, b)
        return D.expected_tsv("chrM", exp, a, b, md, mq, mbq, ex, per, cnt, k), exp

    out = str(tmp_path / "o.tsv")
    w0, e0 = want()
    assert [(e["start"], e["length"]) for e in D.events(e0["candidates"])] == [(3001, 9), (8282, 9), (12001, 70)] and "\t.\t" in w0
    V.find_deletions(bam, fa, "chrM", out)
    assert open(out).read() == w0
    w1, e1 = want(mbq=20, ex=0x704, k=2, per=2500, cnt=2)
    assert e1["deleted"] > e0["deleted"] and "\tstrand\n" in w1 and "\tPASS\n" in w1
    V.find_deletions(bam, fa, "chrM", out, min_del_fraction="0.25", min_del_count=2, min_base_quality=20, exclude_flags=0x704, min_del_per_strand=2)
    assert open(out).read() == w1

    def cli(*args):
        return subprocess.run([_b.CLI, "find-deletions", bam, "-r", fa, "-o", out, "-L", "chrM"] + list(args), capture_output=True, text=True)

    r = cli()
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w0
    r = cli("--min-del-fraction", "0.25", "--min-del-count=2", "--min-base-quality", "20", "--exclude-flags", "0x704", "--min-del-per-strand=2")
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w1
    a, b = 3_000 + 4, 12_030                                            # cuts the first and the last event
    r = cli(f"--region={a}-{b}", "--min-depth", "12", "--min-quality=30", "--exclude-flags", "1796", "--min-del-fraction=.0125", "--min-del-count", "1")
    assert r.returncode == 0, r.stderr
    w2, e2 = want(mq=30, md=12, per=125, cnt=1, ex=0x704, a=a, b=b)
    assert open(out).read() == w2 and D.events(e2["candidates"])[0]["start"] == a + 1 and D.events(e2["candidates"])[-1]["end"] == b
    V.find_deletions(bam, fa, "chrM", out, region=(a, b), min_depth=12, min_quality=30, exclude_flags=0x704, min_del_fraction=".0125", min_del_count=1)
    assert open(out).read() == w2
    # an unknown contig and a region beyond the contig: exit 1 with a message
    r = subprocess.run([_b.CLI, "find-deletions", bam, "-r", fa, "-o", out, "-L", "chrZ"], capture_output=True, text=True)
    assert r.returncode == 1 and "chrZ" in r.stderr
    r = cli(f"--region=0-{L + 1}")
    assert r.returncode == 1 and "beyond" in r.stderr
    with pytest.raises(EngineError):
        V.find_deletions(bam, fa, "chrZ", out)
