"""The insertion scan on the device (-m gpu): cl_site_scan_ins in both forms and find-insertions; counts, classes, the full
candidate list and the full observation list compared exactly with the independent reference tests/ins_ref.py (a plain
Python walk written from the rule) -- never with the engine's own other calls, except where the invariant between two calls
is what is tested."""
import ctypes as C
import random
import subprocess

import numpy as np
import pytest

import ins_ref as I
from bamio import write_bam, write_fasta
from test_gpu_filtered_scan import requal
from decodingustools_amd import CallableOptions, Engine, EngineError, _lib, build as _b, synth, variants as V
from decodingustools_amd.callable_loci import HostStage
from decodingustools_amd.records import ContigRecords, pack_seq4

pytestmark = pytest.mark.gpu
W = 1024                                            # the kernel's window
PARAMS = [(1, 1, 1), (2, 1, 2500), (10, 3, 7000)]   # (min_depth, min_ins_count, min_ins_per_10k)
FILTERS = [(0, False), (0x704, False), (0x704, True), (0xFFFF, True)]
FIELDS = ("pos", "ref", "ins", "depth", "ins_fwd", "ins_rev", "depth_fwd", "depth_rev")


def rows(cand):
    return [(int(r["pos"]), chr(r["ref"])) + tuple(int(r[f]) for f in FIELDS[2:]) for r in cand]


def obs_rows(obs):
    return [(int(o["pos"]), int(o["len"]), int(o["key"][0]), int(o["key"][1]), int(o["strand"])) for o in obs]


def first_difference(have, want):
    bad = next((i for i, (x, y) in enumerate(zip(have, want)) if x != y), min(len(have), len(want)))
    return bad, have[bad:bad + 2], want[bad:bad + 2]


def same_ins(got, exp, obs, what):
    assert (got.low_depth, got.kept, got.inserted) == (exp["low_depth"], exp["kept"], exp["inserted"]), what
    assert got.low_depth + got.kept + got.inserted == got.end - got.start, what
    have = rows(got.candidates)
    assert have == exp["candidates"], (what,) + first_difference(have, exp["candidates"])
    assert got.observations.shape[0] == sum(c[2] for c in exp["candidates"]), what
    have = obs_rows(got.observations)
    assert have == obs, (what,) + first_difference(have, obs)


def check_ins(eng, L, ref, rec, mq, mbq, filters=FILTERS, params=PARAMS, ranges=None, what="", plain=True):
    """The resident tile of `eng` is `rec` (attachment at mbq): both forms, every filter, parameter triple and range.
    Returns the number of observations seen."""
    ref_len = ref.shape[0]
    seen = 0
    for flt in ([None] if plain else []) + list(filters):
        if flt is None:
            depth, ins, events = I.walk(L, ref_len, rec, mq)
        else:
            depth, ins, events = I.walk(L, ref_len, rec, mq, flt[0], mbq if flt[1] else None)
        for md, cnt, per in params:
            for a, b in (ranges or [(0, L)]):
                exp = I.reduce(depth, ins, ref, L, md, cnt, per, a, b, stranded=flt is not None)
                obs = I.observations(events, rec, exp["candidates"], stranded=flt is not None)
                got = eng.site_scan_ins(mq, md, cnt, per, ref, a, b, filter=flt)
                assert (got.start, got.end) == (a, b)
                same_ins(got, exp, obs, (what, mq, mbq, flt, (md, cnt, per), (a, b)))
                seen += len(obs)
    return seen


def random_reads(L, n, seed, codes="ACGTACGTACGTNRY="):
    """Reads with every CIGAR operation at random places -- an insertion in two of three, some directly behind a deletion, a
    skip, a pad, a clip, another insertion or the read's start, some as the last operation -- some hanging over the contig's
    end, some with fewer bases than the CIGAR consumes or none at all."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ops, q = [], 0
        k = rng.random()
        if k < 0.1:
            ops.append(f"{rng.randint(1, 9)}H")
        if k < 0.25:
            l = rng.randint(1, 9); ops.append(f"{l}S"); q += l
        if k < 0.05 or k > 0.95:
            l = rng.randint(1, 9); ops.append(f"{l}I"); q += l
        for _ in range(rng.randint(1, 4)):
            l = rng.randint(1, 90); ops.append(f"{l}{rng.choice('MMM=X')}"); q += l
            k = rng.random()
            if k < 0.6:
                l = rng.choice([1, 1, 1, 2, 3, 5, 16, 17, 32, 33, 40]); ops.append(f"{l}I"); q += l
                if k < 0.1:
                    ops.append(f"{rng.randint(1, 20)}D")
                elif k < 0.2:
                    l = rng.randint(1, 4); ops.append(f"{l}I"); q += l
            elif k < 0.7:
                ops.append(f"{rng.randint(1, 60)}{rng.choice('DNP')}")
                l = rng.randint(1, 4); ops.append(f"{l}I"); q += l
            elif k < 0.8:
                ops.append(f"{rng.randint(5, 200)}N")
        k = rng.random()
        if k < 0.8:
            l = rng.randint(1, 40); ops.append(f"{l}M"); q += l
        if k < 0.3:
            l = rng.randint(1, 9); ops.append(f"{l}S"); q += l
        k = rng.random()
        q = 0 if k < 0.03 else rng.randint(1, q) if k < 0.15 else q
        seq = "".join(rng.choice(codes) for _ in range(q))
        out.append((rng.randint(0, L - 1), "".join(ops), rng.choice([0, 5, 19, 20, 40, 60]), 30, 0x10 * (i & 1), f"r{i}", seq))
    return out


PLANT_L = 3 * W + 17
SHORT = PLANT_L - 100
P32 = "ACGTTGCAAGCTTCGAGGATCCATATGCGCTA"            # 32 bases


def rd(pos, cigar, name, ins="", flag=0, mapq=60, qual=30, n_bases=None):
    """A read whose matched bases are A and whose inserted bases are `ins` (in the order of its I operations), cut to n_bases."""
    seq, at = "", 0
    for l, op in ((int(x[:-1]), x[-1]) for x in __import__("re").findall(r"\d+[MIDNSHP=X]", cigar)):
        if op == "I":
            seq += ins[at:at + l]; at += l
        elif op in "MS=X":
            seq += "A" * l
    assert at == len(ins), (cigar, ins)
    return (pos, cigar, mapq, qual, flag, name, seq if n_bases is None else seq[:n_bases])


def planted_reads(L=PLANT_L, short=SHORT):
    q11 = [30] * 11
    reads = [
        # window borders and the ends of the contig and of a shorter reference
        rd(W - 10, "10M2I10M", "m-ends-at-the-windows-hi", "CG"),                       # anchor W - 1
        rd(W - 9, "10M3I10M", "anchor-at-w", "TGA", flag=0x10),                         # anchor W
        rd(L - 10, "10M2I", "anchor-at-l-1", "GT"),
        rd(short - 10, "10M1I5M", "anchor-at-short-1", "C", flag=0x10),
        rd(short - 9, "10M1I5M", "anchor-at-short", "G"),
        # where the I stands
        rd(50, "2I10M", "first-op", "CC"),
        rd(70, "3S2I10M", "behind-s", "CC", flag=0x10),
        rd(90, "5M2D1I5M", "behind-d", "C"),
        rd(110, "5M1I2D5M", "i-then-d", "C", flag=0x10),                                # counts at 114
        rd(130, "5M3N1I5M", "behind-n", "C"),
        rd(150, "5M1P1I5M", "behind-p", "C", flag=0x10),
        rd(170, "5M1I2I5M", "behind-i", "CGG"),                                        # the first counts at 174
        rd(190, "5M2I", "last-op", "CT", flag=0x10),                                    # counts at 194
        # bases that are not there
        rd(210, "5M3I5M", "inserted-bases-just-there", "CGT", n_bases=8),               # y + len == l_seq: counts at 214
        rd(210, "5M3I5M", "one-inserted-base-short", "CGT", flag=0x10, n_bases=7),
        rd(230, "5M1I5M", "anchor-base-missing", "C", n_bases=4),
        rd(250, "5M1I5M", "no-bases", "C", qual=None, n_bases=0),
        # the anchor's quality and the read gates
        rd(270, "5M1I5M", "anchor-below", "C", qual=[30, 30, 30, 30, 19, 5, 30, 30, 30, 30, 30]),
        rd(270, "5M1I5M", "anchor-at", "C", flag=0x10, qual=[10, 10, 10, 10, 20, 5, 10, 10, 10, 10, 10]),
        rd(290, "5M1I5M", "anchor-without-a-value", "C", qual=[10, 10, 10]),
        rd(290, "5M1I5M", "no-values", "C", flag=0x10, qual=[]),
        rd(310, "5M1I5M", "duplicate", "C", flag=0x400, qual=q11),
        rd(310, "5M1I5M", "mapq-19", "C", mapq=19, qual=q11),
        rd(310, "5M1I5M", "mapq-20", "C", flag=0x10, mapq=20, qual=q11),
        rd(L + 5, "5M1I5M", "starts-beyond-the-contig", "C", qual=q11),
        # lengths and keys: 1, 16, 17, 32, 33 and 100 bases behind position 404
        rd(400, "5M1I5M", "len-1", "G"),
        rd(400, "5M16I5M", "len-16", P32[:16], flag=0x10),
        rd(400, "5M17I5M", "len-17", P32[:17]),
        rd(400, "5M32I5M", "len-32", P32, flag=0x10),
        rd(400, "5M33I5M", "len-33", P32 + "T"),
        rd(400, "5M100I5M", "len-100", P32 + "C" * 68, flag=0x10),
        # an equal prefix of 32 bases: two lengths are two alleles, two tails of one length are one
        rd(500, "5M33I5M", "prefix-33-a", P32 + "A"),
        rd(500, "5M33I5M", "prefix-33-c", P32 + "C", flag=0x10),
        rd(500, "5M100I5M", "prefix-100", P32 + "G" * 68),
        # the first inserted base at an odd and at an even index of the read
        rd(600, "5M2I5M", "first-at-5", "CT"),
        rd(620, "4M2I6M", "first-at-4", "TC", flag=0x10),
        rd(640, "5M4I5M", "other-codes", "NR=Y"),
        rd(660, "5M2I5M", "both-strands-fwd", "GG"),
        rd(660, "5M2I5M", "both-strands-rev", "GG", flag=0x10),
        rd(680, "5M2I5M", "two-alleles-ac", "AC"),
        rd(680, "5M2I5M", "two-alleles-ca", "CA", flag=0x10),
        rd(680, "5M2I5M", "two-alleles-ac-again", "AC", flag=0x10),
    ]
    return reads


def planted_and_random():
    return sorted(planted_reads() + random_reads(PLANT_L, 300, 3), key=lambda r: r[0])


def test_ins_scan_planted_insertions_at_window_borders_and_the_rules_corners():
    L, short = PLANT_L, SHORT
    rec = ContigRecords.from_reads(planted_and_random())
    ref = synth.make_reference(L, 5, lowercase=True)
    ranges = [(0, L), (1000, 1030), (W - 1, W), (W, W + 1), (7, 7), (W - 5, W - 1), (2 * W - 3, L)]
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        assert check_ins(eng, L, ref, rec, 20, 20, ranges=ranges, what="planted") > 1000
        check_ins(eng, L, ref, rec, 0, 20, filters=[(0, True)], params=[(1, 1, 1)], what="planted, every mapq", plain=False)
        # what the planted reads say by themselves, whatever the reference walk does: under (1, 1, 1) every position with a
        # counted insertion is listed with its counts
        only = ContigRecords.from_reads(sorted(planted_reads(), key=lambda r: r[0]))
        eng.site_upload(L, L, only)
        eng.site_attach_quals(only, 20)
        assert {e[2] & 1 for e in I.walk(L, L, only, 20)[2]} == {0, 1}      # first inserted bases at even and at odd seq4 indices
        res = eng.site_scan_ins(20, 1, 1, 1, ref)
        got = {r[0] - 1: r for r in rows(res.candidates)}
        al = {}
        for a in V.ins_alleles(res.observations):
            al.setdefault(a["pos"] - 1, []).append((a["len"], a["seq"], a["count"]))
        assert got[W - 1][2:4] == (1, 2) and got[W][2:4] == (1, 2) and got[L - 1][2:4] == (1, 1) and max(got) == L - 1
        assert al[W - 1] == [(2, "CG", 1)] and al[W] == [(3, "TGA", 1)] and al[L - 1] == [(2, "GT", 1)]
        assert got[short - 1][2] == 1 and got[short][2] == 1
        assert not any(p in got for p in (49, 69, 96, 137, 154))           # first operation; behind S, D, N, P
        assert got[114][2] == 1 and got[174][2] == 1 and al[174] == [(1, "C", 1)] and got[194][2] == 1 and al[194] == [(2, "CT", 1)]
        assert got[214][2:4] == (1, 2) and al[214] == [(3, "CGT", 1)]       # y + len == l_seq counts, one base fewer does not
        assert 234 not in got and 254 not in got                           # no anchor base; no bases at all
        assert got[274][2] == 2 and got[294][2] == 2 and got[314][2:4] == (2, 2)        # mapq 20 and the duplicate; not mapq 19
        assert al[404] == [(1, "G", 1), (16, P32[:16], 1), (17, P32[:17], 1), (32, P32, 1), (33, P32, 1), (100, P32, 1)]
        assert al[504] == [(33, P32, 2), (100, P32, 1)]
        assert al[604] == [(2, "CT", 1)] and al[623] == [(2, "TC", 1)] and al[644] == [(4, "NR=Y", 1)]
        assert al[664] == [(2, "GG", 2)] and al[684] == [(2, "AC", 2), (2, "CA", 1)]
        assert len(got) == 19 and res.observations.shape[0] == sum(r[2] for r in got.values()) == 32
        flt = eng.site_scan_ins(20, 1, 1, 1, ref, filter=(0x400, True))
        frow = {r[0] - 1: r for r in rows(flt.candidates)}
        assert frow[274][2:6] == (1, 1, 0, 1)                              # the anchor at 20 passes, the one at 19 does not
        assert frow[294][2:6] == (2, 2, 1, 1)                              # an anchor without a value passes
        assert frow[314][2:6] == (1, 1, 0, 1)
        assert [(a["count"], a["fwd"], a["rev"]) for a in V.ins_alleles(flt.observations) if a["pos"] == 665] == [(2, 1, 1)]
        assert [(a["seq"], a["fwd"], a["rev"]) for a in V.ins_alleles(flt.observations) if a["pos"] == 685] == [("AC", 1, 1), ("CA", 0, 1)]
        # ref_len < contig_len: nothing counts at or beyond it
        for r in (rec, only):
            eng.site_upload(L, short, r)
            eng.site_attach_quals(r, 20)
            check_ins(eng, L, ref[:short], r, 20, 20, filters=[(0, False), (0x704, True)], ranges=[(0, L), (short - 5, short + 5), (short, L), (short - 1, short)],
                      what="short reference")
        got = {r[0] - 1: r for r in rows(eng.site_scan_ins(20, 1, 1, 1, ref[:short]).candidates)}
        assert got[short - 1][2:4] == (1, 2) and max(got) == short - 1
        tail = eng.site_scan_ins(0, 1, 1, 1, ref[:short], short, L)
        assert (tail.low_depth, tail.kept, tail.inserted, tail.observations.shape[0]) == (L - short, 0, 0, 0)


def test_ins_scan_of_random_reads_and_of_an_unsorted_copy():
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
                assert check_ins(eng, L, ref, rec, 10, 20, ranges=ranges, what="random") > 1000
        # the same qualities and flags on both orders: attached by name
        plain = ContigRecords.from_reads([r[:3] + ([20 + (int(r[5][1:]) * 7) % 25] * max(0, len(r[6]) - int(r[5][1:]) % 4),
                                                   [0, 0x10, 0x400, 0x10][int(r[5][1:]) % 4]) + r[5:] for r in order])
        with Engine(CallableOptions(), 0) as eng:
            eng.site_upload(L, L, plain)
            eng.site_attach_quals(plain, 30)
            check_ins(eng, L, ref, plain, 10, 30, filters=[(0x704, True)], params=[(2, 1, 2500)], ranges=[(0, L), (W - 3, W + 3)], what=f"order {k}", plain=False)
            results.append([eng.site_scan_ins(10, 1, 1, 1, ref, filter=f) for f in (None, (0x704, True))])
    for a, b in zip(*results):
        assert (a.low_depth, a.kept, a.inserted) == (b.low_depth, b.kept, b.inserted) and np.array_equal(a.candidates, b.candidates) and a.inserted > 100
        assert np.array_equal(a.observations, b.observations) and a.observations.shape[0] >= a.inserted


def column(p, n_ins, depth, name):
    """depth reads with a base at p, n_ins of them with an insertion behind it; strands alternate."""
    return [(p - 1, "2M1I1M" if i < n_ins else "3M", 60, 30, 0x10 * (i & 1), f"{name}{i}", "ACGT" if i < n_ins else "ACT") for i in range(depth)]


def test_ins_scan_threshold_edges():
    L = 2 * W + 100
    ref = synth.make_reference(L, 9)
    cols = {10: (7, 10),           # 7 / 10: exactly 0.7
            20: (6, 10),           # one read below it
            30: (3, 3),            # exactly min_ins_count 3
            40: (2, 3),            # one below
            W - 1: (7, 10), W + 2: (6, 9),                             # depth 10 == min_depth, depth 9: low_depth
            W + 50: (1, 10)}                                 # 1 of 10 at 1000 per 10 000
    reads = sorted((r for p, (i, d) in cols.items() for r in column(p, i, d, f"c{p}_")), key=lambda r: r[0])
    rec = ContigRecords.from_reads(reads)
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        check_ins(eng, L, ref, rec, 20, 20, filters=[(0, False), (0x10, False)], params=[(1, 1, 1), (1, 1, 7000), (1, 3, 1), (10, 1, 1), (10, 3, 7000), (1, 1, 1000), (1, 1, 1001)],
                  ranges=[(0, L), (W - 1, W + 3)], what="edges")
        for flt in (None, (0, False)):
            def at(*prm):
                return {r[0] - 1 for r in rows(eng.site_scan_ins(20, *prm, ref, filter=flt).candidates)}
            assert at(1, 1, 1) == set(cols)
            assert at(1, 1, 7000) == {10, 30, W - 1}                    # 7 / 10 and 3 / 3; 6 / 10, 2 / 3 and 6 / 9 are below
            assert at(1, 3, 1) == {10, 20, 30, W - 1, W + 2}
            assert at(10, 1, 1) == {10, 20, W - 1, W + 50}
            got = eng.site_scan_ins(20, 10, 1, 1, ref, W + 2, W + 3, filter=flt)
            assert (got.low_depth, got.kept, got.inserted) == (1, 0, 0)
            assert W + 50 in at(1, 1, 1000) and W + 50 not in at(1, 1, 1001)
            assert I.classify(7, 10, 1, 1, 7000) == I.INSERTED and I.classify(6, 10, 1, 1, 7000) == I.KEPT


def test_ins_scan_one_deep_column_needs_64_bits():
    """2^20 reads over one position, 45 % of them with an insertion behind it: 10000 * ins is past 2^32.  The column is
    reported with exact counts and every observation; the same column with one inserting read fewer is not."""
    n = 1 << 20
    d = -(-4500 * n // 10000)                                            # the smallest count with 10000 d >= 4500 n: 471 860
    assert 10000 * d >= 4500 * n > 10000 * (d - 1) and 10000 * d > 1 << 32
    L = 2 * W
    is_ins = np.zeros(2 * n, bool)
    is_ins[:d] = True                                                    # d behind 1000 ...
    is_ins[n:n + d - 1] = True                                           # ... d - 1 behind 1500
    pos = np.concatenate([np.full(n, 999, np.int32), np.full(n, 1499, np.int32)])
    n_ops = np.where(is_ins, 3, 1)
    cigar_off = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.uint32)
    cigar = np.full(int(cigar_off[-1]), (1 << 4) | 0, np.uint32)         # ... 1M
    first = cigar_off[:-1].astype(np.int64)
    cigar[first[~is_ins]] = (3 << 4) | 0                                 # 3M
    cigar[first[is_ins]] = (2 << 4) | 0                                  # 2M 1I 1M
    cigar[first[is_ins] + 1] = (1 << 4) | 1
    n_bases = np.where(is_ins, 4, 3)
    base_off = np.concatenate([[0], np.cumsum(n_bases)]).astype(np.uint64)
    flag = ((np.arange(2 * n) % 3 == 0).astype(np.uint16) << np.uint16(4))
    codes = np.full(int(base_off[-1]), 2, np.uint8)                      # C everywhere ...
    is_a = is_ins & (np.arange(2 * n) % 4 == 1)
    codes[base_off[:-1].astype(np.int64)[is_a] + 2] = 1                  # ... but an inserted A in every fourth inserting read
    rec = ContigRecords(pos=pos, flag=flag, mapq=np.full(2 * n, 60, np.uint8), cigar_off=cigar_off, cigar=cigar, qual_off=base_off,
                        qual=np.full(int(base_off[-1]), 30, np.uint8), qname_off=np.arange(2 * n + 1, dtype=np.uint32),
                        qname=np.full(2 * n, ord("p"), np.uint8)).validate()
    rec.seq_off = base_off.copy()
    rec.seq4 = pack_seq4(codes)
    ref = synth.make_reference(L, 4)
    rev = flag != 0
    i_rev, d_rev = int((rev & is_ins)[:n].sum()), int(rev[:n].sum())
    a_all, a_rev = int(is_a[:n].sum()), int((is_a & rev)[:n].sum())
    assert I.classify(d, n, 10, 3, 4500) == I.INSERTED and I.classify(d - 1, n, 10, 3, 4500) == I.KEPT
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        for flt in (None, (0, False), (0, True)):
            strands = (0, 0, 0, 0) if flt is None else (d - i_rev, i_rev, n - d_rev, d_rev)
            got = eng.site_scan_ins(20, 10, 3, 4500, ref, filter=flt)
            assert (got.low_depth, got.kept, got.inserted) == (L - 6, 5, 1), flt
            assert rows(got.candidates) == [(1001, chr(ref[1000] & 0xDF), d, n) + strands], flt
            assert got.observations.shape[0] == d and (got.observations["pos"] == 1001).all() and (got.observations["len"] == 1).all()
            want = [dict(pos=1001, len=1, key=(2 << 60, 0), seq="C", count=d - a_all, fwd=d - a_all - (i_rev - a_rev), rev=i_rev - a_rev),
                    dict(pos=1001, len=1, key=(1 << 60, 0), seq="A", count=a_all, fwd=a_all - a_rev, rev=a_rev)]
            if flt is None:
                want = [dict(a, fwd=a["count"], rev=0) for a in want]
            assert V.ins_alleles(got.observations) == want, flt
            both = eng.site_scan_ins(20, 10, 3, 4499, ref, 900, 1600, filter=flt)
            assert [r[:4] for r in rows(both.candidates)] == [(1001, chr(ref[1000] & 0xDF), d, n), (1501, chr(ref[1500] & 0xDF), d - 1, n)], flt
            assert both.observations.shape[0] == 2 * d - 1 and int((both.observations["pos"] == 1501).sum()) == d - 1
            assert [a["count"] for a in V.ins_alleles(both.observations)][:2] == [d - a_all, a_all]


def test_ins_scan_grows_its_candidate_buffer_and_sizes_the_observations_exactly():
    """66 000 inserted positions from two reads of 1M1I over and over: more candidates than the buffer's first 65 536
    entries, 132 000 observations in a buffer of exactly that size."""
    n_ins = 66_000
    L = n_ins + 2
    seqs = ["AC" * n_ins + "A", "AG" * n_ins + "A"]                        # every inserted base is C in one read, G in the other
    reads = [(0, "1M1I" * n_ins + "1M", 60, 30, 0x10 * i, f"w{i}", seqs[i]) for i in range(2)] + [(5, "20M", 60, 30, 0, "m", "A" * 20)]
    rec = ContigRecords.from_reads(reads)
    ref = synth.make_reference(L, 6)
    depth, ins, events = I.walk(L, L, rec, 20)
    every = I.observations(events, rec, I.reduce(depth, ins, ref, L, 1, 1, 1, 0, L)["candidates"])
    assert len(every) == 2 * n_ins
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, 20)
        for flt in (None, (0, False)):
            full = every if flt is not None else sorted(o[:4] + (0,) for o in every)

            def want(a, b):
                # (under (1, 1, 1) the candidates of a range are the full scan's there, and so are their observations)
                return I.reduce(depth, ins, ref, L, 1, 1, 1, a, b, stranded=flt is not None), [o for o in full if a < o[0] <= b]
            exp, obs = want(0, L)
            assert exp["inserted"] == n_ins
            got = eng.site_scan_ins(20, 1, 1, 1, ref, filter=flt)
            same_ins(got, exp, obs, flt)
            assert np.array_equal(got.candidates["pos"], np.arange(1, n_ins + 1)) and got.kernel_ms > 0
            scan_ms, alleles_ms = eng.site_scan_ins_stats()
            assert scan_ms > 0 and alleles_ms > 0 and abs(scan_ms + alleles_ms - got.kernel_ms) < 1e-3 * got.kernel_ms
            # one position more than the first buffer holds, then a smaller range: the grown buffers serve it
            same_ins(eng.site_scan_ins(20, 1, 1, 1, ref, 0, 65_537, filter=flt), *want(0, 65_537), (flt, "65537"))
            same_ins(eng.site_scan_ins(20, 1, 1, 1, ref, 100, 1100, filter=flt), *want(100, 1100), (flt, "range"))
        al = V.ins_alleles(got.observations[:4])
        assert [(a["pos"], a["seq"], a["count"], a["fwd"], a["rev"]) for a in al] == [(1, "C", 1, 1, 0), (1, "G", 1, 0, 1), (2, "C", 1, 1, 0), (2, "G", 1, 0, 1)]


QUALS = [10, 19, 20, 30, 40]
# (1-based anchor, [(inserted bases, carriers)], strands): homoplasmic, heteroplasmic, forward only, two alleles
LOCI = [(3000, [("C", 60)], "both"), (5000, [("C", 25)], "both"), (8281, [("C", 60)], "fwd"), (12000, [("CC", 40), ("C", 18)], "both")]


def ins_sample(L, seed, n=3000, rl=100):
    """Reads of rl bases over a reference, a small insertion in one of ten, a deletion or a clip in a few; at LOCI sixty
    reads each, `carriers` of them with the insertion.  Qualities around 20, strands alternate, a few flagged reads."""
    ref = synth.make_reference(L, seed)
    text = bytes(ref & 0xDF).decode()
    rng = random.Random(seed + 1)
    reads = []

    def add(p, a, ins, name, strand, other=None):
        """a matched bases, `ins`, then the rest of the read's rl bases matched."""
        k = rng.random()
        flag = (0x10 if strand else 0) | (0x400 if k < 0.03 else 0x100 if k < 0.05 else 0)
        cigar = other or (f"{a}M{len(ins)}I{rl - a - len(ins)}M" if ins else f"{rl}M")
        seq = text[p:p + rl] if other else text[p:p + a] + ins + text[p + a:p + rl - len(ins)]
        reads.append((p, cigar, rng.choice([60, 60, 60, 30, 5]), rng.choices(QUALS, k=rl), flag, name, seq))

    for i in range(n):
        p = rng.randint(0, L - rl - 80)
        k = rng.random()
        a = rng.randint(5, rl - 10)
        if k < 0.85:
            add(p, 0, "", f"s{i}", i & 1)
        elif k < 0.95:
            add(p, a, "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 4))), f"s{i}", i & 1)
        elif k < 0.98:
            add(p, a, "", f"s{i}", i & 1, other=f"{a}M2D{rl - a}M")
        else:
            add(p, a, "", f"s{i}", i & 1, other=f"{a}S{rl - a}M")
    for locus, alleles, strands in LOCI:
        which = [s for s, c in alleles for _ in range(c)]
        for i in range(60):
            ins = which[i] if i < len(which) else ""
            add(locus - 50, 50, ins, f"l{locus}_{i}", 0 if strands == "fwd" and ins else i & 1)
    reads.sort(key=lambda r: r[0])
    return ref, ContigRecords.from_reads(reads)


def expect(L, rec, ref, mq, ex, mbq, prm, a=0, b=None, stranded=True):
    b = L if b is None else b
    depth, ins, events = I.walk(L, L, rec, mq, ex, mbq)
    exp = I.reduce(depth, ins, ref, L, *prm, a, b, stranded=stranded)
    return exp, I.observations(events, rec, exp["candidates"], stranded=stranded)


def test_ins_scan_invariants_and_interleaving():
    L = 20_000
    ref, rec = ins_sample(L, 40)
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
        dels0 = eng.site_scan_dels(20, 1, 1, 1, ref, filter=(0x704, True))
        c5, c9 = eng.site_scan_counts(20, 0, L), eng.site_scan_counts_ex(20, 0, L, 0x704, True)
        r1, r2, r3, r4 = _lib.cl_scan_result(), _lib.cl_scan_result_ex(), _lib.cl_minor_result(), _lib.cl_del_result()
        f704 = _lib.cl_scan_filter(0x704, 1, 0)
        prm, dprm = _lib.cl_minor_params(10, 3, 500), _lib.cl_del_params(1, 1, 1)
        assert lib.cl_site_scan(h, 20, 10, refp, L, 0, L, C.byref(r1)) == 0
        assert lib.cl_site_scan_ex(h, 20, 10, C.byref(f704), refp, L, 0, L, C.byref(r2)) == 0
        assert lib.cl_site_scan_minor(h, 20, C.byref(f704), C.byref(prm), refp, L, 0, L, C.byref(r3)) == 0
        assert lib.cl_site_scan_dels(h, 20, C.byref(f704), C.byref(dprm), refp, L, 0, L, C.byref(r4)) == 0

        def others():
            return [C.string_at(r1.candidates, int(r1.n_variant) * 28), C.string_at(r2.candidates, int(r2.n_variant) * 44),
                    C.string_at(r3.candidates, int(r3.n_minor) * 44), C.string_at(r4.candidates, int(r4.n_deleted) * 32)]
        keep = others()
        assert int(r4.n_deleted) > 50
        plain = eng.site_scan_ins(20, 10, 3, 7000, ref)
        off = eng.site_scan_ins(20, 10, 3, 7000, ref, filter=(0, False))
        on = eng.site_scan_ins(20, 10, 3, 7000, ref, filter=(0x704, True))
        every = eng.site_scan_ins(20, 1, 1, 1, ref, filter=(0x704, True))
        every_plain = eng.site_scan_ins(20, 1, 1, 1, ref)
        assert every.inserted > 100 and every_plain.inserted > every.inserted
        same_ins(every, *expect(L, rec, ref, 20, 0x704, 20, (1, 1, 1)), "every")
        assert keep == others()
        # the planted loci, by the default rule: the heteroplasmic one at 5000 is not among them
        assert [int(p) for p in plain.candidates["pos"]] == [3000, 8281, 12000] == [int(p) for p in on.candidates["pos"]]
        al = {}
        for a in V.ins_alleles(on.observations):
            al.setdefault(a["pos"], []).append(a)
        assert [a["seq"] for a in al[3000]] == ["C"] and [a["seq"] for a in al[12000]] == ["CC", "C"] and al[12000][0]["count"] > al[12000][1]["count"] > 5
        assert al[8281][0]["rev"] == 0 and al[8281][0]["fwd"] == int(on.candidates["ins_fwd"][1]) > 10 and int(on.candidates["ins_rev"][1]) == 0
        hetero = [r for r in rows(every.candidates) if r[0] == 5000]
        assert len(hetero) == 1 and 10 * hetero[0][2] < 7 * hetero[0][3] and hetero[0][2] > 5
        # filter {0, 0} and no filter agree in everything but the strand fields
        assert (plain.low_depth, plain.kept, plain.inserted) == (off.low_depth, off.kept, off.inserted)
        for f in FIELDS[:4]:
            assert np.array_equal(plain.candidates[f], off.candidates[f]), f
        for f in FIELDS[4:]:
            assert not plain.candidates[f].any()
        for f in ("pos", "len", "key"):
            assert np.array_equal(plain.observations[f], off.observations[f]), f       # (the strand is the last sort key)
        assert not plain.observations["strand"].any() and off.observations["strand"].any()
        # the strand counts add up, ins <= depth by strand, n_obs == sum(ins); a candidate's depth is the dense scan's depth there
        for res in (off, on, every):
            c = res.candidates
            assert np.array_equal(c["ins_fwd"].astype(np.int64) + c["ins_rev"], c["ins"]) and np.array_equal(c["depth_fwd"].astype(np.int64) + c["depth_rev"], c["depth"])
            assert (c["ins_fwd"] <= c["depth_fwd"]).all() and (c["ins_rev"] <= c["depth_rev"]).all()
            assert res.low_depth + res.kept + res.inserted == L and (np.diff(c["pos"].astype(np.int64)) > 0).all()
            assert res.observations.shape[0] == int(c["ins"].astype(np.int64).sum())
            assert np.array_equal(np.bincount(res.observations["pos"], minlength=L + 1)[c["pos"]], c["ins"])
            assert np.array_equal(np.bincount(res.observations["pos"], weights=res.observations["strand"], minlength=L + 1)[c["pos"]], c["ins_rev"])
        for res in (plain, every_plain):
            assert (res.candidates["ins"] <= res.candidates["depth"]).all() and res.observations.shape[0] == int(res.candidates["ins"].astype(np.int64).sum())
        assert np.array_equal(every.candidates["depth"], c9[every.candidates["pos"].astype(np.int64) - 1, 8])
        assert np.array_equal(on.candidates["depth"], c9[on.candidates["pos"].astype(np.int64) - 1, 8])
        assert np.array_equal(every_plain.candidates["depth"], c5[every_plain.candidates["pos"].astype(np.int64) - 1, 4])
        # ... and each equals the reference
        same_ins(on, *expect(L, rec, ref, 20, 0x704, 20, (10, 3, 7000)), "on")
        same_ins(plain, *expect(L, rec, ref, 20, 0, None, (10, 3, 7000), stranded=False), "plain")
        same_ins(every_plain, *expect(L, rec, ref, 20, 0, None, (1, 1, 1), stranded=False), "every, plain")
        ms, nbytes = eng.site_scan_stats()
        assert ms > 0 and nbytes > 20 * rec.n + 32 * every_plain.inserted + 32 * every_plain.observations.shape[0]
        scan_ms, alleles_ms = eng.site_scan_ins_stats()
        assert scan_ms > 0 and alleles_ms > 0 and abs(scan_ms + alleles_ms - ms) < 1e-3 * ms
        # the other calls after: the same results, and the insertion scan's own arrays stay as they are across them
        r5, iprm = _lib.cl_ins_result(), _lib.cl_ins_params(10, 3, 7000)
        assert lib.cl_site_scan_ins(h, 20, C.byref(f704), C.byref(iprm), refp, L, 0, L, C.byref(r5)) == 0
        keep_ins = (C.string_at(r5.candidates, int(r5.n_inserted) * 32), C.string_at(r5.obs, int(r5.n_obs) * 32))
        assert int(r5.n_inserted) == on.inserted and keep_ins == (on.candidates.tobytes(), on.observations.tobytes())
        assert keep == others()
        assert np.array_equal(eng.site_run(20, sites), run0)
        scan1, ex1 = eng.site_scan(20, 10, ref), eng.site_scan_ex(20, 10, ref, 0x704, True)
        for x, y in ((scan0, scan1), (ex0, ex1)):
            assert (x.low_depth, x.mixed, x.uncomparable, x.match, x.variant) == (y.low_depth, y.mixed, y.uncomparable, y.match, y.variant)
            assert np.array_equal(x.candidates, y.candidates)
        minor1 = eng.site_scan_minor(20, 10, 3, 500, ref, filter=(0x704, True))
        assert (minor0.low_depth, minor0.single, minor0.minor) == (minor1.low_depth, minor1.single, minor1.minor) and np.array_equal(minor0.candidates, minor1.candidates)
        dels1 = eng.site_scan_dels(20, 1, 1, 1, ref, filter=(0x704, True))
        assert (dels0.low_depth, dels0.kept, dels0.deleted) == (dels1.low_depth, dels1.kept, dels1.deleted) and np.array_equal(dels0.candidates, dels1.candidates)
        assert keep_ins == (C.string_at(r5.candidates, int(r5.n_inserted) * 32), C.string_at(r5.obs, int(r5.n_obs) * 32))
        assert np.array_equal(eng.site_scan_counts_ex(20, 0, L, 0x704, True), c9) and np.array_equal(eng.site_scan_counts(20, 0, L), c5)
        again = eng.site_scan_ins(20, 10, 3, 7000, ref, filter=(0x704, True))
        assert np.array_equal(again.candidates, on.candidates) and np.array_equal(again.observations, on.observations)
        # a range without a candidate: no observation, and the stats speak of the scan alone
        none = eng.site_scan_ins(20, 10, 3, 7000, ref, 100, 2000, filter=(0x704, True))
        assert (none.inserted, none.observations.shape[0]) == (0, 0) and eng.site_scan_ins_stats()[1] == 0.0


def test_ins_scan_refusals_leave_the_context_usable():
    L = 20_000
    ref, rec = ins_sample(L, 50, n=1500)
    sites = np.arange(1, 2000, 7, dtype=np.uint32)

    def refused(*a, **k):
        with pytest.raises(EngineError) as e:
            eng.site_scan_ins(*a, **k)
        assert e.value.status == -1 and len(str(e.value)) > len(" (cl_status -1)") + 10, str(e.value)
        return str(e.value)

    with Engine(CallableOptions(), 0) as eng:
        refused(20, 10, 3, 7000, ref)                                               # nothing resident
        eng.site_pileup(20, L, L, rec, sites)                                      # a tile filtered for its own list
        refused(20, 10, 3, 7000, ref)
        eng.site_upload(L, L, rec)
        assert "attach" in refused(20, 10, 3, 7000, ref, filter=(0, False))         # nothing attached
        ok = eng.site_scan_ins(20, 10, 3, 7000, ref)                               # the unfiltered form needs no attachment
        eng.site_attach_quals(rec, 20)
        for flt in (None, (0x704, True)):
            assert "min_depth" in refused(20, 0, 3, 7000, ref, filter=flt)
            assert "min_ins_count" in refused(20, 10, 0, 7000, ref, filter=flt)
            assert "min_ins_per_10k" in refused(20, 10, 3, 0, ref, filter=flt)
            assert "min_ins_per_10k" in refused(20, 10, 3, 10001, ref, filter=flt)
            refused(20, 10, 3, 7000, ref, 0, L + 1, filter=flt)                     # end > contig_len
            refused(20, 10, 3, 7000, ref, 10, 9, filter=flt)                        # start > end
            refused(20, 10, 3, 7000, ref[:L - 1], 0, L, filter=flt)                 # another ref_len
        out = _lib.cl_ins_result()
        st = eng._lib.cl_site_scan_ins(eng._h, 20, None, None, ref.ctypes.data, L, 0, L, C.byref(out))        # null params
        assert st == -1 and b"params" in eng._lib.cl_last_error(eng._h)
        prm = _lib.cl_ins_params(10, 3, 7000)
        assert eng._lib.cl_site_scan_ins(eng._h, 20, None, C.byref(prm), ref.ctypes.data, L, 0, L, None) == -1     # null result
        assert eng._lib.cl_site_scan_ins(eng._h, 20, None, C.byref(prm), None, L, 0, L, C.byref(out)) == -1        # null reference
        # the next valid calls succeed and equal the reference
        got = eng.site_scan_ins(20, 10, 3, 7000, ref)
        assert np.array_equal(got.candidates, ok.candidates) and np.array_equal(got.observations, ok.observations) and got.inserted == 3
        same_ins(eng.site_scan_ins(20, 10, 3, 10000, ref, filter=(0x704, True)), *expect(L, rec, ref, 20, 0x704, 20, (10, 3, 10000)), "after the refusals")
        same_ins(eng.site_scan_ins(20, 5, 2, 3000, ref, filter=(0x704, True)), *expect(L, rec, ref, 20, 0x704, 20, (5, 2, 3000)), "after the refusals, 0.3")
        empty = eng.site_scan_ins(20, 10, 3, 7000, ref, 5, 5, filter=(0x704, True))
        assert (empty.low_depth, empty.kept, empty.inserted, empty.candidates.shape[0], empty.observations.shape[0]) == (0, 0, 0, 0, 0)
    with HostStage(CallableOptions()) as hs:
        with pytest.raises(EngineError) as e:
            hs.site_scan_ins(20, 10, 3, 7000, ref)
        assert e.value.status == -2


def test_find_insertions_on_files_and_cli(tmp_path):
    L = 20_000
    ref, rec = ins_sample(L, 60)
    names = ["chr1", "chrM", "chrY"]; lens = [248956422, L, 57227415]
    bam = str(tmp_path / "i.bam"); fa = str(tmp_path / "i.fa")
    write_bam(bam, list(zip(names, lens)), {1: rec}, block_every=5000)
    write_fasta(fa, [("chrM", ref)])

    def want(mq=20, md=10, per=7000, cnt=3, mbq=None, ex=0, k=0, a=0, b=L):
        exp, obs = expect(L, rec, ref, mq, ex, mbq, (md, cnt, per), a, b)
        return I.expected_tsv("chrM", exp, obs, a, b, md, mq, mbq, ex, per, cnt, k), exp

    out = str(tmp_path / "o.tsv")
    w0, e0 = want()
    assert [c[0] for c in e0["candidates"]] == [3000, 8281, 12000] and "\t2\t2\tCC\t" in w0 and "\t1\t1\tC\t" in w0
    V.find_insertions(bam, fa, "chrM", out)
    assert open(out).read() == w0
    w1, e1 = want(mbq=20, ex=0x704, k=2, per=2500, cnt=2)
    assert e1["inserted"] > e0["inserted"] and 5000 in [c[0] for c in e1["candidates"]] and "\tstrand\n" in w1 and "\tPASS\n" in w1
    V.find_insertions(bam, fa, "chrM", out, min_ins_fraction="0.25", min_ins_count=2, min_base_quality=20, exclude_flags=0x704, min_ins_per_strand=2)
    assert open(out).read() == w1

    def cli(*args):
        return subprocess.run([_b.CLI, "find-insertions", bam, "-r", fa, "-o", out, "-L", "chrM"] + list(args), capture_output=True, text=True)

    r = cli()
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w0
    r = cli("--min-ins-fraction", "0.25", "--min-ins-count=2", "--min-base-quality", "20", "--exclude-flags", "0x704", "--min-ins-per-strand=2")
    assert r.returncode == 0, r.stderr
    assert open(out).read() == w1
    a, b = 3_500, 11_000                                                 # between the first two and the last two planted loci
    r = cli(f"--region={a}-{b}", "--min-depth", "12", "--min-quality=30", "--exclude-flags", "1796", "--min-ins-fraction=.3", "--min-ins-count", "1")
    assert r.returncode == 0, r.stderr
    w2, e2 = want(mq=30, md=12, per=3000, cnt=1, ex=0x704, a=a, b=b)
    assert open(out).read() == w2 and [c[0] for c in e2["candidates"]] == [5000, 8281]
    V.find_insertions(bam, fa, "chrM", out, region=(a, b), min_depth=12, min_quality=30, exclude_flags=0x704, min_ins_fraction=".3", min_ins_count=1)
    assert open(out).read() == w2
    # an unknown contig and a region beyond the contig: exit 1 with a message
    r = subprocess.run([_b.CLI, "find-insertions", bam, "-r", fa, "-o", out, "-L", "chrZ"], capture_output=True, text=True)
    assert r.returncode == 1 and "chrZ" in r.stderr
    r = cli(f"--region=0-{L + 1}")
    assert r.returncode == 1 and "beyond" in r.stderr
    with pytest.raises(EngineError):
        V.find_insertions(bam, fa, "chrZ", out)
