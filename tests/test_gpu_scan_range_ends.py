"""The seams of the window scan that turns range ends into counts (-m gpu): a thread holds four positions, a wave 256, a
workgroup the window of 1024.  Runs of deleted and of matched positions start, end and cross exactly where one wave's last
thread hands its sum to the next wave (offsets 256, 512, 768) and where the window ends (1024); insertions are anchored on
both sides of each.  The deletion, insertion and consensus scans of both forms are compared exactly -- class counts, the
whole candidate list, the observations, the bytes -- with the independent references dels_ref, ins_ref and cons_ref."""
import numpy as np
import pytest

from test_gpu_consensus import check_cons
from test_gpu_del_scan import check_dels
from test_gpu_ins_scan import check_ins
from decodingustools_amd import CallableOptions, Engine, synth
from decodingustools_amd.records import ContigRecords

pytestmark = pytest.mark.gpu
W = 1024                                            # the kernel's window
L = 2 * W + 17
SEAMS = (256, 512, 768, 1024)
RANGES = [(0, L)] + [(s - 2, s + 2) for s in SEAMS]
MQ, MBQ = 20, 20
FILTER = (0x704, True)


def seam_reads():
    """Per seam s: a D that starts at s - 1, s, s + 1 and one that ends just before each of them; M runs whose first or last
    position is s - 1 or s; an I anchored at s - 1 and at s.  Strands alternate.  At every seam one carrier and one anchor
    have a base quality below MBQ: their pass bit is clear.  One D crosses all four waves of the second window."""
    reads = []

    def add(pos, cigar, n_bases, low=None):
        qual = [30] * n_bases
        if low is not None:
            qual[low] = MBQ - 1
        i = len(reads)
        reads.append((pos, cigar, 60, qual, 0x10 * (i & 1), f"s{i}", "ACGT"[i % 4] * n_bases))

    for s in SEAMS:
        for e in (s - 1, s, s + 1):
            add(e - 5, "5M3D5M", 10)                                     # the D starts at e: the +1 falls on e
            add(e - 8, "5M3D5M", 10)                                     # the D ends just before e: the -1 falls on e
        add(s - 5, "5M3D5M", 10, low=4)                                  # as the first one at s, its carrier below MBQ
        add(s - 1, "4M", 4); add(s, "4M", 4)                             # M runs that start at s - 1, s ...
        add(s - 4, "4M", 4); add(s - 3, "4M", 4)                         # ... and that end with s - 1, s
        add(s - 4, "4M2I3M", 9); add(s - 3, "4M2I3M", 9)                 # anchors s - 1, s
        add(s - 3, "4M2I3M", 9, low=3)                                   # the anchor s again, below MBQ
    add(W + 90, "10M800D10M", 20)                                        # [W + 100, W + 900): over all four waves
    add(W - 110, "10M300D10M", 20)                                       # [W - 100, W + 200): over the window's end
    reads.sort(key=lambda r: r[0])
    return reads


@pytest.fixture(scope="module")
def tile():
    rec = ContigRecords.from_reads(seam_reads())
    ref = synth.make_reference(L, 5, lowercase=True)
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, MBQ)
        yield eng, rec, ref


def test_deleted_runs_that_start_end_and_cross_at_every_seam(tile):
    eng, rec, ref = tile
    assert check_dels(eng, L, ref, rec, MQ, MBQ, filters=[FILTER], params=[(1, 1, 1)], ranges=RANGES, what="seams") > 2 * 1000
    # the tile is what seam_reads says, whatever the reference walk does: three of the six short deletions cover each of
    # s - 2 .. s + 1, the one whose carrier is below MBQ covers s and s + 1 without a filter
    for flt, low in ((None, 1), (FILTER, 0)):
        got = {int(c["pos"]) - 1: int(c["del"]) for c in eng.site_scan_dels(MQ, 1, 1, 1, ref, filter=flt).candidates}
        for s in SEAMS:
            over = 1 if s == W else 0                                     # the D over the window's end
            assert (got[s - 2], got[s - 1], got[s], got[s + 1]) == (3 + over, 3 + over, 3 + low + over, 3 + low + over), (flt, s)
        assert got[W + 100] == 2 and got[W + 200] == got[W + 511] == got[W + 513] == got[W + 899] == 1 and W + 900 not in got


def test_insertions_anchored_on_both_sides_of_every_seam(tile):
    eng, rec, ref = tile
    assert check_ins(eng, L, ref, rec, MQ, MBQ, filters=[FILTER], params=[(1, 1, 1)], ranges=RANGES, what="seams") > 2 * 3 * len(SEAMS)
    for flt, at_seam in ((None, 2), (FILTER, 1)):
        got = {int(c["pos"]) - 1: int(c["ins"]) for c in eng.site_scan_ins(MQ, 1, 1, 1, ref, filter=flt).candidates}
        for s in SEAMS:                                                   # (the anchor below MBQ counts only without a filter)
            assert got[s - 1] == 1 and got[s] == at_seam and s - 2 not in got and s + 1 not in got, (flt, s)


def test_consensus_bytes_around_every_seam(tile):
    eng, rec, ref = tile
    seen = check_cons(eng, L, ref, rec, MQ, MBQ, [None, FILTER], params=[(1, 1, 1), (2, 1, 2500)], ranges=RANGES, what="seams")
    # (reads over one column carry different bases: most covered columns are N, a called base is a column of one read)
    assert seen["-"] > 1000 and seen["n"] > 1000 and seen["N"] > 0 and any(b in seen for b in "ACGT"), seen
