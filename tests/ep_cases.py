"""The inputs the error-profile tests share (tests/test_ep_host.py without a device, tests/test_gpu_ep.py on one): a contig
of 5 000 positions -- five windows of the scan's read index -- with a reference that holds N, IUPAC codes and lower case;
planted reads, each named for what it pins; seeded random reads with every CIGAR operation at random places; single reads
with hand-derived tables (PINS); and the reference results over them by tests/ep_ref.py, computed once and left unchanged."""
import functools
import random
import re

import numpy as np

import ep_ref as R
from decodingustools_amd.records import SEQ_CODES, ContigRecords

W = 1024                                    # the window of the scan's read index
L = 5000
CYCLES = (1, 7, 201, 256)                   # 201: above the longest read (200 stored bases); 256: the largest table
QUALS = (0, 20)
MBQ = 20                                    # the threshold the attachment is built with
# (exclude_flags, use_base_quality); None: the unfiltered form
FILTERS = (None, (0, False), (0x704, False), (0x704, True))
RANGES = ((0, L), (500, 3100), (W, 2 * W), (2 * W - 1, 2 * W + 1), (1500, 1500), (4090, L))


def make_ref(seed=11):
    rng = random.Random(seed)
    ref = [rng.choice("ACGT") for _ in range(L)]
    for p in range(300, 330):
        ref[p] = ref[p].lower()                                               # lower case counts as its letter
    for p in (400, 401, 1023, 1024, 2500):
        ref[p] = "N"
    for p, c in ((410, "R"), (411, "y"), (3071, "M"), (2048, "n")):
        ref[p] = c
    return np.frombuffer("".join(ref).encode(), np.uint8).copy()


REF = make_ref()
COMPLEMENT = {"A": "C", "C": "G", "G": "T", "T": "A"}                         # (not the complement: any other base, a mismatch to plant)


def rd(pos, cigar, name, flag=0, mapq=60, quals=30, n_bases=None, edits=(), rng=None):
    """A read that follows the reference over its matches (another base where the reference has none), with bases of
    `rng` (or A) in insertions and clips; edits: (query index, base or 4-bit code letter) to plant.  n_bases: fewer stored
    bases than the CIGAR consumes, or none.  quals: one value, a list (any length), or None."""
    seq, x = [], pos
    for l, op in ((int(t[:-1]), t[-1]) for t in re.findall(r"\d+[MIDNSHP=X]", cigar)):
        if op in "M=X":
            for p in range(x, x + l):
                c = chr(REF[p]).upper() if 0 <= p < L else "A"
                seq.append(c if c in "ACGT" else "G")
            x += l
        elif op in "IS":
            seq += [rng.choice("ACGT") if rng else "A" for _ in range(l)]
        elif op in "DN":
            x += l
    for q, c in edits:
        if q < len(seq):
            seq[q] = COMPLEMENT.get(seq[q], "T") if c == "*" else c
    if n_bases is not None:
        seq = seq[:n_bases]
    if not seq:
        quals = None
    return (pos, cigar, mapq, quals, flag, name, "".join(seq))


def planted_reads():
    around = [19, 20, 21, 255, 0, 20, 19, 40]
    reads = [
        rd(1000, "100M", "over-a-window-border", edits=[(0, "*"), (23, "*"), (24, "*"), (99, "*")]),
        rd(980, "40M10D50M", "d-straddles-a-border", flag=0x10),              # first deleted position 1020: the window below
        rd(2000, "48M5D40M", "d-begins-at-a-windows-first-position"),         # x == 2048
        rd(2040, "8M3D40M", "d-begins-at-a-windows-first-position-reverse", flag=0x10),
        rd(3000, "72M3I20M", "i-anchored-at-a-windows-last-position"),        # anchor 3071
        rd(3060, "12M2I30M", "i-anchored-at-a-windows-last-position-reverse", flag=0x10),
        rd(3072, "10M1I10M", "starts-at-a-windows-first-position"),
        rd(150, "5I50M", "leading-i"),                                        # not behind a match: no event
        rd(150, "4D50M", "leading-d", flag=0x10),                             # no carrier: no event
        rd(160, "3S4D50M", "d-behind-a-clip"),                                # its carrier is the last clipped base
        rd(200, "5S40M6S", "clips-forward", edits=[(5, "*"), (44, "*")]),
        rd(200, "5S40M6S", "clips-reverse", flag=0x10, edits=[(5, "*"), (44, "*")]),
        rd(260, "3H40M2H", "hard-clips", flag=0x10, edits=[(0, "*")]),
        rd(290, "20M30N20M", "skip-over-lower-case", edits=[(19, "*"), (20, "*")]),
        rd(295, "10=1X10=", "eq-and-x", flag=0x10, edits=[(10, "*")]),
        rd(380, "20M2I20M", "fewer-stored-bases-than-the-cigar", n_bases=10),  # the I and the second M hold no base
        rd(380, "20M2I20M", "stored-bases-end-inside-the-insertion", flag=0x10, n_bases=21),
        rd(380, "20M2D20M", "stored-bases-end-at-the-deletion", n_bases=20),  # y == L: the carrier is the last stored base
        rd(380, "40M", "no-stored-bases", n_bases=0),
        rd(395, "30M", "over-n-and-iupac-in-the-reference", edits=[(3, "N"), (4, "R"), (10, "="), (16, "Y")]),
        rd(390, "12M1I20M", "i-anchored-on-an-n-of-the-reference", flag=0x10),
        rd(2490, "10M4D20M", "d-at-an-n-of-the-reference"),
        rd(L - 30, "60M", "over-the-contig-end"),
        rd(L - 40, "20M5I30M", "insertion-before-the-contig-end", flag=0x10),
        rd(L, "40M", "starts-at-the-contig-end"),
        rd(L + 5, "40M", "starts-beyond-the-contig-end", flag=0x10),
        rd(4870, "60M", "runs-past-a-short-reference"),                       # ref_len 4900: thirty bases count
        rd(4890, "9M2I30M", "i-anchored-at-a-short-references-last-position"),  # anchor 4898; 4899 is the last
        rd(4890, "10M3D30M", "d-begins-at-a-short-references-end", flag=0x10),  # x == 4900: outside
        rd(4895, "5M1I30M", "i-anchored-just-inside-a-short-reference"),      # anchor 4899
        rd(600, "1M1D" * 100 + "1M1I" * 30 + "10M", "more-than-255-operations"),
        rd(650, "1M1D" * 70 + "2M1D" * 60 + "5M", "more-than-255-operations-reverse", flag=0x10, edits=[(0, "*"), (190, "*")]),   # 261 operations, 195 bases
        rd(800, "200M", "the-longest-read", edits=[(0, "*"), (199, "*"), (100, "N")]),
        rd(800, "50M", "mapq-19", mapq=19, edits=[(7, "*")]),
        rd(800, "50M", "mapq-20", mapq=20, flag=0x10, edits=[(7, "*")]),
        rd(800, "50M", "duplicate", flag=0x400, edits=[(8, "*")]),
        rd(800, "50M", "secondary-reverse", flag=0x110, edits=[(9, "*")]),
        rd(800, "50M", "qc-fail", flag=0x200, edits=[(10, "*")]),
        rd(820, "8M", "qualities-around-the-threshold", quals=around, edits=[(0, "*"), (1, "*"), (3, "*")]),
        rd(820, "4M2I4M", "anchor-below-the-threshold", quals=[30, 30, 30, 19, 30, 30, 30, 30, 30, 30]),
        rd(820, "4M2I4M", "anchor-at-the-threshold", flag=0x10, quals=[30, 30, 30, 20, 0, 0, 30, 30, 30, 30]),
        rd(820, "4M2D4M", "carrier-below-the-threshold", quals=[30, 30, 30, 19, 30, 30, 30, 30]),
        rd(820, "4M2D4M", "carrier-without-a-quality", flag=0x10, quals=[30, 30, 30]),
        rd(830, "12M", "fewer-qualities-than-bases", quals=[10, 10, 10], edits=[(1, "*"), (5, "*")]),
        rd(830, "12M", "no-qualities", quals=[], flag=0x10, edits=[(2, "*")]),
        rd(-5, "40M", "negative-start"),
        rd(2100, "10M0D5M0I5M1I0M2I4M", "zero-length-operations"),            # the 2I stands behind a match of no base
        rd(2200, "10M2I3I10M", "two-insertions-in-a-row"),                    # the second stands behind an insertion
        rd(2300, "10M2P3I10M", "pad-between-match-and-insertion", flag=0x10),
        rd(2400, "10M2D3D10M", "two-deletions-in-a-row"),                     # two events, one carrier
        rd(2450, "12I", "no-reference-span"),
    ]
    # 700 reads over one window: more than two strides of a workgroup; a mismatch planted at query index 0 of every tenth
    rng = random.Random(5)
    for i in range(700):
        p = 1100 + i % 30
        edits = [(0, "*")] if i % 10 == 0 else [(rng.randrange(50), "*")] if i % 3 == 0 else []
        reads.append(rd(p, "50M" if i % 7 else "20M1I10M2D19M", f"deep-{i}", flag=0x10 * (i & 1) | (0x400 if i % 50 == 49 else 0), mapq=60 if i % 40 else 10,
                        quals=[(13 * i + 7 * k) % 45 for k in range(50)], edits=edits))
    return reads


def random_reads(n, seed):
    """Reads with every CIGAR operation at random places: clips, insertions, deletions, skips and pads between matches of
    1..60 bases, at most 200 stored bases; some without a reference span, some over the contig's end, some with fewer
    stored bases than the CIGAR consumes or none, some with fewer qualities than bases; random codes now and then."""
    rng = random.Random(seed)
    reads = []
    for i in range(n):
        ops, stored = [], 0
        if rng.random() < 0.2:
            ops.append(f"{rng.randint(1, 5)}H")
        if rng.random() < 0.3:
            l = rng.randint(1, 8); ops.append(f"{l}S"); stored += l
        for _ in range(rng.randint(0, 6)):
            l = rng.randint(1, 60)
            if stored + l > 180:
                break
            ops.append(f"{l}{rng.choice('MMMM=X')}"); stored += l
            k = rng.random()
            if k < 0.25:
                l = rng.randint(0, 6); ops.append(f"{l}I"); stored += l
            elif k < 0.5:
                ops.append(f"{rng.randint(0, 40)}D")
            elif k < 0.6:
                ops.append(f"{rng.randint(1, 300)}N")
            elif k < 0.65:
                ops.append(f"{rng.randint(1, 3)}P")
        if rng.random() < 0.3:
            l = rng.randint(1, 8); ops.append(f"{l}S"); stored += l
        if not ops:
            ops = ["7I"]
        k = rng.random()
        n_bases = None if k < 0.85 else 0 if k < 0.9 else rng.randint(1, 40)
        edits = [(rng.randrange(200), rng.choice("*****NR=")) for _ in range(rng.randint(0, 4))]
        quals = [rng.choice((0, 10, 19, 20, 21, 35, 255)) for _ in range(rng.choice((0, 5, 200)))] if rng.random() < 0.8 else 30
        pos = rng.choice((rng.randint(0, L - 1), rng.randint(W - 80, W + 5), rng.randint(L - 100, L + 20), rng.randint(4850, 4910)))
        reads.append(rd(pos, "".join(ops), f"rnd-{seed}-{i}", flag=rng.choice((0, 0x10, 0x10, 0, 0x400, 0x110, 0x4)), mapq=rng.choice((60, 60, 60, 20, 19, 0)),
                        quals=quals, n_bases=n_bases, edits=edits, rng=rng))
    return reads


class Case:
    """Reads as ContigRecords (coordinate sorted unless sort=False), their expansion by the reference, and the reference's
    results, each computed once."""

    def __init__(self, reads, ref_len=L, sort=True):
        self.reads = sorted(reads, key=lambda r: r[0]) if sort else list(reads)
        self.rec = ContigRecords.from_reads(self.reads)
        self.ref_len = ref_len
        self.events = R.expand(self.rec)
        self._seen = {}

    def expected(self, n_cycles, min_quality, flt, start=0, end=L):
        key = (n_cycles, min_quality, flt, start, end)
        if key not in self._seen:
            ex, bq = (None, None) if flt is None else (flt[0], MBQ if flt[1] else None)
            self._seen[key] = R.profile(self.events, self.rec, L, REF, self.ref_len, start, end, n_cycles, min_quality, ex, bq)
        return self._seen[key]

    @property
    def ref(self):
        return REF[:self.ref_len]


@functools.lru_cache(maxsize=None)
def planted(ref_len=L):
    return Case(planted_reads(), ref_len)


@functools.lru_cache(maxsize=None)
def randomised(seed):
    return Case(random_reads(400, seed), L if seed % 2 else 4900)


def all_cases():
    return [("planted", planted()), ("planted-short-reference", planted(4900)), ("random-1", randomised(1)), ("random-2", randomised(2))]


# ---- single reads with tables derived by hand, each alone on a tile of PIN_L positions over PIN_REF, C = 4, mapq 20 ------
# A pin: (name, read, filter, expected).  expected: the scalars that are not zero and, per table, its cells that are not
# zero -- total {"X>Y": n}, from5 / from3 {(cycle, "X>Y"): n} and ins5 / ins3 / del5 / del3 {cycle: n}, cycles 0-based.
PIN_L = 64
PIN_REF = np.frombuffer(("ACGT" * 16).encode(), np.uint8).copy()
PIN_C = 4


def pin_read(pos, cigar, seq, flag=0, quals=30):
    return (pos, cigar, 60, quals, flag, "pin", seq)


PINS = [
    # ref[4:10] = ACGTAC; the read says ACGAAC: T>A at query index 3.  Forward: d5 = q, d3 = 5 - q.
    ("forward-one-mismatch", pin_read(4, "6M", "ACGAAC"), (0, False),
     dict(reads=1, bases=6, total={"A>A": 2, "C>C": 2, "G>G": 1, "T>A": 1},
          from5={(0, "A>A"): 1, (1, "C>C"): 1, (2, "G>G"): 1, (3, "T>A"): 1},
          from3={(0, "C>C"): 1, (1, "A>A"): 1, (2, "T>A"): 1, (3, "G>G"): 1})),
    # the same read reverse: every pair complemented (A>A -> T>T, C>C -> G>G, G>G -> C>C, T>A -> A>T), d5 = 5 - q, d3 = q
    ("reverse-one-mismatch", pin_read(4, "6M", "ACGAAC", flag=0x10), (0, False),
     dict(reads=1, bases=6, total={"T>T": 2, "G>G": 2, "C>C": 1, "A>T": 1},
          from5={(0, "G>G"): 1, (1, "T>T"): 1, (2, "A>T"): 1, (3, "C>C"): 1},
          from3={(0, "T>T"): 1, (1, "G>G"): 1, (2, "C>C"): 1, (3, "A>T"): 1})),
    # ... and without a filter the flag is not read: the forward tables
    ("reverse-flag-unfiltered", pin_read(4, "6M", "ACGAAC", flag=0x10), None,
     dict(reads=1, bases=6, total={"A>A": 2, "C>C": 2, "G>G": 1, "T>A": 1},
          from5={(0, "A>A"): 1, (1, "C>C"): 1, (2, "G>G"): 1, (3, "T>A"): 1},
          from3={(0, "C>C"): 1, (1, "A>A"): 1, (2, "T>A"): 1, (3, "G>G"): 1})),
    # 2S3M2I2M1D2M at 8, L = 11.  Aligned: q 2..4 over ref[8:11] = ACG, q 7..8 over ref[11:13] = TA, q 9..10 over
    # ref[14:16] = GT (position 13 deleted).  Insertion: anchor q 4 (d5 4, d3 6: outside C = 4), 2 bases.  Deletion:
    # carrier q 8 (d5 8, d3 2), 1 base.  from5 sees q 2, 3 (d5 < 4), from3 q 7..10 (d3 = 10 - q < 4).
    ("clips-insertion-deletion", pin_read(8, "2S3M2I2M1D2M", "TTACGCCTAGT"), (0, False),
     dict(reads=1, bases=7, ins=1, ins_bases=2, dels=1, del_bases=1, total={"A>A": 2, "C>C": 1, "G>G": 2, "T>T": 2},
          from5={(2, "A>A"): 1, (3, "C>C"): 1}, from3={(3, "T>T"): 1, (2, "A>A"): 1, (1, "G>G"): 1, (0, "T>T"): 1}, del3={2: 1})),
    # the same reverse: d5 = 10 - q, d3 = q.  Anchor q 4: d5 6, d3 4 -- both outside.  Carrier q 8: d5 2.  from5 sees q 7..10
    # complemented (T>T -> A>A, A>A -> T>T, G>G -> C>C, T>T -> A>A), from3 q 2, 3 (A>A -> T>T, C>C -> G>G).
    ("clips-insertion-deletion-reverse", pin_read(8, "2S3M2I2M1D2M", "TTACGCCTAGT", flag=0x10), (0, False),
     dict(reads=1, bases=7, ins=1, ins_bases=2, dels=1, del_bases=1, total={"T>T": 2, "G>G": 1, "C>C": 2, "A>A": 2},
          from5={(3, "A>A"): 1, (2, "T>T"): 1, (1, "C>C"): 1, (0, "A>A"): 1}, from3={(2, "T>T"): 1, (3, "G>G"): 1}, del5={2: 1})),
    # 3M1I2M at 4 with an N at q 1 and qualities 30 30 10 30 30 30 under the base-quality filter (threshold 20): q 0 A>A,
    # q 1 not comparable, q 2 (the anchor) fails: neither its base nor the insertion counts; q 4, 5 over ref[7:9] = TA
    ("n-and-a-failing-anchor", pin_read(4, "3M1I2M", "ANGCTA", quals=[30, 30, 10, 30, 30, 30]), (0, True),
     dict(reads=1, bases=3, uncomparable=1, total={"A>A": 2, "T>T": 1},
          from5={(0, "A>A"): 1}, from3={(1, "T>T"): 1, (0, "A>A"): 1})),
]


def pin_expected(want):
    """A pin's expected cells as the dict ep_ref.profile returns."""
    out = dict(start=0, end=PIN_L, n_cycles=PIN_C, reads=0, bases=0, uncomparable=0, ins=0, ins_bases=0, dels=0, del_bases=0,
               total=np.zeros((4, 4), np.uint64), from5=np.zeros((PIN_C, 4, 4), np.uint64), from3=np.zeros((PIN_C, 4, 4), np.uint64),
               ins5=np.zeros(PIN_C, np.uint64), ins3=np.zeros(PIN_C, np.uint64), del5=np.zeros(PIN_C, np.uint64), del3=np.zeros(PIN_C, np.uint64))
    for k, v in want.items():
        if k == "total":
            for cell, n in v.items():
                out[k][divmod(R.CELLS.index(cell), 4)] = n
        elif k in ("from5", "from3"):
            for (d, cell), n in v.items():
                out[k][(d,) + divmod(R.CELLS.index(cell), 4)] = n
        elif k in R.TABLES:
            for d, n in v.items():
                out[k][d] = n
        else:
            out[k] = v
    return out


assert all(c in SEQ_CODES for c in "ACGTNRY=")
