"""The inputs the short-tandem-repeat tests share (tests/test_str_host.py without a device, tests/test_gpu_str.py on one):
planted reads and loci, each named for what it pins, a generator of reads with every CIGAR operation at random places,
random loci, and the reference results over them by tests/str_ref.py -- computed once and left unchanged."""
import functools
import random
import re

import str_ref as R
from decodingustools_amd.records import ContigRecords

W = 1024                                    # the window of the scan's read index
L = 3 * W + 17
FLANKS = (1, 5, 64)
FILTERS = (None, 0, 0x704, 0xFFFF)          # None: the unfiltered form, one strand


def rd(pos, cigar, name, flag=0, mapq=60, n_bases=None):
    """A read of A's: as many bases as its CIGAR consumes, or n_bases of them."""
    q = sum(int(x[:-1]) for x in re.findall(r"\d+[MIDNSHP=X]", cigar) if x[-1] in "MIS=X")
    n = q if n_bases is None else n_bases
    return (pos, cigar, mapq, 30 if n else None, flag, name, "A" * n)


# name -> (start, end); the flank the names speak of is 5 unless they say otherwise
PLANTED_LOCI = {
    "ends-at-the-window-border": (1000, W),
    "starts-at-the-window-border": (W, W + 16),
    "straddles-the-window-border": (W - 9, W + 11),
    "s-below-the-flank": (3, 12),
    "s-equals-the-flank": (5, 14),
    "right-flank-ends-at-the-contig-end": (L - 15, L - 5),
    "right-flank-beyond-the-contig-end": (L - 13, L - 3),
    "ends-at-the-contig-end": (L - 10, L),
    "insertions": (200, 220),
    "deletions": (300, 320),
    "skips": (400, 420),
    "deltas": (500, 600),
    "read-boundaries": (700, 720),
    "gates": (800, 820),
    "deep": (900, 912),
    "one-base": (1500, 1501),
    "longest": (1600, 1600 + 1024),
}


def planted_reads():
    reads = [
        # locus placement
        rd(W - 39, "80M", "over-the-window-border"),
        rd(W - 39, "39M2I41M", "i-at-the-window-border", flag=0x10),          # x == 1024: e of one locus, s of the next, inside the third
        rd(W + 2, "60M", "second-window-only"),
        rd(0, "40M", "from-position-0"),                                       # s == 5: the left flank is [0, 5); s == 3: it cannot be matched
        rd(1, "40M", "from-position-1", flag=0x10),                            # s == 5: one base of the flank is missing
        rd(L - 49, "44M", "ends-at-l-minus-5"),                                # where the first of the three loci ends: its right flank is missing
        rd(L - 49, "60M", "hangs-over-the-contig-end", flag=0x10),             # matched past contig_len: spans all three loci by its CIGAR
        rd(L - 49, "49M", "ends-at-the-contig-end"),                           # e + F == contig_len: spanning; two positions further: partial
        # I placement around [200, 220)
        rd(150, "100M", "no-gap"),
        rd(150, "50M3I50M", "i-at-s", flag=0x10),
        rd(150, "70M3I30M", "i-at-e"),
        rd(150, "51M3I49M", "i-at-s-plus-1", flag=0x10),
        rd(150, "49M3I51M", "i-at-s-minus-1"),                                 # inside the flank of 5; outside the flank of 1
        rd(150, "45M3I55M", "i-at-s-minus-5", flag=0x10),                      # x == s - F: outside the flank of 5
        rd(150, "71M3I29M", "i-at-e-plus-1"),
        rd(150, "75M3I25M", "i-at-e-plus-5", flag=0x10),
        rd(150, "50M2I10M1I10M3I30M", "three-insertions-one-length"),          # + 6 wherever they stand
        # D placement around [300, 320)
        rd(250, "55M4D41M", "d-inside"),
        rd(250, "50M20D30M", "d-covers-the-locus-exactly", flag=0x10),         # delta == -(e - s)
        rd(250, "40M10D50M", "d-ends-at-s"),
        rd(250, "70M5D25M", "d-starts-at-e", flag=0x10),
        rd(250, "45M10D45M", "d-crosses-s"),
        rd(250, "55M2D3I40M", "d-then-i-inside", flag=0x10),
        # N
        rd(350, "55M4N41M", "n-inside"),
        rd(350, "46M3N51M", "n-in-the-left-flank", flag=0x10),                 # partial through m_left, not through skipped
        rd(350, "72M2N26M", "n-in-the-right-flank"),
        rd(350, "40M10N50M", "n-ends-at-s", flag=0x10),
        # delta = +63, +64, -63, -64 over [500, 600), and a 500-base insertion
        rd(450, "60M63I140M", "delta-plus-63"),
        rd(450, "60M64I140M", "delta-plus-64", flag=0x10),
        rd(450, "60M63D77M", "delta-minus-63"),
        rd(450, "60M64D76M", "delta-minus-64", flag=0x10),
        rd(450, "60M500I140M", "insertion-of-500"),
        # read boundaries around [700, 720)
        rd(695, "40M", "starts-at-s-minus-f"),
        rd(696, "40M", "starts-at-s-minus-f-plus-1", flag=0x10),
        rd(680, "45M", "ends-at-e-plus-f"),
        rd(680, "44M", "ends-at-e-plus-f-minus-1", flag=0x10),
        rd(690, "5S40M", "leading-s"),
        rd(690, "3H40M", "leading-h", flag=0x10),
        rd(690, "40M2P3S", "trailing-p-and-s"),
        rd(690, "40M", "no-stored-bases", n_bases=0),
        rd(690, "20M2I20M", "fewer-stored-bases-than-the-cigar", flag=0x10, n_bases=10),
        rd(705, "5I10M", "only-inside"),
        rd(690, "12I", "no-reference-span"),
        # gates around [800, 820)
        rd(780, "60M", "plain"),
        rd(780, "60M", "mapq-19", mapq=19),
        rd(780, "60M", "mapq-20", mapq=20, flag=0x10),
        rd(780, "60M", "reverse", flag=0x10),
        rd(780, "60M", "duplicate", flag=0x400),
        rd(780, "60M", "secondary", flag=0x100),
        rd(L + 5, "60M", "starts-beyond-the-contig"),
        rd(L, "60M", "starts-at-the-contig-end", flag=0x10),
        # one base and the longest locus
        rd(1490, "30M", "over-one-base"),
        rd(1490, "10M1D19M", "one-base-deleted", flag=0x10),
        rd(1530, "1200M", "over-the-longest-locus"),
        rd(1590, "600M7I500M", "plus-7-in-the-longest", flag=0x10),
    ]
    # 700 reads over [900, 912): more than two strides of the workgroup, two bins past 255
    reads += [rd(880, "25M4I25M" if i % 7 < 3 else "50M", f"deep-{i}", flag=0x10 * (i & 1)) for i in range(700)]
    return reads


def random_reads(n, seed):
    """Reads with every CIGAR operation at random places: clips in front and behind, insertions, deletions, skips and pads
    between matches of 1..90 bases, some reads without a reference span, some over the contig's end, some with fewer stored
    bases than the CIGAR consumes or none."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ops = []
        k = rng.random()
        if k < 0.1:
            ops.append(f"{rng.randint(1, 9)}H")
        if k < 0.25:
            ops.append(f"{rng.randint(1, 9)}S")
        if k < 0.08:
            ops.append(f"{rng.randint(1, 9)}I")
        if rng.random() < 0.97:
            for _ in range(rng.randint(1, 6)):
                ops.append(f"{rng.randint(1, 90)}{rng.choice('MMM=X')}")
                k = rng.random()
                if k < 0.35:
                    ops.append(f"{rng.choice([1, 1, 2, 3, 5, 8, 20, 63, 64, 70])}I")
                elif k < 0.6:
                    ops.append(f"{rng.choice([1, 1, 2, 3, 5, 8, 20, 63, 64, 70])}D")
                elif k < 0.7:
                    ops.append(f"{rng.randint(1, 120)}N")
                elif k < 0.75:
                    ops.append(f"{rng.randint(1, 4)}P")
                elif k < 0.8:
                    ops.append(f"{rng.randint(1, 5)}I"); ops.append(f"{rng.randint(1, 5)}D")
            if rng.random() < 0.7:
                ops.append(f"{rng.randint(1, 60)}M")
        if rng.random() < 0.2:
            ops.append(f"{rng.randint(1, 9)}S")
        cigar = "".join(ops) or "5S"
        k = rng.random()
        r = rd(rng.randint(0, L - 1), cigar, f"r{i}", flag=rng.choice([0, 0x10, 0, 0x10, 0x400, 0x110, 0x4]), mapq=rng.choice([0, 5, 19, 20, 40, 60]))
        n_bases = len(r[6])
        n_bases = 0 if k < 0.03 else rng.randint(0, n_bases) if k < 0.1 else n_bases
        out.append(rd(r[0], cigar, r[5], flag=r[4], mapq=r[2], n_bases=n_bases))
    return out


def random_loci(seed):
    """150 loci of span 1..40 and five of span 1000..1024, anywhere inside the contig, in no order."""
    rng = random.Random(seed)
    spans = [rng.randint(1, 40) for _ in range(150)] + [rng.randint(1000, 1024) for _ in range(4)] + [1024]
    rng.shuffle(spans)
    return [(s, s + span) for span in spans for s in [rng.randint(0, L - span)]]


class Case:
    """A tile (rec), its loci and the reference's results over them: expected(flank, min_quality, exclude_flags)."""

    def __init__(self, reads, loci, sort=True):
        self.reads = sorted(reads, key=lambda r: r[0]) if sort else list(reads)
        self.rec = ContigRecords.from_reads(self.reads)
        self.loci = [(int(s), int(e)) for s, e in loci]
        self.events = R.expand(self.rec)
        self._cache, self._done = {}, {}

    def expected(self, flank, min_quality, exclude_flags):
        key = (flank, min_quality, exclude_flags)
        if key not in self._done:
            hist, partial = R.measure(self.events, self.rec, L, self.loci, flank, min_quality, exclude_flags, cache=self._cache)
            hist.setflags(write=False); partial.setflags(write=False)
            self._done[key] = (hist, partial)
        return self._done[key]

    def index(self, name):
        return [r[5] for r in self.reads].index(name)


@functools.lru_cache(maxsize=None)
def planted():
    return Case(planted_reads(), list(PLANTED_LOCI.values()))


@functools.lru_cache(maxsize=None)
def randomised(seed):
    return Case(random_reads(300, seed), random_loci(seed + 100))


# (read, locus, flank) -> (spanning, delta or None): what the planted reads say by themselves, derived by hand from the rule
PINS = [
    ("over-the-window-border", "ends-at-the-window-border", 5, True, 0),
    ("over-the-window-border", "starts-at-the-window-border", 5, True, 0),
    ("i-at-the-window-border", "ends-at-the-window-border", 5, True, 2),      # I at x == e
    ("i-at-the-window-border", "starts-at-the-window-border", 5, True, 2),    # I at x == s
    ("i-at-the-window-border", "straddles-the-window-border", 5, True, 2),
    ("second-window-only", "starts-at-the-window-border", 5, False, None),
    ("from-position-0", "s-below-the-flank", 5, False, None),
    ("from-position-0", "s-below-the-flank", 1, True, 0),
    ("from-position-0", "s-equals-the-flank", 5, True, 0),
    ("from-position-1", "s-equals-the-flank", 5, False, None),
    ("ends-at-l-minus-5", "right-flank-ends-at-the-contig-end", 5, False, None),
    ("ends-at-the-contig-end", "right-flank-ends-at-the-contig-end", 5, True, 0),
    ("hangs-over-the-contig-end", "right-flank-beyond-the-contig-end", 5, True, 0),
    ("hangs-over-the-contig-end", "ends-at-the-contig-end", 5, True, 0),
    ("ends-at-the-contig-end", "ends-at-the-contig-end", 5, False, None),
    ("ends-at-the-contig-end", "right-flank-beyond-the-contig-end", 5, False, None),
    ("ends-at-the-contig-end", "right-flank-beyond-the-contig-end", 1, True, 0),
    ("no-gap", "insertions", 5, True, 0),
    ("i-at-s", "insertions", 5, True, 3),
    ("i-at-e", "insertions", 5, True, 3),
    ("i-at-s-plus-1", "insertions", 5, True, 3),
    ("i-at-s-minus-1", "insertions", 5, False, None),
    ("i-at-s-minus-1", "insertions", 1, True, 0),                             # s - 1 lies outside a flank of 1
    ("i-at-s-minus-5", "insertions", 5, True, 0),                             # x == s - F: outside the flank
    ("i-at-e-plus-1", "insertions", 5, False, None),
    ("i-at-e-plus-5", "insertions", 5, True, 0),
    ("three-insertions-one-length", "insertions", 5, True, 6),
    ("d-inside", "deletions", 5, True, -4),
    ("d-covers-the-locus-exactly", "deletions", 5, True, -20),
    ("d-ends-at-s", "deletions", 5, False, None),
    ("d-starts-at-e", "deletions", 5, False, None),
    ("d-crosses-s", "deletions", 5, False, None),
    ("d-then-i-inside", "deletions", 5, True, 1),
    ("n-inside", "skips", 5, False, None),
    ("n-in-the-left-flank", "skips", 5, False, None),
    ("n-in-the-left-flank", "skips", 1, True, 0),
    ("n-ends-at-s", "skips", 5, False, None),
    ("delta-plus-63", "deltas", 5, True, 63),
    ("delta-plus-64", "deltas", 5, True, 64),
    ("delta-minus-63", "deltas", 5, True, -63),
    ("delta-minus-64", "deltas", 5, True, -64),
    ("insertion-of-500", "deltas", 5, True, 500),
    ("starts-at-s-minus-f", "read-boundaries", 5, True, 0),
    ("starts-at-s-minus-f-plus-1", "read-boundaries", 5, False, None),
    ("ends-at-e-plus-f", "read-boundaries", 5, True, 0),
    ("ends-at-e-plus-f-minus-1", "read-boundaries", 5, False, None),
    ("leading-s", "read-boundaries", 5, True, 0),
    ("leading-h", "read-boundaries", 5, True, 0),
    ("no-stored-bases", "read-boundaries", 5, True, 0),
    ("fewer-stored-bases-than-the-cigar", "read-boundaries", 5, True, 2),
    ("only-inside", "read-boundaries", 5, False, None),
    ("over-one-base", "one-base", 5, True, 0),
    ("one-base-deleted", "one-base", 5, True, -1),
    ("over-the-longest-locus", "longest", 64, True, 0),
    ("plus-7-in-the-longest", "longest", 5, True, 7),
]
