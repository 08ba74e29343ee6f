"""The inputs the linked-sites tests share (tests/test_link_host.py without a device, tests/test_gpu_link.py on one): a contig
of 20 000 positions; planted reads, each named for the corner of the rule it pins, with what it observes at its own sites
derived by hand (PINS); reads planted for the shapes of the kernel; seeded random reads with every CIGAR operation at random
places over a dense cluster of sites; and the reference results over them by tests/link_ref.py, computed once and left
unchanged.  The rule never reads the reference sequence, so every read spells its own bases."""
import functools
import random
import re

import numpy as np

import link_ref as R
from decodingustools_amd.records import SEQ_CODES, ContigRecords

W = 1024                                    # the window of the scan's read index
L = 20_000
MBQ = 20                                    # the threshold the attachment is built with
QUALS = (0, 20)
# (exclude_flags, use_base_quality); None: the unfiltered form
FILTERS = (None, (0, False), (0x704, False), (0x704, True))


def query_length(cigar):
    return sum(int(t[:-1]) for t in re.findall(r"\d+[MIDNSHP=X]", cigar) if t[-1] in "MIS=X")


def rd(pos, cigar, name, seq=None, flag=0, mapq=60, quals=30, rng=None):
    """(pos, cigar, mapq, quals, flag, name, seq).  seq: the stored bases; None: the bases ACGT in turn by query index (or
    of rng)."""
    if seq is None:
        n = query_length(cigar)
        seq = "".join(rng.choice("ACGT") if rng else "ACGT"[q & 3] for q in range(n))
    return (pos, cigar, mapq, quals if seq else None, flag, name, seq)


# ---- single reads with observations derived by hand ---------------------------------------------------------------------
# A pin: (name, read, sites, filter, min_quality, what the read observes at each site: a class name or None).  The counts
# follow: site i gains one in its class when the read observes one there; pair (i, j) of the pair set gains one in
# (class at i, class at j) when it observes one at both.  Under max_dist 1000 and max_partners 15 every site of a pin is a
# partner of every site in front of it.
def pin(pos, cigar, seq, flag=0, mapq=60, quals=30):
    return rd(pos, cigar, "pin", seq=seq, flag=flag, mapq=mapq, quals=quals)


PINS = [
    # 10M at 100: query index = position - 100.  109 is the last position of the span; at 110 the read has just ended
    ("first-and-last-position-and-just-behind", pin(100, "10M", "ACGTACGTAC"), [100, 109, 110], None, 20, ["A", "C", None]),
    # 4M3D4M at 200: 200..203 = q 0..3, 204..206 deleted (carrier q 3), 207..210 = q 4..7
    ("deletion-with-a-carrier", pin(200, "4M3D4M", "ACGTTGCA"), [203, 204, 206, 207], (0, False), 20, ["T", "del", "del", "T"]),
    # a leading D has no carrier (y = 0): the read covers 300..302 and observes nothing there
    ("leading-deletion", pin(300, "3D5M", "ACGTA"), [300, 302, 303], None, 20, [None, None, "A"]),
    # the carrier q 3 has quality 10 < 20: neither its own base nor the deletion it carries is seen; q 4 = T at 406
    ("deletion-whose-carrier-fails", pin(400, "4M2D4M", "ACGTTGCA", quals=[30, 30, 30, 10, 30, 30, 30, 30]), [403, 404, 405, 406], (0, True), 20,
     [None, None, None, "T"]),
    # ... and without use_base_quality the same read shows all four
    ("deletion-whose-carrier-fails-unasked", pin(400, "4M2D4M", "ACGTTGCA", quals=[30, 30, 30, 10, 30, 30, 30, 30]), [403, 404, 405, 406], (0, False), 20,
     ["T", "del", "del", "T"]),
    # 4M10N4M at 500: 504..513 skipped, 514 = q 4
    ("skip", pin(500, "4M10N4M", "ACGTTGCA"), [503, 505, 514], None, 20, ["T", None, "T"]),
    # five stored bases under 10M: 604 = q 4 exists, 605 = q 5 does not
    ("fewer-stored-bases-than-the-cigar", pin(600, "10M", "ACGTA"), [604, 605], None, 20, ["A", None]),
    ("no-stored-bases", pin(600, "10M", ""), [604, 605], (0, False), 20, [None, None]),
    # N (code 15) and R (an IUPAC code) are `other`
    ("n-and-iupac", pin(700, "4M", "ANRC"), [700, 701, 702, 703], None, 20, ["A", "other", "other", "C"]),
    # 2S3M2I3M at 800: q 0..1 clipped, 800..802 = q 2..4 (A C G), q 5..6 inserted, 803..805 = q 7..9 (T C A)
    ("clip-and-insertion-shift-the-query-index", pin(800, "2S3M2I3M", "TTACGGGTCA"), [800, 802, 803, 805], (0, False), 20, ["A", "G", "T", "A"]),
    ("below-min-quality", pin(900, "4M", "ACGT", mapq=19), [900, 901], None, 20, [None, None]),
    ("below-min-quality-unasked", pin(900, "4M", "ACGT", mapq=19), [900, 901], None, 0, ["A", "C"]),
    ("negative-start", pin(-5, "40M", "ACGT" * 10), [0, 10], None, 0, [None, None]),
    ("excluded-flag", pin(950, "4M", "ACGT", flag=0x400), [950, 953], (0x704, False), 20, [None, None]),
    ("excluded-flag-unmasked", pin(950, "4M", "ACGT", flag=0x400), [950, 953], (0, False), 20, ["A", "T"]),
    ("excluded-flag-unfiltered", pin(950, "4M", "ACGT", flag=0x400), [950, 953], None, 20, ["A", "T"]),
    # the pass bit clear at the anchor only: the partner is still counted as a site of its own, the pair gains nothing
    ("anchor-fails", pin(1000, "4M", "ACGT", quals=[10, 30, 30, 30]), [1000, 1002], (0, True), 20, [None, "G"]),
    ("partner-fails", pin(1000, "4M", "ACGT", quals=[30, 30, 10, 30]), [1000, 1002], (0, True), 20, ["A", None]),
    # fewer quality values than bases: a base without one passes
    ("base-without-a-quality", pin(1000, "4M", "ACGT", quals=[30, 10]), [1000, 1001, 1003], (0, True), 20, ["A", None, "T"]),
    ("eq-and-x", pin(1100, "2=1X2=", "ACGTA"), [1100, 1102, 1104], None, 20, ["A", "G", "A"]),
    # 1022..1025 over a window border: the read lies in both windows of the index
    ("over-a-window-border", pin(1020, "8M", "ACGTACGT"), [1023, 1024], None, 20, ["T", "A"]),
]
PIN_D, PIN_K = 1000, 15


def pin_expected(sites, seen, max_dist=PIN_D, max_partners=PIN_K):
    """A pin's counts as the dict link_ref.counts returns, from what the read observes."""
    first = R.pair_set(sites, max_dist, max_partners)
    tables = np.zeros((int(first[-1]), 6, 6), np.uint32)
    site_counts = np.zeros((len(sites), 6), np.uint32)
    for i, a in enumerate(seen):
        if a is None:
            continue
        site_counts[i, R.CLASSES.index(a)] = 1
        for k in range(int(first[i + 1]) - int(first[i])):
            b = seen[i + 1 + k]
            if b is not None:
                tables[int(first[i]) + k, R.CLASSES.index(a), R.CLASSES.index(b)] = 1
    return dict(first=first, tables=tables, site_counts=site_counts)


# ---- the planted case: every pin together, and reads for the shapes of the kernel -------------------------------------------
CLUSTER = list(range(3000, 3034, 2))        # 17 sites: the first has 15 partners and a 16th site within max_dist
DEEP = (6000, 6010)                         # one pair under 700 reads
LONELY = 9000                               # an anchor without partners, with reads
EMPTY = 15_000                              # an anchor in a window without reads


def planted_reads():
    reads = [rd(r[0], r[1], name, seq=r[6], flag=r[4], mapq=r[2], quals=r[3]) for name, r, _, _, _, _ in PINS]
    reads += [rd(L, "40M", "starts-at-the-contig-end"), rd(L + 5, "40M", "starts-beyond-the-contig-end", flag=0x10),
              rd(L - 30, "60M", "over-the-contig-end"), rd(2450, "12I", "no-reference-span"),
              rd(1010, "1M1D" * 140 + "10M", "more-than-255-operations")]                   # over 1023, 1024, 1030 with gaps at the odd positions
    rng = random.Random(7)
    for i in range(40):                                                                     # over the cluster, with bases of their own
        reads.append(rd(2985 + i % 20, "60M" if i % 5 else "25M4D31M", f"cluster-{i}", rng=rng, flag=0x10 * (i & 1), quals=[(11 * i + 3 * k) % 40 for k in range(60)]))
    for i in range(30):                                                                     # over the window border at 1024
        reads.append(rd(1000 + i, "40M", f"border-{i}", rng=rng, mapq=60 if i % 6 else 5))
    for i in range(25):
        reads.append(rd(8970 + i, "50M", f"lonely-{i}", rng=rng, flag=0x400 if i % 8 == 7 else 0))
    # 700 reads over one pair: more than two strides of a workgroup; most of them A at 6000 and C at 6010 (a cell past
    # 255), one in nine another base or an N at the second site, one in fifty a deletion over the first
    for i in range(700):
        p = 5980 + i % 15
        seq = ["G"] * 50
        seq[6000 - p], seq[6010 - p] = "A", "AGTN"[i // 9 % 4] if i % 9 == 8 else "C"
        cigar = "50M" if i % 50 != 49 else f"{6000 - p}M2D{50 - (6000 - p)}M"
        reads.append(rd(p, cigar, f"deep-{i}", seq="".join(seq), flag=0x10 * (i & 1) | (0x400 if i % 70 == 69 else 0), mapq=60 if i % 40 else 10,
                        quals=[(13 * i + 7 * k) % 45 for k in range(50)]))
    return reads


PLANTED_SITES = sorted(set(s for _, _, sites, _, _, _ in PINS for s in sites) | set(CLUSTER) | set(DEEP) | {1030, LONELY, EMPTY, L - 1})


def random_reads(n, seed):
    """Reads with every CIGAR operation at random places: clips, insertions, deletions, skips and pads between matches of
    1..40 bases; a third of them over the dense cluster at 5000, some over the window border at 1024, some over the contig's
    end; some with fewer stored bases than the CIGAR consumes or none, some with fewer qualities than bases; N and IUPAC
    codes now and then."""
    rng = random.Random(seed)
    reads = []
    for i in range(n):
        ops, stored = [], 0
        if rng.random() < 0.2:
            ops.append(f"{rng.randint(1, 5)}H")
        if rng.random() < 0.3:
            l = rng.randint(1, 8); ops.append(f"{l}S"); stored += l
        for _ in range(rng.randint(1, 6)):
            l = rng.randint(1, 40)
            ops.append(f"{l}{rng.choice('MMMM=X')}"); stored += l
            k = rng.random()
            if k < 0.2:
                l = rng.randint(0, 6); ops.append(f"{l}I"); stored += l
            elif k < 0.5:
                ops.append(f"{rng.randint(0, 12)}D")
            elif k < 0.55:
                ops.append(f"{rng.randint(1, 60)}N")
            elif k < 0.6:
                ops.append(f"{rng.randint(1, 3)}P")
        if rng.random() < 0.1:
            ops.insert(0, f"{rng.randint(1, 4)}D")                                          # a leading D: no carrier
        if rng.random() < 0.3:
            l = rng.randint(1, 8); ops.append(f"{l}S"); stored += l
        seq = [rng.choice("AAAACCGT") for _ in range(stored)]
        for _ in range(rng.randint(0, 3)):
            seq[rng.randrange(stored)] = rng.choice("NNR=Y")
        k = rng.random()
        if k > 0.9:
            seq = seq[:0 if k > 0.95 else rng.randint(1, 30)]
        quals = [rng.choice((0, 10, 19, 20, 21, 35, 255)) for _ in range(rng.choice((0, 5, 200)))] if rng.random() < 0.8 else 30
        k = rng.random()
        pos = rng.randint(4985, 5040) if k < 0.6 else rng.randint(W - 80, W + 5) if k < 0.7 else rng.randint(L - 100, L + 20) if k < 0.75 else rng.randint(0, L - 1)
        reads.append(rd(pos, "".join(ops), f"rnd-{seed}-{i}", seq="".join(seq), flag=rng.choice((0, 0x10, 0x10, 0, 0, 0x400, 0x110, 0x4)),
                        mapq=rng.choice((60, 60, 60, 60, 20, 19, 0)), quals=quals))
    return reads


def random_sites(seed):
    rng = random.Random(1000 + seed)
    sites = set(range(5040, 5074, 2)) | {1023, 1024, 1030, L - 1, 0}                        # 17 sites in 33 positions: 15 partners and one more
    sites |= set(rng.sample(range(4950, 5200), 25)) | set(rng.sample(range(0, L), 40)) | set(rng.sample(range(W - 60, W + 60), 8))
    return sorted(sites)


class Case:
    """Reads as ContigRecords (coordinate sorted unless sort=False), their sites, their expansion by the reference, and
    the reference's results, each computed once."""

    def __init__(self, reads, sites, sort=True):
        self.reads = sorted(reads, key=lambda r: r[0]) if sort else list(reads)
        self.rec = ContigRecords.from_reads(self.reads)
        self.sites = np.array(sites, np.uint32)
        self.events = R.expand(self.rec)
        self._seen = {}

    def expected(self, max_dist, max_partners, min_quality, flt, sites=None):
        sites = self.sites if sites is None else np.array(sites, np.uint32)
        key = (max_dist, max_partners, min_quality, flt, sites.tobytes())
        if key not in self._seen:
            ex, bq = (None, None) if flt is None else (flt[0], MBQ if flt[1] else None)
            self._seen[key] = R.counts(self.events, self.rec, L, sites, max_dist, max_partners, min_quality, ex, bq)
        return self._seen[key]


@functools.lru_cache(maxsize=None)
def planted():
    return Case(planted_reads(), PLANTED_SITES)


# per seed: (max_dist, max_partners) -- the cluster's first site has 15 partners under each
RANDOM_SETS = {1: (1000, 15), 2: (40, 15), 3: (200, 15)}


@functools.lru_cache(maxsize=None)
def randomised(seed):
    return Case(random_reads(3000, seed), random_sites(seed))


def all_cases():
    return [("planted", planted(), (PIN_D, PIN_K))] + [(f"random-{s}", randomised(s), RANDOM_SETS[s]) for s in (1, 2, 3)]


def hollow(case, max_dist, max_partners):
    """Why the reference's own output says a random case tests too little; None when it does not."""
    seen = False
    for mq in QUALS:
        for flt in FILTERS:
            z = case.expected(max_dist, max_partners, mq, flt)
            t = z["tables"].astype(np.int64)
            if int(t.sum()) <= 5000:
                return f"the tables sum to {int(t.sum())} under {mq}, {flt}"
            if int(t.sum((1, 2)).max()) < 256:
                return f"no pair has both >= 256 under {mq}, {flt}"
            if not (t[:, R.DEL, :].any() and t[:, :, R.DEL].any() and (t[:, R.OTHER, :].any() or t[:, :, R.OTHER].any())):
                return f"a del row, a del column or an other cell is missing under {mq}, {flt}"
            seen = True
    if int(np.diff(case.expected(max_dist, max_partners, 20, None)["first"].astype(np.int64)).max()) != 15:
        return "no anchor has 15 partners"
    return None if seen else "nothing was looked at"


assert all(c in SEQ_CODES for c in "ACGTNRY=")
