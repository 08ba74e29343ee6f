"""The long-read input that the error-profile, phase-sites and find-strs tests share (tests/test_ep_host.py,
tests/test_link_host.py and tests/test_str_host.py without a device, tests/test_gpu_long_reads.py on one): a contig of
270 000 positions -- 264 windows of the scan's read index, more than the 256 workgroups of k_site_error_profile -- with a
reference that holds N, IUPAC codes and lower case; reads past the base-count escape of a SiteRec (65 535 stored bases and
more), past its operation-count escape (255 operations and more) and past what BAM keeps outside CG (65 535 operations),
ONT-like reads of some 6 000 operations, one of them over a 50 000N, a stack of 300 reads of 3 000 bases, and reads at both
ends of the tile; the sites and loci the tests ask; and the reference results over them by tests/ep_ref.py,
tests/link_ref.py and tests/str_ref.py, each expansion computed once per process and left unchanged."""
import functools
import random
import re
import types

import numpy as np

import ep_ref
import link_ref
import str_ref
from decodingustools_amd.records import SEQ_CODES, ContigRecords

W = 1024                                    # the window of the scan's read index
LC = 270_000
N_WINDOWS = (LC + W - 1) // W
MBQ = 20                                    # the threshold the attachment is built with
MAX_BASES = 3_000_000                       # the references expand per base
ESCAPES = (65_534, 65_535, 65_536, 70_000)
FWD0, REV0, STEP = 3000, 100_000, 7000      # the single-M reads: forward from FWD0, reverse from REV0, STEP apart
TRUNCATED, BARE, FEW_QUALS = 20_000, 45_000, 50_000
GAPPED = (122_200, 123_200)                 # 69800M2I3D198M, forward and reverse: an insertion and a deletion past the escape
GAP_AT = 69_800
OPS0 = 195_000                              # the reads of 254, 255, 256 and 300 operations
MANY_OPS = 200_000                          # the read of 66 001 operations
N_PAIRS = 16_500                            # ... "1M1D" and "1M1I" that many times each, then 1M
STACK0, STACK_SITE = 250_000, 251_500
assert N_WINDOWS == 264 > 256


def make_ref(seed=17):
    rng = random.Random(seed)
    ref = [rng.choice("ACGT") for _ in range(LC)]
    for a, b in ((300, 330), (66_000, 66_100), (STACK_SITE - 40, STACK_SITE - 20)):
        for p in range(a, b):
            ref[p] = ref[p].lower()                                           # lower case counts as its letter
    for p in (400, 401, W - 1, W, 2500, FWD0 + 65_535, REV0 + 255, 66 * W, 67 * W - 1, MANY_OPS + 40, LC - 1):
        ref[p] = "N"
    for p, c in ((410, "R"), (411, "y"), (3 * W - 1, "M"), (2 * W, "n"), (FWD0 + 3 * STEP + 65_536, "K"), (LC - 700, "s")):
        ref[p] = c
    return np.frombuffer("".join(ref).encode(), np.uint8).copy()


REF = make_ref()
_UP = REF & 0xDF
FOLLOW = np.where(np.isin(_UP, np.frombuffer(b"ACGT", np.uint8)), _UP, ord("G")).astype(np.uint8)   # what a read says over a match
OTHER_BASE = {"A": "C", "C": "G", "G": "T", "T": "A"}                         # a mismatch to plant
ACGT = np.frombuffer(b"ACGT", np.uint8)


def rd(pos, cigar, name, flag=0, mapq=60, n_bases=None, n_quals=None, edits=(), low=()):
    """A read that follows the reference over its matches (G where the reference has no base, A beyond the contig), with the
    bases ACGT in turn by query index in insertions and clips; edits: (query index, base or 4-bit code letter, "*": another
    base) to plant.  n_bases: fewer stored bases than the CIGAR consumes, or none.  Quality values: 25..35 by query index,
    and at the indices of `low` 19 and 20 in turn, with the other of the two behind each; n_quals: fewer of them."""
    parts, x, y = [], pos, 0
    for l, op in ((int(t[:-1]), t[-1]) for t in re.findall(r"\d+[MIDNSHP=X]", cigar)):
        if op in "M=X":
            a, b = max(0, min(x, LC)), max(0, min(x + l, LC))
            parts += [np.full(a - x, ord("A"), np.uint8), FOLLOW[a:b], np.full(x + l - b, ord("A"), np.uint8)]
            x += l; y += l
        elif op in "IS":
            parts.append(ACGT[np.arange(y, y + l) & 3]); y += l
        elif op in "DN":
            x += l
    seq = bytearray(np.concatenate(parts).tobytes() if parts else b"")
    for q, c in edits:
        if 0 <= q < len(seq):
            seq[q] = ord(OTHER_BASE.get(chr(seq[q]), "T") if c == "*" else c)
    if n_bases is not None:
        del seq[n_bases:]
    quals = (25 + np.arange(len(seq)) % 11).astype(np.uint8)
    for k, q in enumerate(i for i in low if 0 <= i < len(seq)):
        quals[q] = 19 + (k & 1)
        if q + 1 < len(seq) and q + 1 not in low:
            quals[q + 1] = 20 - (k & 1)
    if n_quals is not None:
        quals = quals[:n_quals]
    return (pos, cigar, mapq, quals.tolist() if seq else None, flag, name, seq.decode())


def edges(n):
    """The query indices on both sides of every cycle-table edge at C = 256 and of the base-count escape, in a read of n."""
    return sorted(q for q in {0, 255, 256, n - 257, n - 256, n - 1, 65_534, 65_535, 65_536} if 0 <= q < n)


def alternating(n, m=3):
    """n operations M D M I ... that end in an M of m bases (a leading 2S where n is even)."""
    body = n - 1 + n % 2
    ops = [f"{m}M" if k % 2 == 0 else "1D" if k % 4 == 1 else "1I" for k in range(body)]
    return ("" if n % 2 else "2S") + "".join(ops)


def ont_cigar(seed, lead="", skip_at=None, plant=()):
    """(cigar, reference span, marks): 3 000 x (M 5..30, then I or D 1..3) and a last match.  plant: {operation pair: gap} puts
    that gap between two matches of 30; skip_at: a 50 000N behind that pair.  marks: gap -> the offset from the read's start
    of the position an insertion stands at or of the first deleted one; "skip" -> the skipped offsets [a, b)."""
    rng = random.Random(seed)
    plant, ops, x, marks, wide = dict(plant), [lead], 0, {}, False
    for i in range(3000):
        m = 30 if (i in plant or wide) else rng.randint(5, 30)
        wide = i in plant
        gap = f"{rng.randint(1, 3)}{rng.choice('ID')}"
        ops.append(f"{m}M"); x += m
        if i in plant:
            gap = plant[i]; marks[gap] = x
        ops.append(gap)
        if gap[-1] == "D":
            x += int(gap[:-1])
        if i == skip_at:
            ops.append("20M50000N"); marks["skip"] = (x + 20, x + 50_020); x += 50_020
    ops.append("25M")
    return "".join(ops), x + 25, marks


GAPS = {500: "7I", 1000: "12D", 1500: "70I", 2000: "80D"}                      # net +7, -12 and beyond +-63 (the `other` bin)
# name -> (start, flag, cigar, reference span, marks)
ONT = {}
for _i, (_name, _pos, _flag, _lead, _skip, _plant) in enumerate((
        ("ont-forward", 10_000, 0, "", None, GAPS), ("ont-reverse", 60_000, 0x10, "", None, GAPS),
        ("ont-leading-5000s", 120_000, 0, "5000S", None, ()), ("ont-leading-3h-5000s-reverse", 150_000, 0x10, "3H5000S", None, ()),
        ("ont-over-50000n-reverse", 90_000, 0x10, "", 1500, ()), ("ont-last", 205_000, 0, "", None, ()))):
    ONT[_name] = (_pos, _flag) + ont_cigar(40 + _i, _lead, _skip, _plant)
SKIP = tuple(ONT["ont-over-50000n-reverse"][0] + o for o in ONT["ont-over-50000n-reverse"][4]["skip"])
MANY_OPS_CIGAR = "1M1D" * N_PAIRS + "1M1I" * N_PAIRS + "1M"                    # 66 001 operations; sites and loci fall on deleted positions
MANY_OPS_SPAN = 3 * N_PAIRS + 1                                                # and behind insertions
STACK_CIGAR = "1000M2I500M3D1498M"


def stack_start(i):
    return STACK0 + (i * 3) % 400


def long_reads():
    reads = []
    for k, n in enumerate(ESCAPES):
        reads.append(rd(FWD0 + k * STEP, f"{n}M", f"m{n}-forward", edits=[(q, "*") for q in edges(n)], low=edges(n)))
        reads.append(rd(REV0 + k * STEP, f"{n}M", f"m{n}-reverse", flag=0x10, edits=[(q, "*") for q in edges(n)], low=edges(n)))
    reads += [
        # escape and truncation meet: L = 65 535 comes from the next record's offsets, the CIGAR says 70 000
        rd(TRUNCATED, "70000M", "m70000-with-65535-stored", flag=0x10, n_bases=65_535, edits=[(q, "*") for q in edges(65_535)], low=edges(65_535)),
        rd(BARE, "70000M", "m70000-no-stored-bases", n_bases=0),
        rd(FEW_QUALS, "70000M", "m70000-fewer-qualities-than-bases", n_quals=30_000, edits=[(29_999, "*"), (30_000, "*"), (69_999, "*")], low=[29_999]),
        # (beside the shapes of single-M reads: the carriers of an insertion and of a deletion at query index 69 799)
        rd(GAPPED[0], f"{GAP_AT}M2I3D198M", "m70000-gaps-past-the-escape", edits=[(GAP_AT - 1, "*"), (GAP_AT + 2, "*")], low=[GAP_AT - 1]),
        rd(GAPPED[1], f"{GAP_AT}M2I3D198M", "m70000-gaps-past-the-escape-reverse", flag=0x10, edits=[(GAP_AT, "*")], low=[GAP_AT - 2]),
        rd(OPS0, alternating(254), "ops-254"), rd(OPS0 + 100, alternating(255), "ops-255", flag=0x10),
        rd(OPS0 + 200, alternating(256), "ops-256"), rd(OPS0 + 300, alternating(300), "ops-300", flag=0x10, edits=[(0, "*"), (2, "*")]),
        rd(MANY_OPS, MANY_OPS_CIGAR, "ops-66001", edits=[(0, "*"), (N_PAIRS, "*"), (3 * N_PAIRS, "*")], low=[100, N_PAIRS + 1]),
        # the contig's end, the tile's last record (its escape reads the sentinel record) and its first
        rd(LC - 1000, "70000M", "m70000-over-the-contig-end", edits=[(0, "*"), (999, "*"), (1000, "*")], low=[999]),
        rd(LC - 500, "65535M", "m65535-the-highest-start", flag=0x10, edits=[(0, "*"), (499, "*")], low=[0, 499]),
        rd(0, "65535M", "m65535-the-lowest-start", edits=[(0, "*"), (65_534, "*")], low=[65_534]),
    ]
    for i, (name, (pos, flag, cigar, _, _)) in enumerate(ONT.items()):
        reads.append(rd(pos, cigar, name, flag=flag, edits=[(q, "*") for q in range(7 + i, 60_000, 997)], low=range(11, 60_000, 1499)))
    # 300 reads of 3 000 bases over one stretch: more than one stride of 256 threads, more than 16 waves; most say the
    # reference's base at STACK_SITE, one in five another, one in eleven an N ten positions on
    for i in range(300):
        p, plain = stack_start(i), i % 7 != 0
        edits = ([(STACK_SITE - p, "*")] if plain and i % 5 == 0 else []) + ([(STACK_SITE + 10 - p, "N")] if plain and i % 11 == 0 else []) + [(i, "*"), (2999 - i, "*")]
        flag = 0x10 * (i & 1) | {49: 0x400, 48: 0x100, 47: 0x200}.get(i % 50, 0)
        reads.append(rd(p, "3000M" if plain else STACK_CIGAR, f"stack-{i}", flag=flag, mapq={0: 19, 1: 20}.get(i % 40, 60), edits=edits, low=[i, 1500]))
    return reads


REDUCED = ([f"m{n}-{s}" for n in ESCAPES for s in ("forward", "reverse")] + ["ops-254", "ops-255", "ops-256", "ops-300", "ops-66001", "ont-forward", "ont-reverse"])


class Case:
    """Reads as ContigRecords (coordinate sorted unless sort=False), their three expansions by the references, and the
    references' results, each computed once."""

    def __init__(self, reads, sort=True):
        self.reads = sorted(reads, key=lambda r: r[0]) if sort else list(reads)
        self.rec = ContigRecords.from_reads(self.reads)
        assert int(self.rec.seq_off[-1]) <= MAX_BASES
        self.ref, self.ref_len = REF, LC
        self._seen = {}

    def index(self, name):
        return [r[5] for r in self.reads].index(name)

    @functools.cached_property
    def ep_events(self):
        return ep_ref.expand(self.rec)

    @functools.cached_property
    def link_events(self):
        return link_ref.expand(self.rec)

    @functools.cached_property
    def str_events(self):
        return str_ref.expand(self.rec)

    def _once(self, key, make):
        if key not in self._seen:
            self._seen[key] = make()
        return self._seen[key]

    def ep_expected(self, n_cycles, min_quality, flt, start=0, end=LC):
        ex, bq = (None, None) if flt is None else (flt[0], MBQ if flt[1] else None)
        return self._once(("ep", n_cycles, min_quality, flt, start, end),
                          lambda: ep_ref.profile(self.ep_events, self.rec, LC, REF, LC, start, end, n_cycles, min_quality, ex, bq))

    def link_expected(self, max_dist, max_partners, min_quality, flt, sites=None):
        sites = np.array(SITES if sites is None else sites, np.uint32)
        ex, bq = (None, None) if flt is None else (flt[0], MBQ if flt[1] else None)
        return self._once(("link", max_dist, max_partners, min_quality, flt, sites.tobytes()),
                          lambda: link_ref.counts(self.link_events, self.rec, LC, sites, max_dist, max_partners, min_quality, ex, bq))

    def str_expected(self, flank, min_quality, exclude_flags, loci=None):
        loci = LOCI if loci is None else loci
        cache = self._once(("str-reads",), dict)
        return self._once(("str", flank, min_quality, exclude_flags, tuple(loci)),
                          lambda: str_ref.measure(self.str_events, self.rec, LC, loci, flank, min_quality, exclude_flags, cache=cache))

    # the case as each of the three host tests' own programs want it
    @property
    def as_ep(self):
        return types.SimpleNamespace(rec=self.rec, events=self.ep_events, ref=REF, ref_len=LC)

    @property
    def as_link(self):
        return types.SimpleNamespace(rec=self.rec, events=self.link_events, sites=np.array(SITES, np.uint32))

    @property
    def as_str(self):
        return types.SimpleNamespace(rec=self.rec, events=self.str_events, loci=list(LOCI), expected=self.str_expected)


@functools.lru_cache(maxsize=None)
def whole():
    return Case(long_reads())


@functools.lru_cache(maxsize=None)
def reduced():
    """The tile the file tests write: the escape reads, the operation-count reads and two ONT-like reads, in the order they
    have in the whole tile.  Its expansions are those reads' records of the whole tile's expansions, renumbered."""
    big = whole()
    idx = np.array(sorted(big.index(n) for n in REDUCED))
    case = Case([big.reads[i] for i in idx], sort=False)
    new = np.full(big.rec.n, -1, np.int64)
    new[idx] = np.arange(len(idx))
    ev, out = big.ep_events, {}
    for k in ("base", "ins", "dele"):
        keep = new[ev[k][0]] >= 0
        out[k] = (new[ev[k][0][keep]],) + tuple(col[keep] for col in ev[k][1:])
    case.__dict__["ep_events"] = dict(out, lo=ev["lo"][idx], hi=ev["hi"][idx], L=ev["L"][idx])
    ev = big.link_events
    case.__dict__["link_events"] = dict(maps=[ev["maps"][i] for i in idx], lo=ev["lo"][idx], hi=ev["hi"][idx])
    case.__dict__["str_events"] = [big.str_events[i] for i in idx]
    return case


# ---- error-profile -----------------------------------------------------------------------------------------------------------
EP_CYCLES = (1, 256)
QUALS = (0, 20)
EP_FILTERS = (None, (0, False), (0x704, True))
# (n_cycles, min_quality, filter): every value of each of the three, not their product -- the reference counts two million
# records per call
EP_COMBOS = ((256, 20, (0x704, True)), (1, 0, None), (256, 0, (0, False)), (1, 20, (0x704, True)))
# the whole contig; mid-window to mid-window inside the long reads; one window deep inside them; two positions over a
# window border; the contig's last thousand
EP_RANGES = ((0, LC), (33_333, 99_999), (66 * W, 67 * W), (40 * W - 1, 40 * W + 1), (LC - 1000, LC))
EP_SPLIT = (30_000, 60 * W, 90_000)         # a split at a window border inside the forward read of 70 000 bases

# ---- phase-sites -------------------------------------------------------------------------------------------------------------
M70 = FWD0 + 3 * STEP                       # the forward read of 70 000 bases: [M70, M70 + 70 000)
ANCHOR_1 = M70 + 1000                       # ... fifteen partners spread over 60 000 positions inside it, no other site between
_ont4 = ONT["ont-over-50000n-reverse"]
ANCHOR_2 = _ont4[0] + 5000                  # inside the read over the 50 000N: partners in front of the skip, inside it and behind it
_before = [ANCHOR_2 + (SKIP[0] - 2000 - ANCHOR_2) * k // 5 for k in range(1, 6)]
_inside = [SKIP[0] + 10_000 * k for k in range(1, 5)]
_behind = [SKIP[1] + 1500 + 4000 * k for k in range(6)]
LINK_SETS = ((1, 1), (1000, 4), (70_000, 15), (2 ** 32 - 1, 15))
LINK_FILTERS = (None, (0x704, False), (0x704, True))
# per pair set the (min_quality, filter) it is asked under: every filter under every set of fifteen partners, both
# mapping qualities under every set -- not the product, the reference walks every read over every site per call
LINK_COMBOS = {(1, 1): ((0, None), (20, (0x704, True))), (1000, 4): ((20, None), (0, (0x704, False))),
               (70_000, 15): ((20, (0x704, False)), (0, (0x704, True))), (2 ** 32 - 1, 15): ((20, (0x704, False)), (20, (0x704, True)), (0, None))}


def make_sites():
    s = {ANCHOR_1} | {ANCHOR_1 + 4000 * k for k in range(1, 16)}
    s |= {ANCHOR_2} | set(_before) | set(_inside) | set(_behind)
    for k in (4, 10, 20, 196, 245):                                            # both sides of window borders inside long reads
        s |= {k * W - 1, k * W}
    s |= {MANY_OPS + 100, MANY_OPS + 101, MANY_OPS + 201, MANY_OPS + 300, MANY_OPS + 2 * N_PAIRS + 500, MANY_OPS + 2 * N_PAIRS + 7000}   # kept, deleted, behind insertions
    s |= {MANY_OPS + MANY_OPS_SPAN - 1, MANY_OPS + MANY_OPS_SPAN}              # a read's last reference position, and the one behind it
    s |= {M70 + 65_534, M70 + 65_535, M70 + 65_536, M70 + 69_999, M70 + 70_000}
    s |= {TRUNCATED + 65_534, TRUNCATED + 65_535, TRUNCATED + 66_000, TRUNCATED + 69_999}      # at and beyond the stored bases of the truncated read
    s |= {GAPPED[0] + GAP_AT - 1, GAPPED[0] + GAP_AT, GAPPED[0] + GAP_AT + 2, GAPPED[0] + GAP_AT + 3, GAPPED[1] + GAP_AT + 1}   # carrier, deleted, behind
    s |= {0, 1, FWD0 - 1, FWD0, LC - 1000, LC - 500, LC - 2, LC - 1}
    s |= {STACK_SITE, STACK_SITE + 10} | set(range(STACK0 + 500, STACK0 + 2500, 9))           # a cluster under the stack
    return sorted(s)


SITES = make_sites()
assert all(0 <= p < LC for p in SITES) and 250 <= len(SITES) <= 350
assert not [p for p in SITES if ANCHOR_1 < p < ANCHOR_1 + 60_000 and (p - ANCHOR_1) % 4000]
assert SITES[SITES.index(ANCHOR_2) + 1:SITES.index(ANCHOR_2) + 16] == _before + _inside + _behind and _behind[-1] < _ont4[0] + _ont4[3]

# ---- find-strs ---------------------------------------------------------------------------------------------------------------
STR_FLANKS = (1, 5, 64)
STR_FILTERS = (None, 0, 0x704, 0xFFFF)      # None: the unfiltered form, one strand
# (flank, min_quality, exclude_flags): every flank under every form at mapping quality 20, and 0 once per flank
STR_COMBOS = tuple((f, 20, ex) for f in STR_FLANKS for ex in STR_FILTERS) + ((1, 0, 0x704), (5, 0, None), (64, 0, 0))
R70 = REV0 + 3 * STEP                       # the reverse read of 70 000 bases


def make_loci():
    loci = []
    for at in (M70, R70):                                                      # at least 65 536 past a read's start: spans 1, 12, 300, 1024
        loci += [(at + 65_536, at + 65_537), (at + 65_600, at + 65_612), (at + 66_000, at + 66_300), (at + 67_000, at + 68_024)]
        loci += [(at + 69_900, at + 69_912), (at + 69_940, at + 69_952), (at + 69_990, at + 70_002)]       # at its last bases: partial by the flank, then by the span
    loci += [(88 * W - 6, 88 * W + 6), (88 * W, 88 * W + 12), (88 * W - 12, 88 * W), (89 * W - 1, 89 * W)]  # across, from and up to a window border
    for name in ("ont-forward", "ont-reverse"):
        pos, marks = ONT[name][0], ONT[name][4]
        loci += [(pos + marks["7I"] - 6, pos + marks["7I"] + 6), (pos + marks["12D"] - 4, pos + marks["12D"] + 16),
                 (pos + marks["70I"] - 6, pos + marks["70I"] + 6), (pos + marks["80D"] - 10, pos + marks["80D"] + 90),
                 (pos + marks["7I"], pos + marks["7I"] + 1), (pos + 20_000, pos + 20_300), (pos + 30_000, pos + 31_024)]
    loci += [(SKIP[0] - 6, SKIP[0] + 6), (SKIP[0] + 100, SKIP[0] + 400), (SKIP[1] - 5, SKIP[1] + 7), (SKIP[0] - 500, SKIP[0] - 200)]   # skipped, hence partial
    x = MANY_OPS + 2 * N_PAIRS                                                 # where "1M1I" begins
    loci += [(MANY_OPS + 100, MANY_OPS + 112), (MANY_OPS + 1000, MANY_OPS + 1300), (x - 10, x + 10), (x + 500, x + 512), (x + 1000, x + 2024)]
    loci += [(GAPPED[0] + GAP_AT - 6, GAPPED[0] + GAP_AT + 9), (GAPPED[1] + GAP_AT, GAPPED[1] + GAP_AT + 3)]   # +2 -3 past the escape
    loci += [(LC - 1024, LC), (LC - 1, LC), (0, 12)]
    loci += [(STACK0 + 990, STACK0 + 1410), (STACK0 + 1100, STACK0 + 1112), (STACK0 + 990, STACK0 + 2014), (STACK_SITE, STACK_SITE + 1)]   # under the stack
    return loci


LOCI = make_loci()
assert all(0 <= s < e <= LC and e - s <= 1024 for s, e in LOCI) and {e - s for s, e in LOCI} >= {1, 12, 300, 1024}


def read_lines(rec, bases=True):
    """The reads of a case file of the stand-alone walk programs (tests/native/*_walk_host.cpp), one line each: pos flag mapq,
    the number of operations and the CIGAR words; with bases: the number of bases and their 4-bit codes, the number of quality
    values and the values."""
    codes = np.empty(2 * rec.seq4.shape[0], np.uint8)
    codes[0::2], codes[1::2] = rec.seq4 >> 4, rec.seq4 & 15
    lines = []
    for i in range(rec.n):
        a, b = int(rec.cigar_off[i]), int(rec.cigar_off[i + 1])
        words = [int(rec.pos[i]), int(rec.flag[i]), int(rec.mapq[i]), b - a] + rec.cigar[a:b].tolist()
        if bases:
            s0, s1 = int(rec.seq_off[i]), int(rec.seq_off[i + 1])
            q0, q1 = int(rec.qual_off[i]), int(rec.qual_off[i + 1])
            words += [s1 - s0] + codes[s0:s1].tolist() + [q1 - q0] + rec.qual[q0:q1].tolist()
        lines.append(" ".join(map(str, words)))
    return lines


def check_shape(case, ends=True):
    """What the tile was built for, from its arrays alone (ends=False: the reduced tile, whose ends are other reads)."""
    rec = case.rec
    bases, ops = np.diff(rec.seq_off.astype(np.int64)), np.diff(rec.cigar_off.astype(np.int64))
    assert set(ESCAPES) <= set(bases.tolist()) and {254, 255, 256} <= set(ops.tolist()) and int(ops.max()) > 65_535
    assert not ends or (bases[0] >= 65_535 and bases[-1] >= 65_535)            # the first and the last record are escape reads
    assert int(rec.seq_off[-1]) <= MAX_BASES
    # a read whose reference span (the lengths of its M D N = X operations) covers 64 windows of the index and more
    consumes = np.isin(rec.cigar & 15, (0, 2, 3, 7, 8)) * (rec.cigar >> 4).astype(np.int64)
    span = np.add.reduceat(consumes, rec.cigar_off[:-1].astype(np.int64))
    first, last = rec.pos.astype(np.int64) // W, (rec.pos.astype(np.int64) + span - 1) // W
    assert int((last - first + 1).max()) >= 64
    return bases, ops


assert all(c in SEQ_CODES for c in "ACGTNRY=")
