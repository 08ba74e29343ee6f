"""The inputs the `fingerprint` edge tests share (tests/test_fingerprint_host.py without a device,
tests/test_gpu_fingerprint_edges.py on one): sequences whose window counts sit on the kernel's strip of 64 window starts,
a special byte at every place around a strip seam, one read long enough to cross waves and workgroups, a tandem repeat whose
counts add up over batches, a list of reads that the batch split cuts at odd bases -- and the split rule of `push` restated,
so that a test can say which batches its input makes.  Seeded; the same lists on every call."""
import functools

import numpy as np

import fp_ref

KS = (1, 2, 15, 16, 17, 21, 31, 32, 33, 51, 63, 64)
STRIP = 64                                  # window starts per thread of k_fp_hash
ACGT = np.frombuffer(b"ACGT", np.uint8)
SPECIAL = (b"N", b"R", b"n", b"=")         # 'n' is no N and no BAM letter: bytes only, and the byte path
LONG = 33_000                               # 516 strips at k = 1: two workgroup seams (256 strips), eight wave seams
BIG, N_RUN = 5001, 301                      # batch_mix's read that is a batch alone, and its read of N


def _acgt(rng, n):
    return bytes(ACGT[rng.integers(0, 4, size=n)])


@functools.lru_cache(maxsize=None)
def edge_lengths(k):
    """Window counts 0, 1, 2, 63 .. 66 and 127 .. 130: every sequence of random content of its own, so that a window
    read across a sequence's end is one hash too many."""
    rng = np.random.default_rng(1000 + k)
    return tuple(_acgt(rng, k + d) for d in (-1, 0, 1, 62, 63, 64, 65, 126, 127, 128, 129))


def seam_places(k):
    L = 5 * STRIP + k - 1
    p = (0, k - 1, 62, 63, 64, 65, 63 + k - 1, 64 + k - 2, 64 + k - 1, 64 + k, 127, 128, 128 + k - 1, L - k, L - 1)
    return tuple(sorted(set(p)))


@functools.lru_cache(maxsize=None)
def seam_bytes(k, seq4=False):
    """Five full strips each, one special byte at a place before, at or behind a strip seam; then two sequences with a run
    of N that leaves the second strip no live window, and the run wider by one base on each side."""
    rng = np.random.default_rng(2000 + k)
    L = 5 * STRIP + k - 1
    out = []
    for p in seam_places(k):
        for b in SPECIAL:
            s = bytearray(_acgt(rng, L))                    # (drawn for 'n' too: both forms get the same sequences)
            s[p] = b[0]
            if not (seq4 and b == b"n"):
                out.append(bytes(s))
    for lo, hi in ((STRIP, 2 * STRIP + k - 1), (STRIP - 1, 2 * STRIP + k)):
        s = bytearray(_acgt(rng, L))
        s[lo:hi] = b"N" * (hi - lo)
        out.append(bytes(s))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def long_read(seed):
    rng = np.random.default_rng(seed)
    s = ACGT[rng.integers(0, 4, size=LONG)].copy()
    u = rng.random(LONG)
    s[u < 0.001] = ord("N")
    s[(u >= 0.001) & (u < 0.002)] = ord("R")
    return bytes(s)


@functools.lru_cache(maxsize=None)
def tandem(k=31, unit=997, copies=33):
    """`copies` reads of unit + k - 1 bases out of the repeat, each with the unit's `unit` windows, and one read that is
    the first half of the unit: its windows are counted once more."""
    rng = np.random.default_rng(3000 + unit)
    u = _acgt(rng, unit)
    return tuple([(u + u)[:unit + k - 1]] * copies + [u[:unit // 2]])


@functools.lru_cache(maxsize=None)
def batch_mix(seed):
    """300 reads of 0 .. 199 random bases; 40 of the first 140 repeated among the later ones (a later batch brings hashes
    the table holds); near the end a read of 301 N, then one of 5 001 bases, then eight of 3 bases.  The long read is a
    batch alone at any cap below its length, so the short reads behind it are the last batch, without a sequence of k
    bases for k > 3, and the N read closes the batch it is in.  Whether the N read also opens that batch (a batch without
    a survivor) is up to the seed and the cap: the test that needs it asserts it, by `batches` below."""
    rng = np.random.default_rng(seed)
    reads = [_acgt(rng, int(rng.integers(0, 200))) for _ in range(300)]
    src = rng.choice(140, size=40, replace=False)
    dst = rng.choice(np.arange(150, 290), size=40, replace=False)
    for a, b in zip(src, dst):
        reads[int(b)] = reads[int(a)]
    reads[290] = b"N" * N_RUN
    reads[291] = _acgt(rng, BIG)
    for i in range(292, 300):
        reads[i] = _acgt(rng, 3)
    return tuple(reads)


def batch_mix_n_first(seed):
    """batch_mix turned so that it begins at the read of N: that read, with the 5 001-base read behind it, is the first
    batch whatever the cap -- no survivor, an empty table -- and the long read the second."""
    reads = batch_mix(seed)
    return reads[290:] + reads[:290]


def split(lens, cap):
    """`push`'s rule: a batch takes sequences while their sum stays <= cap, and at least one.  -> [(i0, i1)]"""
    out, i = [], 0
    while i < len(lens):
        j = i + 1
        while j < len(lens) and sum(lens[i:j + 1]) <= cap:
            j += 1
        out.append((i, j))
        i = j
    return out


def batches(seqs, cap, k):
    """Per batch of `seqs` at `cap`: its range of sequences, its first base offset, whether it has a sequence of >= k
    bases (without one it never reaches the kernel), whether it has a window without 'N' (without one it has no
    survivor), and its windows' hashes at scaled = 1 by the reference."""
    lens = [len(s) for s in seqs]
    first = np.concatenate([[0], np.cumsum(lens)])
    out = []
    for i0, i1 in split(lens, cap):
        data, off = fp_ref.pack(seqs[i0:i1])
        h, has_n = fp_ref.window_hashes(data, off, k)
        out.append({"i0": i0, "i1": i1, "first_base": int(first[i0]), "has_k": any(n >= k for n in lens[i0:i1]),
                    "has_clean_window": bool((~has_n).any()), "hashes": np.unique(h[~has_n])})
    return out


def seq4_of(seqs):
    """(seq4, offsets) of byte strings over BAM's 16 letters."""
    data, off = fp_ref.pack(seqs)
    assert all(c in fp_ref.SEQ4_ALPHABET for c in bytes(data))
    return fp_ref.encode_seq4(data), off


BIG_LINE = 1_100_000                        # beyond the FASTQ reader's refill of 1 MiB, and some 26 BGZF blocks as a record


@functools.lru_cache(maxsize=None)
def file_reads():
    """The long-read file of the reader tests: a read of one base, the 1.1 Mbase read, another of one base (so the long
    record is decoded from an odd and from an even base, and followed at both), long_read, and 50 short reads."""
    rng = np.random.default_rng(77)
    big = ACGT[rng.integers(0, 4, size=BIG_LINE)].copy()
    big[rng.random(BIG_LINE) < 0.0005] = ord("N")
    short = [_acgt(rng, int(rng.integers(1, 152))) for _ in range(50)]
    return tuple([b"A", bytes(big), b"C", long_read(5)] + short)
