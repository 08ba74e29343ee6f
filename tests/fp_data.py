"""Inputs for the `fingerprint` tests: seeded reads, and the same reads written as BAM and as FASTQ."""
import gzip

import numpy as np

from bamio import write_bam
from decodingustools_amd.records import ContigRecords

import fp_ref

BAM_LETTERS = fp_ref.SEQ4_ALPHABET.decode()


def random_reads(n, rng, lo=1, hi=180, alphabet="ACGT", p=None, n_rate=0.0):
    """n reads of random lengths in [lo, hi] over alphabet (weights p), with 'N' at n_rate."""
    letters = np.frombuffer(alphabet.encode(), np.uint8)
    out = []
    for _ in range(n):
        L = int(rng.integers(lo, hi + 1))
        s = rng.choice(letters, size=L, p=None if p is None else np.asarray(p) / np.sum(p))
        if n_rate:
            s[rng.random(L) < n_rate] = ord("N")
        out.append(bytes(s))
    return out


def synthetic_reads(n, read_len, seed, n_rate=0.001):
    """n reads of read_len ACGT bases with sparse N, as one (data, offsets) pair (the large cases)."""
    rng = np.random.default_rng(seed)
    data = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n * read_len)]
    data[rng.random(data.size) < n_rate] = ord("N")
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(read_len)
    return data, off


def write_reads_bam(path, seqs, block_every=None, unmapped_tail=()):
    """seqs (strings over =ACMGRSVTWYHKDBN, at least one base each) as mapped records of one contig, in order."""
    reads = [(10 * i, f"{len(s)}M", 60, 30, 16 if i % 3 == 0 else 0, f"q{i}", s) for i, s in enumerate(seqs)]
    rec = ContigRecords.from_reads(reads)
    L = 10 * len(seqs) + 1000
    write_bam(str(path), [("chr1", L)], {0: rec}, write_index=False, block_every=block_every,
              unmapped_tail=unmapped_tail)


def write_fastq(path, seqs, gz=False, members=1, crlf=False):
    """seqs as 4-line records; gz: gzip, split into `members` concatenated members."""
    nl = b"\r\n" if crlf else b"\n"
    recs = [b"@r%d extra words" % i + nl + s + nl + b"+" + nl + b"I" * len(s) + nl for i, s in enumerate(seqs)]
    if not gz:
        with open(path, "wb") as f:
            f.write(b"".join(recs))
        return
    with open(path, "wb") as f:
        step = max(1, (len(recs) + members - 1) // members)
        for i in range(0, len(recs), step):
            f.write(gzip.compress(b"".join(recs[i:i + step])))
