"""A numpy restatement of the reference's `fingerprint` (collectors/fingerprint/processor.rs:117-140,
utils.rs:11-85), vectorised over windows so that tens of millions of k-mers take seconds.

SeaHash (seahash 4.1, one-shot write): lanes a, b, c, d from fixed seeds, the input read as little-endian
8-byte words (the last one zero padded), word i into lane i % 4 as diffuse(lane ^ w), result
diffuse(a ^ b ^ c ^ d ^ len).  numpy's uint64 multiplication wraps, which is the arithmetic mod 2^64 it needs.
"""
import hashlib

import numpy as np

SEEDS = (0x16f11fe89b0d677c, 0xb480a793d8e6c86c, 0x6fe2e5aaf078ebc9, 0x14f994a4c5259381)
MUL = np.uint64(0x6eed0e9da4d94a4f)
SEQ4_ALPHABET = b"=ACMGRSVTWYHKDBN"

_COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in (("A", "T"), ("T", "A"), ("C", "G"), ("G", "C")):
    _COMP[ord(_a)] = ord(_b)


def _diffuse(x):
    with np.errstate(over="ignore"):
        x = x * MUL
        x = x ^ ((x >> np.uint64(32)) >> (x >> np.uint64(60)))
        return x * MUL


def seahash_rows(rows):
    """rows: (n, L) uint8, every row hashed as L bytes -> (n,) uint64."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, L = rows.shape
    nw = (L + 7) // 8
    pad = np.zeros((n, nw * 8), dtype=np.uint8)
    pad[:, :L] = rows
    words = pad.view("<u8")
    lanes = [np.full(n, s, dtype=np.uint64) for s in SEEDS]
    for i in range(nw):
        lanes[i % 4] = _diffuse(lanes[i % 4] ^ words[:, i])
    return _diffuse(lanes[0] ^ lanes[1] ^ lanes[2] ^ lanes[3] ^ np.uint64(L))


def seahash(data: bytes) -> int:
    return int(seahash_rows(np.frombuffer(bytes(data), dtype=np.uint8)[None, :])[0])


def max_hash(scaled: int) -> int:
    """((u64::MAX as f64) / scaled as f64) as u64 with Rust's saturating cast."""
    two64 = 18446744073709551616.0
    d = two64 / float(scaled) if scaled else float("inf")
    return 2 ** 64 - 1 if d >= two64 else int(d)


def canonical_rows(win):
    """win: (n, k) uint8 -> the canonical bytes of every window (byte order min of window and reverse complement)."""
    rc = _COMP[win[:, ::-1]]
    diff = win != rc
    first = np.argmax(diff, axis=1)
    r = np.arange(win.shape[0])
    use_rc = diff[r, first] & (rc[r, first] < win[r, first])
    return np.where(use_rc[:, None], rc, win)


def _windows(data, off, k):
    """Starts of all windows that lie inside one sequence."""
    off = np.asarray(off, dtype=np.int64)
    lens = np.diff(off)
    nwin = np.maximum(lens - k + 1, 0)
    total = int(nwin.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    seq_of = np.repeat(np.arange(len(lens)), nwin)
    first = np.zeros(len(lens), np.int64)
    np.cumsum(nwin[:-1], out=first[1:])
    return off[:-1][seq_of] + (np.arange(total) - first[seq_of])


def window_hashes(data, off, k, chunk=1 << 21):
    """(hashes, has_n) of every window, sequences in order."""
    data = np.asarray(data, dtype=np.uint8)
    starts = _windows(data, off, k)
    isn = np.zeros(len(data) + 1, np.int64)
    np.cumsum(data == ord("N"), out=isn[1:])
    hashes = np.zeros(len(starts), np.uint64)
    has_n = (isn[starts + k] - isn[starts]) > 0
    cols = np.arange(k)
    for c0 in range(0, len(starts), chunk):
        s = starts[c0:c0 + chunk]
        keep = ~has_n[c0:c0 + chunk]
        if not keep.any():
            continue
        win = data[s[keep][:, None] + cols[None, :]]
        h = hashes[c0:c0 + chunk]
        h[keep] = seahash_rows(canonical_rows(win))
    return hashes, has_n


def kmer_hashes(seq: bytes, k: int):
    a = np.frombuffer(bytes(seq), dtype=np.uint8)
    return window_hashes(a, [0, len(a)], k)


def decode_seq4(seq4, off):
    """BAM 4-bit codes (two per byte, high nibble first) -> bytes, same offsets."""
    seq4 = np.asarray(seq4, dtype=np.uint8)
    total = int(off[-1]) if len(off) else 0
    nib = np.empty(2 * len(seq4), np.uint8)
    nib[0::2] = seq4 >> 4
    nib[1::2] = seq4 & 15
    return np.frombuffer(SEQ4_ALPHABET, np.uint8)[nib[:total]]


def encode_seq4(data):
    """bytes over =ACMGRSVTWYHKDBN -> 4-bit codes."""
    lut = np.zeros(256, np.uint8)
    for i, c in enumerate(SEQ4_ALPHABET):
        lut[c] = i
    codes = lut[np.asarray(data, dtype=np.uint8)]
    if len(codes) % 2:
        codes = np.concatenate([codes, np.zeros(1, np.uint8)])
    return ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8)


def pack(seqs):
    """list of byte strings -> (data uint8, offsets uint64)."""
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    data = np.frombuffer(b"".join(bytes(s) for s in seqs), dtype=np.uint8)
    return data, off


def sketch(data, off, k, scaled, max_frequency=None):
    """The sketch of sequences data[off[i]:off[i+1]]: dict(processed, hashes, counts, n_distinct, hexdigest)."""
    off = np.asarray(off, dtype=np.int64)
    lens = np.diff(off)
    processed = int(np.count_nonzero(lens >= k))
    h, has_n = window_hashes(data, off, k)
    mh = np.uint64(max_hash(scaled))
    kept = h[(~has_n) & (h <= mh)]
    hashes, counts = np.unique(kept, return_counts=True)
    counts = counts.astype(np.uint32)
    n_distinct = len(hashes)
    if max_frequency is not None:
        sel = counts <= max_frequency
        hashes, counts = hashes[sel], counts[sel]
    return {"processed": processed, "hashes": hashes.astype(np.uint64), "counts": counts,
            "n_distinct": n_distinct, "hexdigest": digest(hashes, counts)}


def sketch_seqs(seqs, k, scaled, max_frequency=None):
    data, off = pack(seqs)
    return sketch(data, off, k, scaled, max_frequency)


def digest(hashes, counts):
    rec = np.zeros(len(hashes), dtype=[("h", "<u8"), ("c", "<u4")])
    rec["h"] = hashes
    rec["c"] = counts
    return hashlib.sha256(rec.tobytes()).hexdigest()


def file_text(k, scaled, region, max_frequency, hashes, counts):
    s = f"#ksize={k}\n#scaled={scaled}\n#region={region}\n"
    if max_frequency is not None:
        s += f"#max_frequency={max_frequency}\n"
    return s + "".join(f"{int(h)}\t{int(c)}\n" for h, c in zip(hashes, counts))


def stdout_text(processed, hexdigest):
    return f"Processed {processed} sequences\n{hexdigest}\n"
