"""The `fingerprint` subcommand (include/dut_fingerprint.h): a scaled k-mer MinHash sketch of every read,
hashed on the device.

    with Fingerprint(ksize=31, scaled=1000) as fp:
        fp.push([b"ACGT...", ...])             # or fp.push((seq4, offsets)): BAM's 4-bit codes
        r = fp.finish()                        # r.processed, r.hashes, r.counts, r.n_distinct, r.hexdigest

    fingerprint_file("reads.bam", output="fp.txt")

Bit for bit the reference's sketch (collectors/fingerprint/); 1 <= ksize <= 64.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib


class FingerprintError(RuntimeError):
    pass


@dataclass
class FingerprintResult:
    processed: int
    hashes: np.ndarray          # uint64, ascending, after the max_frequency filter
    counts: np.ndarray          # uint32
    n_distinct: int             # distinct hashes before the filter
    hexdigest: str


def _options(ksize, scaled, max_frequency):
    if not 1 <= int(ksize) <= 64:
        raise ValueError("ksize must be in 1..64")
    if int(scaled) < 0:
        raise ValueError("scaled must be >= 0")
    o = _lib.dut_fp_options()
    o.ksize = int(ksize)
    o.scaled = int(scaled)
    o.has_max_frequency = 0 if max_frequency is None else 1
    o.max_frequency = 0 if max_frequency is None else int(max_frequency)
    return o


def _pack_bytes(seqs):
    lens = np.fromiter((len(s) for s in seqs), dtype=np.uint64, count=len(seqs))
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    data = np.frombuffer(b"".join(bytes(s) for s in seqs) or b"\0", dtype=np.uint8)
    return data, off


class Fingerprint:
    """One device context; sequences are pushed in batches and merged into the device-resident table."""

    def __init__(self, ksize=31, scaled=1000, max_frequency: Optional[int] = None, device=0):
        self._lib = _lib.load()
        self._opt = _options(ksize, scaled, max_frequency)
        ctx = C.c_void_p()
        rc = self._lib.dut_fp_create(C.byref(self._opt), int(device), None, C.byref(ctx))
        if rc != 0:
            raise FingerprintError(f"dut_fp_create failed ({rc})")
        self._ctx = ctx

    def _check(self, rc, what):
        if rc != 0:
            raise FingerprintError(f"{what} failed ({rc}): {self._lib.dut_fp_last_error(self._ctx).decode()}")

    def push(self, batch):
        """batch: a list of byte strings (one per sequence), or (seq4, offsets) with seq4 the uint8 array of
        4-bit codes (two per byte, first base in the high nibble) and offsets the n + 1 base offsets."""
        if isinstance(batch, tuple):
            seq4, off = batch
            seq4 = np.ascontiguousarray(seq4, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            if seq4.size == 0:
                seq4 = np.zeros(1, np.uint8)
            n = off.size - 1
            if n > 0 and int(off[-1]) > 2 * seq4.size:
                raise ValueError("offsets beyond the seq4 buffer")
            self._check(self._lib.dut_fp_push_seq4(self._ctx, seq4.ctypes.data, off.ctypes.data, max(n, 0)), "push_seq4")
        else:
            seqs = list(batch)
            if not seqs:
                return
            data, off = _pack_bytes(seqs)
            self._check(self._lib.dut_fp_push_bytes(self._ctx, data.ctypes.data, off.ctypes.data, len(seqs)), "push_bytes")

    def finish(self) -> FingerprintResult:
        r = _lib.dut_fp_result()
        self._check(self._lib.dut_fp_finish(self._ctx, C.byref(r)), "finish")
        n = int(r.n_entries)
        h = np.ctypeslib.as_array(C.cast(r.hashes, C.POINTER(C.c_uint64)), (n,)).copy() if n else np.zeros(0, np.uint64)
        c = np.ctypeslib.as_array(C.cast(r.counts, C.POINTER(C.c_uint32)), (n,)).copy() if n else np.zeros(0, np.uint32)
        return FingerprintResult(int(r.processed), h, c, int(r.n_distinct), r.hexdigest.decode())

    def stats(self):
        """Device time of the pushes so far (ms, from events) and the windows / batches walked."""
        v = [C.c_double(), C.c_double(), C.c_double(), C.c_uint64(), C.c_uint64()]
        self._check(self._lib.dut_fp_stats(self._ctx, *[C.byref(x) for x in v]), "stats")
        return {"h2d_ms": v[0].value, "hash_ms": v[1].value, "reduce_ms": v[2].value,
                "n_windows": v[3].value, "n_batches": v[4].value}

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.dut_fp_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def fingerprint_file(path, ksize=31, scaled=1000, max_frequency=None, output=None, region="full", reference=None,
                     device=0):
    """The whole file (.bam, or FASTQ: .fastq / .fq / .gz) -> (processed, hexdigest); output: the hash file."""
    lib = _lib.load()
    opt = _options(ksize, scaled, max_frequency)
    if region not in ("full", "chrY", "chrM"):
        raise ValueError("region must be full, chrY or chrM")
    digest = C.create_string_buffer(65)
    processed = C.c_uint64()
    err = C.create_string_buffer(1024)
    rc = lib.dut_fp_files(str(path).encode(), reference.encode() if reference else None,
                          str(output).encode() if output else None, C.byref(opt), region.encode(), int(device),
                          digest, C.byref(processed), err, len(err))
    if rc != 0:
        raise FingerprintError(err.value.decode())
    return int(processed.value), digest.value.decode()


def kmer_hashes_host(seq: bytes, k: int):
    """The shared hash code on the host: (hashes uint64[len - k + 1], has_n bool[len - k + 1])."""
    lib = _lib.load()
    a = np.frombuffer(bytes(seq) or b"\0", dtype=np.uint8)
    n = max(len(seq) - k + 1, 0)
    out = np.zeros(max(n, 1), np.uint64)
    hn = np.zeros(max(n, 1), np.uint8)
    rc = lib.dut_fp_kmer_hashes_host(a.ctypes.data, len(seq), int(k), out.ctypes.data, hn.ctypes.data)
    if rc != 0:
        raise ValueError(f"dut_fp_kmer_hashes_host failed ({rc})")
    return out[:n], hn[:n].astype(bool)


def kmer_hashes_host_seq4(seq4, n_bases: int, k: int):
    """The same over n_bases BAM 4-bit codes (uint8 array, two per byte, first base in the high nibble)."""
    lib = _lib.load()
    a = np.ascontiguousarray(seq4, dtype=np.uint8)
    if 2 * a.size < n_bases:
        raise ValueError("seq4 shorter than n_bases")
    if a.size == 0:
        a = np.zeros(1, np.uint8)
    n = max(n_bases - k + 1, 0)
    out = np.zeros(max(n, 1), np.uint64)
    hn = np.zeros(max(n, 1), np.uint8)
    rc = lib.dut_fp_kmer_hashes_host_seq4(a.ctypes.data, int(n_bases), int(k), out.ctypes.data, hn.ctypes.data)
    if rc != 0:
        raise ValueError(f"dut_fp_kmer_hashes_host_seq4 failed ({rc})")
    return out[:n], hn[:n].astype(bool)


def max_hash(scaled: int) -> int:
    return int(_lib.load().dut_fp_max_hash(int(scaled)))


def sha256(data: bytes) -> bytes:
    out = C.create_string_buffer(32)
    buf = C.create_string_buffer(bytes(data), len(data) or 1)
    _lib.load().dut_fp_sha256(buf, len(data), out)
    return out.raw
