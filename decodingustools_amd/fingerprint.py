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


# ---- fingerprint-compare: similarity of many sketches (dut_fpc_* of include/dut_fingerprint.h) ----
@dataclass
class SketchFile:
    ksize: int
    scaled: int
    region: str
    max_frequency: Optional[int]
    hashes: np.ndarray          # uint64, strictly ascending
    counts: np.ndarray          # uint32, >= 1


_FIELDS = ("n_a", "n_b", "n_common", "sum_a", "sum_b", "sum_min")


def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(num.shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


@dataclass
class CompareResult:
    """One record per pair, in the order asked for: the exact integers; the ratios are nan where undefined."""
    n_a: np.ndarray
    n_b: np.ndarray
    n_common: np.ndarray
    sum_a: np.ndarray
    sum_b: np.ndarray
    sum_min: np.ndarray
    kernel_ms: float = 0.0
    n_tiles: int = 0
    bytes: int = 0

    @classmethod
    def from_records(cls, rec, **kw):
        rec = np.asarray(rec, np.uint64).reshape(-1, 6)
        return cls(*[rec[:, i].copy() for i in range(6)], **kw)

    def records(self):
        return np.stack([getattr(self, f) for f in _FIELDS], axis=1).astype(np.uint64)

    def jaccard(self):
        return _ratio(self.n_common, self.n_a + self.n_b - self.n_common)

    def containment(self):
        """(n_common / n_a, n_common / n_b)"""
        return _ratio(self.n_common, self.n_a), _ratio(self.n_common, self.n_b)

    def weighted_jaccard(self):
        return _ratio(self.sum_min, self.sum_a + self.sum_b - self.sum_min)


def tile_size() -> int:
    """Merged elements per tile of the compare kernel."""
    return int(_lib.load().dut_fpc_tile())


def read_fingerprint_file(path) -> SketchFile:
    """A file `fingerprint -o` (or the reference) wrote; FingerprintError with "<path>:<line>: ..." when malformed."""
    lib = _lib.load()
    s = _lib.dut_fpc_sketch()
    err = C.create_string_buffer(1024)
    if lib.dut_fp_file_read(str(path).encode(), C.byref(s), err, len(err)) != 0:
        raise FingerprintError(err.value.decode())
    try:
        n = int(s.n)
        h = np.ctypeslib.as_array(C.cast(s.hashes, C.POINTER(C.c_uint64)), (n,)).copy() if n else np.zeros(0, np.uint64)
        c = np.ctypeslib.as_array(C.cast(s.counts, C.POINTER(C.c_uint32)), (n,)).copy() if n else np.zeros(0, np.uint32)
        return SketchFile(int(s.ksize), int(s.scaled), s.region.decode(), int(s.max_frequency) if s.has_max_frequency else None, h, c)
    finally:
        lib.dut_fp_file_free(C.byref(s))


def _pair_arrays(pairs):
    p = np.asarray(list(pairs) if not isinstance(pairs, np.ndarray) else pairs, dtype=np.int64).reshape(-1, 2)
    if p.size and (p.min() < 0 or p.max() > 0xFFFFFFFF):
        raise ValueError("pair ids must be in 0 .. 2^32 - 1")
    return np.ascontiguousarray(p[:, 0], np.uint32), np.ascontiguousarray(p[:, 1], np.uint32)


class SketchSet:
    """Sketches resident on one device; compare(pairs) is one launch over all of them."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        ctx = C.c_void_p()
        rc = self._lib.dut_fpc_create(int(device), None, C.byref(ctx))
        if rc != 0:
            raise FingerprintError(f"dut_fpc_create failed ({rc})")
        self._ctx = ctx
        self._n = 0

    def __len__(self):
        return self._n

    def _check(self, rc, what):
        if rc != 0:
            raise FingerprintError(f"{what} failed ({rc}): {self._lib.dut_fpc_last_error(self._ctx).decode()}")

    def add(self, hashes, counts=None, ksize=31, scaled=1000) -> int:
        """hashes, counts: the sketch; or add(result, ksize=.., scaled=..) with a FingerprintResult or SketchFile
        (a SketchFile brings its own ksize and scaled).  Returns the id."""
        if isinstance(hashes, SketchFile):
            hashes, counts, ksize, scaled = hashes.hashes, hashes.counts, hashes.ksize, hashes.scaled
        elif isinstance(hashes, FingerprintResult):
            hashes, counts = hashes.hashes, hashes.counts
        h = np.ascontiguousarray(hashes, dtype=np.uint64)
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        if h.shape != c.shape or h.ndim != 1:
            raise ValueError("hashes and counts must be one-dimensional and of one length")
        sid = C.c_uint32()
        self._check(self._lib.dut_fpc_add(self._ctx, int(ksize), int(scaled), h.ctypes.data if h.size else None,
                                          c.ctypes.data if c.size else None, h.size, C.byref(sid)), "add")
        self._n += 1
        return int(sid.value)

    def _result(self, out, n):
        rec = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), (n, 6)).copy() if n else np.zeros((0, 6), np.uint64)
        v = [C.c_double(), C.c_uint64(), C.c_uint64()]
        self._check(self._lib.dut_fpc_stats(self._ctx, *[C.byref(x) for x in v]), "stats")
        return CompareResult.from_records(rec, kernel_ms=v[0].value, n_tiles=int(v[1].value), bytes=int(v[2].value))

    def compare(self, pairs) -> CompareResult:
        """pairs: (a, b) ids, any order, repeats and (i, i) allowed."""
        a, b = _pair_arrays(pairs)
        out = C.c_void_p()
        self._check(self._lib.dut_fpc_compare(self._ctx, a.ctypes.data if a.size else None, b.ctypes.data if b.size else None,
                                              a.size, C.byref(out)), "compare")
        return self._result(out, a.size)

    def compare_all(self) -> CompareResult:
        """The pairs i < j in row-major order."""
        out, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.dut_fpc_compare_all(self._ctx, C.byref(out), C.byref(n)), "compare_all")
        return self._result(out, int(n.value))

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.dut_fpc_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def compare_host(sketches, pairs) -> CompareResult:
    """The yardstick: sketches as (hashes, counts, ksize, scaled) tuples or SketchFile, by a two-pointer merge on
    DUT_THREADS host threads."""
    lib = _lib.load()
    keep, arr = [], (_lib.dut_fpc_sketch * max(len(sketches), 1))()
    for i, s in enumerate(sketches):
        if isinstance(s, SketchFile):
            s = (s.hashes, s.counts, s.ksize, s.scaled)
        h = np.ascontiguousarray(s[0], dtype=np.uint64)
        c = np.ascontiguousarray(s[1], dtype=np.uint32)
        if h.shape != c.shape or h.ndim != 1:
            raise ValueError("hashes and counts must be one-dimensional and of one length")
        keep.append((h, c))
        arr[i].ksize, arr[i].scaled, arr[i].n = int(s[2]), int(s[3]), h.size
        arr[i].hashes, arr[i].counts = (h.ctypes.data, c.ctypes.data) if h.size else (None, None)
    a, b = _pair_arrays(pairs)
    out = np.zeros((max(a.size, 1), 6), np.uint64)
    err = C.create_string_buffer(1024)
    rc = lib.dut_fpc_compare_host(arr, len(sketches), a.ctypes.data if a.size else None, b.ctypes.data if b.size else None,
                                  a.size, out.ctypes.data, err, len(err))
    if rc != 0:
        raise FingerprintError(f"compare_host failed ({rc}): {err.value.decode()}")
    return CompareResult.from_records(out[:a.size])


def compare_files(paths, out=None, matrix=None, query=None, min_jaccard=None, device=0):
    """`fingerprint-compare`: the files against each other (or `query` against each of them) on the device, the table
    to `out` (a temporary file when None) and the square Jaccard matrix to `matrix`.  Returns the table's text."""
    import os
    import tempfile
    lib = _lib.load()
    plist = [str(p).encode() for p in paths]
    arr = (C.c_char_p * max(len(plist), 1))(*plist)
    opt = _lib.dut_fpc_file_options(str(query).encode() if query is not None else None,
                                    0.0 if min_jaccard is None else float(min_jaccard), 0 if min_jaccard is None else 1)
    err = C.create_string_buffer(1024)
    tmp = None
    if out is None:
        fd, tmp = tempfile.mkstemp(suffix=".tsv")
        os.close(fd)
    try:
        rc = lib.dut_fingerprint_compare_files(arr, len(plist), C.byref(opt), str(out if out is not None else tmp).encode(),
                                               str(matrix).encode() if matrix is not None else None, int(device), err, len(err))
        if rc != 0:
            raise FingerprintError(err.value.decode())
        with open(out if out is not None else tmp) as f:
            return f.read()
    finally:
        if tmp:
            os.unlink(tmp)
