"""`fingerprint` without a device: the numpy restatement against the known answers, the library's shared hash code,
max_hash and SHA-256 against it, the BAM and FASTQ readers, and the command line's argument and format errors."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import fp_data
import fp_ref
from decodingustools_amd import _lib, build as _b
from decodingustools_amd import fingerprint as fpm

# golden/fingerprint_kat.json: seahash 4.1's documented example (hash(b"to be or not to be")), four hand-worked
# windows of the canonical-byte rule (an IUPAC code and lower case included), the sketch and digest of ACGT at k = 3,
# the digest of an empty sketch, and max_hash for several `scaled` values (Rust's saturating float-to-integer cast)
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "fingerprint_kat.json")))


@pytest.fixture(scope="module")
def lib():
    _b.build()
    return _lib.load()


def test_fp_ref_known_answers():
    for c in GOLD["seahash"]:
        assert fp_ref.seahash(c["input"].encode()) == c["hash"]
    for c in GOLD["windows"]:
        w = np.frombuffer(c["input"].encode(), np.uint8)[None, :]
        assert bytes(fp_ref.canonical_rows(w)[0]) == c["canonical"].encode()
        h, hn = fp_ref.kmer_hashes(c["input"].encode(), c["k"])
        assert not hn[0] and int(h[0]) == c["hash"]
    for c in GOLD["sketch"]:
        r = fp_ref.sketch_seqs([s.encode() for s in c["sequences"]], c["k"], c["scaled"])
        assert [[int(h), int(n)] for h, n in zip(r["hashes"], r["counts"])] == c["entries"]
        assert r["hexdigest"] == c["hexdigest"]
    assert fp_ref.digest([], []) == GOLD["empty_digest"]
    for s, v in GOLD["max_hash"].items():
        assert fp_ref.max_hash(int(s)) == v


def test_host_entry_points_known_answers(lib):
    for c in GOLD["windows"]:
        h, hn = fpm.kmer_hashes_host(c["input"].encode(), c["k"])
        assert not hn[0] and int(h[0]) == c["hash"]
    for s, v in GOLD["max_hash"].items():
        assert fpm.max_hash(int(s)) == v
    for s in (5, 7, 10, 999, 1001, 12345, 2 ** 40 + 3, 2 ** 63, 2 ** 64 - 1):
        assert fpm.max_hash(s) == fp_ref.max_hash(s), s


def test_sha256(lib):
    rng = np.random.default_rng(5)
    for n in (0, 1, 55, 56, 63, 64, 65, 119, 120, 1000, 12 * 1001):
        d = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        assert fpm.sha256(d) == hashlib.sha256(d).digest(), n


def test_shared_hash_code_all_k(lib):
    rng = np.random.default_rng(11)
    # BAM's 16 letters, and every byte value with lower case and IUPAC letters weighted up
    bam = fp_data.random_reads(1, rng, 400, 400, fp_data.BAM_LETTERS)[0]
    weights = np.ones(256)
    for ch in b"ACGTNacgtnRYSWKMBDHV=":
        weights[ch] = 40.0
    weights[ord("A")] = weights[ord("C")] = weights[ord("G")] = weights[ord("T")] = 400.0
    anyb = bytes(rng.choice(256, size=400, p=weights / weights.sum()).astype(np.uint8))
    acgt = fp_data.random_reads(1, rng, 300, 300, "ACGT")[0]
    for k in range(1, 65):
        for s in (bam, anyb, acgt):
            h, hn = fpm.kmer_hashes_host(s, k)
            rh, rhn = fp_ref.kmer_hashes(s, k)
            assert np.array_equal(hn, rhn), k
            assert np.array_equal(h[~hn], rh[~rhn]), k
    # every byte value inside an otherwise ACGT window, at several places
    for k in (1, 5, 31, 33, 64):
        for b in range(256):
            s = bytearray(acgt[:k + 8])
            s[3 % len(s)] = b
            s[(k + 2) % len(s)] = b
            h, hn = fpm.kmer_hashes_host(bytes(s), k)
            rh, rhn = fp_ref.kmer_hashes(bytes(s), k)
            assert np.array_equal(hn, rhn) and np.array_equal(h[~hn], rh[~rhn]), (k, b)


def test_shared_hash_code_seq4_all_k(lib):
    rng = np.random.default_rng(12)
    s = fp_data.random_reads(1, rng, 301, 301, fp_data.BAM_LETTERS)[0]
    s4 = fp_ref.encode_seq4(np.frombuffer(s, np.uint8))
    for k in range(1, 65):
        h, hn = fpm.kmer_hashes_host_seq4(s4, len(s), k)
        rh, rhn = fp_ref.kmer_hashes(s, k)
        assert np.array_equal(hn, rhn) and np.array_equal(h[~hn], rh[~rhn]), k
    # every one of the 16 codes alone
    for c in fp_data.BAM_LETTERS.encode():
        h, hn = fpm.kmer_hashes_host_seq4(fp_ref.encode_seq4(np.array([c], np.uint8)), 1, 1)
        rh, rhn = fp_ref.kmer_hashes(bytes([c]), 1)
        assert hn[0] == rhn[0] and (hn[0] or h[0] == rh[0]), chr(c)


def test_host_entry_point_rejects_k(lib):
    out = np.zeros(4, np.uint64)
    hn = np.zeros(4, np.uint8)
    a = np.frombuffer(b"ACGTACGT", np.uint8)
    assert lib.dut_fp_kmer_hashes_host(a.ctypes.data, 8, 0, out.ctypes.data, hn.ctypes.data) < 0
    assert lib.dut_fp_kmer_hashes_host(a.ctypes.data, 8, 65, out.ctypes.data, hn.ctypes.data) < 0


def _bam_walk(lib, path, max_bases):
    err = C.create_string_buffer(512)
    b = lib.dut_bam_open(str(path).encode(), err, 512)
    assert b, err.value
    seqs, batches = [], 0
    try:
        while True:
            n, off, s4 = C.c_uint64(), C.c_void_p(), C.c_void_p()
            assert lib.dut_bam_next_seqs(b, max_bases, C.byref(n), C.byref(off), C.byref(s4)) == 0, lib.dut_bam_error(b)
            if n.value == 0:
                break
            batches += 1
            o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (n.value + 1,)).copy()
            nbytes = (int(o[-1]) + 1) // 2
            d = np.ctypeslib.as_array(C.cast(s4, C.POINTER(C.c_uint8)), (max(nbytes, 1),))[:nbytes].copy()
            assert int(o[0]) == 0 and np.all(np.diff(o.astype(np.int64)) >= 0)
            if n.value > 1:
                assert int(o[-1]) <= max_bases
            txt = fp_ref.decode_seq4(d, o)
            seqs += [bytes(txt[int(o[i]):int(o[i + 1])]) for i in range(n.value)]
    finally:
        lib.dut_bam_close(b)
    return seqs, batches


def test_bam_whole_file_walk(lib, tmp_path):
    rng = np.random.default_rng(3)
    seqs = [s.decode() for s in fp_data.random_reads(300, rng, 1, 151, fp_data.BAM_LETTERS)]
    tail = [(b"u%d" % i, 4, l, 0) for i, l in enumerate((0, 7, 0, 1, 33, 0))]
    path = tmp_path / "w.bam"
    fp_data.write_reads_bam(path, seqs, block_every=7, unmapped_tail=tail)
    want = [s.encode() for s in seqs] + [b"=" * l for _, _, l, _ in tail]
    for cap in (1, 100, 1000, 1 << 30):
        got, batches = _bam_walk(lib, path, cap)
        assert got == want, cap
        if cap == 1:
            assert batches >= sum(1 for s in want if s)          # (an empty record may join the batch before it)


def _fastq_walk(lib, path, max_bases=1 << 30):
    err = C.create_string_buffer(512)
    f = lib.dut_fastq_open(str(path).encode(), err, 512)
    assert f, err.value
    seqs = []
    try:
        while True:
            n, off, d = C.c_uint64(), C.c_void_p(), C.c_void_p()
            assert lib.dut_fastq_next(f, max_bases, C.byref(n), C.byref(off), C.byref(d)) == 0
            if n.value == 0:
                break
            o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (n.value + 1,)).copy()
            data = C.string_at(d, int(o[-1]))
            seqs += [data[int(o[i]):int(o[i + 1])] for i in range(n.value)]
    finally:
        lib.dut_fastq_close(f)
    return seqs


def test_fastq_reader(lib, tmp_path):
    rng = np.random.default_rng(8)
    seqs = fp_data.random_reads(200, rng, 1, 160, "ACGTN")
    for name, kw in (("a.fq", {}), ("b.fastq", {"crlf": True}), ("c.fq.gz", {"gz": True}),
                     ("d.fq.gz", {"gz": True, "members": 7, "crlf": True})):
        p = tmp_path / name
        fp_data.write_fastq(p, seqs, **kw)
        assert _fastq_walk(lib, p) == seqs, name
        assert _fastq_walk(lib, p, 50) == seqs, name
    # a plain file named .gz reads as it is
    p = tmp_path / "plain.gz"
    fp_data.write_fastq(p, seqs[:5])
    assert _fastq_walk(lib, p) == seqs[:5]


def test_fastq_stops_at_empty_id(lib, tmp_path, capfd):
    p = tmp_path / "e.fq"
    p.write_bytes(b"@a\nACGT\n+\nIIII\n@b x\nGGGA \n+\nIIII\n@ desc\nTTTT\n+\nIIII\n@c\nCCCC\n+\nIIII\n")
    assert _fastq_walk(lib, p) == [b"ACGT", b"GGGA"]
    assert "empty id" in capfd.readouterr().err


def _cli(*args, cwd=None):
    return subprocess.run([_b.CLI, "fingerprint"] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd)


def test_cli_errors_without_device(lib, tmp_path):
    r = _cli(tmp_path / "x.txt")
    assert r.returncode == 1
    assert r.stderr.strip() == "Error: Unsupported file format. Must be .fastq, .fq, .fastq.gz, .fq.gz, .bam, or .cram"
    assert r.stdout == ""
    r = _cli(tmp_path / "x.cram")
    assert r.returncode == 1 and "CRAM is not supported" in r.stderr
    r = _cli(tmp_path / "x.gam")
    assert r.returncode == 1 and "GAM input is not supported" in r.stderr
    for k in ("0", "65", "x"):
        r = _cli(tmp_path / "x.fq", "--ksize", k)
        assert r.returncode == 2, k
    r = _cli(tmp_path / "missing.fq")
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "missing.fq" in r.stderr
    r = _cli(tmp_path / "missing.bam", "-R", "chrX")
    assert r.returncode == 2 and "possible values: full, chrY, chrM" in r.stderr
    r = _cli()
    assert r.returncode == 2 and "fingerprint <INPUT>" in r.stderr
    r = _cli("--help")
    assert r.returncode == 0 and "only labels" in r.stderr
    r = subprocess.run([_b.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--max-low-mapq-fraction 0.1" in r.stderr and "fingerprint" in r.stderr


def test_input_kind(lib):
    err = C.create_string_buffer(256)
    for name, kind in (("a.bam", 1), ("a.fastq", 2), ("a.fq", 2), ("a.fq.gz", 2), ("a.fastq.gz", 2), ("x/y.gz", 2)):
        assert lib.dut_fp_input_kind(name.encode(), err, 256) == kind, name
    for name in ("a.sam", "a", ".bam", "a.BAM", "dir.bam/a", "a.fa"):
        assert lib.dut_fp_input_kind(name.encode(), err, 256) < 0, name
