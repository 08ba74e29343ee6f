"""`fingerprint` without a device: the numpy restatement against the known answers, the library's shared hash code,
max_hash and SHA-256 against it, the BAM and FASTQ readers, and the command line's argument and format errors."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import fp_cases as F
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


def test_edge_lengths_and_seam_bytes_every_k(lib):
    """The shared hash code, strip after strip as the kernel cuts them, on the inputs of the device's edge tests."""
    for k in range(1, 65):
        seqs = F.edge_lengths(k) + F.seam_bytes(k)
        rh, rhn = fp_ref.window_hashes(*fp_ref.pack(seqs), k)
        got = [fpm.kmer_hashes_host(s, k) for s in seqs]
        h, hn = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
        assert np.array_equal(hn, rhn) and np.array_equal(h[~hn], rh[~rhn]), k
        assert [len(g[0]) for g in got[:11]] == [0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 130]
        seqs = F.edge_lengths(k) + F.seam_bytes(k, seq4=True)
        rh, rhn = fp_ref.window_hashes(*fp_ref.pack(seqs), k)
        got = [fpm.kmer_hashes_host_seq4(fp_ref.encode_seq4(np.frombuffer(s, np.uint8)), len(s), k) for s in seqs]
        h, hn = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
        assert np.array_equal(hn, rhn) and np.array_equal(h[~hn], rh[~rhn]), k
    # what the seam cases are for: a special byte on each side of the first three seams, and a strip without a live window
    for k in F.KS:
        places = F.seam_places(k)
        assert {63, 64, 127, 128, 64 + k - 1, 64 + k - 2, 5 * 64 - 1, 5 * 64 + k - 2} <= set(places)
        assert len(F.seam_bytes(k)) == 4 * len(places) + 2 and len(F.seam_bytes(k, seq4=True)) == 3 * len(places) + 2
        _, hn = fp_ref.kmer_hashes(F.seam_bytes(k)[-2], k)           # N over [64, 127 + k): windows 65 - k .. 126 + k
        assert hn[64:128].all() and hn[max(65 - k, 0):127 + k].all() and not hn[127 + k] and not hn[64 - k]
        _, hn = fp_ref.kmer_hashes(F.seam_bytes(k)[-1], k)           # N over [63, 128 + k): windows 64 - k .. 127 + k
        assert hn[max(64 - k, 0):128 + k].all() and not hn[128 + k] and (k == 64 or not hn[63 - k])


def _write_long_fastq(path, seqs, members=0, crlf=False, final_newline=True):
    nl = b"\r\n" if crlf else b"\n"
    recs = [b"@r%d long" % i + nl + s + nl + b"+" + nl + b"I" * len(s) + nl for i, s in enumerate(seqs)]
    if not final_newline:
        recs[-1] = recs[-1][:-len(nl)]
    with open(path, "wb") as f:
        if not members:
            f.write(b"".join(recs))
        else:
            step = (len(recs) + members - 1) // members
            for i in range(0, len(recs), step):
                f.write(gzip.compress(b"".join(recs[i:i + step]), 1))


@pytest.fixture(scope="module")
def long_lines():
    """Sequence lines around and beyond the reader's refill of 1 MiB, an empty one, and two short ones."""
    rng = np.random.default_rng(31)
    return [bytes(F.ACGT[rng.integers(0, 4, size=n)]) for n in ((3 << 20) + 17, 1 << 20, (1 << 20) - 1, 0, 100, 50)]


FASTQ_FORMS = (("plain.fq", {}), ("two.fq.gz", {"members": 2}), ("crlf.fq", {"crlf": True}), ("open_end.fq", {"final_newline": False}))


def test_fastq_reader_long_lines(lib, tmp_path, long_lines):
    for name, kw in FASTQ_FORMS:
        p = tmp_path / name
        _write_long_fastq(p, long_lines, **kw)
        for cap in (1, 1000, 1 << 30):
            got = _fastq_walk(lib, p, cap)
            assert [len(s) for s in got] == [len(s) for s in long_lines], (name, cap)
            assert got == long_lines, (name, cap)


@pytest.fixture(scope="module")
def long_bam(tmp_path_factory):
    p = tmp_path_factory.mktemp("fp_long") / "long.bam"
    fp_data.write_reads_bam(p, [s.decode() for s in F.file_reads()])
    return p


def test_bam_walk_long_record(lib, long_bam):
    want = list(F.file_reads())
    assert len(want[0]) == 1 and len(want[2]) == 1 and len(want[1]) == F.BIG_LINE and len(want[1]) % 2 == 0
    assert os.path.getsize(long_bam) > 4 * 65536                  # (the long record alone is many BGZF blocks)
    for cap in (1, 20_000, 1 << 30):
        got, batches = _bam_walk(lib, long_bam, cap)
        assert [len(s) for s in got] == [len(s) for s in want], cap
        assert got == want, cap
        # one batch: the long record from base 1, its followers from an odd and an even base; small caps: from base 0
        assert batches == {1: len(want), 20_000: batches, 1 << 30: 1}[cap] and (cap == 1 << 30 or batches >= 5), (cap, batches)


def _checksum(seqs):
    """tests/native/fp_readers_host.cpp's, in numpy's wrapping 64-bit arithmetic."""
    b = np.frombuffer(b"".join(seqs), np.uint8).astype(np.uint64)
    lens = np.array([len(s) for s in seqs], np.uint64)
    with np.errstate(over="ignore"):
        s = ((np.arange(len(b), dtype=np.uint64) + np.uint64(1)) * (b + np.uint64(1))).sum(dtype=np.uint64)
        s += (((np.arange(len(lens), dtype=np.uint64) + np.uint64(1)) * lens) << np.uint64(32)).sum(dtype=np.uint64)
    return int(s)


def test_fp_readers_under_sanitizers(tmp_path, long_lines, long_bam):
    """dut_fastq_next and dut_bam_next_seqs, in a program of their own under AddressSanitizer + UBSan, on the long-line
    files: the numbers it prints are Python's, and the sanitizers have nothing to say."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "decodingustools_amd", "csrc")
    exe = str(tmp_path / "fp_readers_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(root, "tests", "native", "fp_readers_host.cpp"), os.path.join(csrc, "fastq_io.cpp"), os.path.join(csrc, "bam_io.cpp"),
           os.path.join(csrc, "qual_pack.cpp"), "-lz", "-ldl", "-lpthread", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if any(m in r.stderr for m in ("cannot find -lasan", "cannot find -lubsan", "unrecognized command-line option", "unrecognized argument")):
            pytest.skip("sanitizer runtimes not installed here: " + r.stderr[-300:])
        pytest.fail("the sanitizer build failed:\n" + r.stderr[-3000:])
    runs = []
    for name, kw in FASTQ_FORMS:
        _write_long_fastq(tmp_path / name, long_lines, **kw)
        runs += [(tmp_path / name, "fastq", cap, long_lines) for cap in (1, 1000, 1 << 30)]
    runs += [(long_bam, "bam", cap, list(F.file_reads())) for cap in (1, 20_000, 1 << 30)]
    for path, kind, cap, seqs in runs:
        r = subprocess.run([exe, str(path), kind, str(cap)], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0", DUT_THREADS="3"))
        assert r.returncode == 0 and r.stderr == "", (path, cap, r.stderr[-3000:])
        rec, bases, chk, batches = (int(x) for x in r.stdout.split())
        assert (rec, bases, chk) == (len(seqs), sum(len(s) for s in seqs), _checksum(seqs)), (path, cap)
        assert batches == 1 if cap == 1 << 30 else batches > 1, (path, cap, batches)


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
