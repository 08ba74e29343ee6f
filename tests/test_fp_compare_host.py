"""fingerprint-compare without a device: the host yardstick (dut_fpc_compare_host) against tests/fpc_ref.py on every case of
tests/fpc_cases.py, the reader of `fingerprint -o` files with each refusal and its line, the writers' NA rules, the command
line's argument errors, and csrc/fp_compare.h in a program of its own under AddressSanitizer + UBSan."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import fp_data
import fp_ref
import fpc_cases
import fpc_ref
from decodingustools_amd import _lib, build as _b
from decodingustools_amd import fingerprint as fpm


@pytest.fixture(scope="module")
def lib():
    _b.build()
    return _lib.load()


@pytest.fixture(scope="module")
def T(lib):
    return fpm.tile_size()


@pytest.fixture(scope="module")
def cases(T):
    return fpc_cases.cases(T)


def test_tile_constant_and_max_hash(lib, T):
    assert T >= 64 and T % 64 == 0
    for s in (0, 1, 2, 3, 7, 1000, 3000, 12345, 2 ** 40 + 3, 2 ** 63, 2 ** 64 - 1):
        assert fpc_ref.max_hash(s) == fp_ref.max_hash(s) == fpm.max_hash(s), s


def test_cases_are_what_they_claim(T, cases):
    """The seam cases put a common hash on each tile boundary of the merged order; the cut cases straddle the cut."""
    def merged(a, b):
        # (hash, which) sorted with the first sketch's element first on a tie
        both = sorted([(int(h), 0) for h in a[0]] + [(int(h), 1) for h in b[0]])
        return both
    for shift in (0, -1, 1):
        a, b = cases[f"seam_{shift}"][0]
        for x, y in ((a, b), (b, a)):
            m = merged(x, y)
            assert len(m) == 4 * T
            for d in (T, 2 * T, 3 * T):
                p = d - 1 + shift
                assert m[p][0] == m[p + 1][0] and (m[p][1], m[p + 1][1]) == (0, 1)
    a, b = cases["identical_2T+1"][0]
    assert len(a[0]) == 2 * T + 1 and np.array_equal(a[0], b[0])
    a, b = cases["all_below"][0]
    assert a[0][-1] < b[0][0]
    for name in ("cut_1000_3000", "cut_1_7"):
        sk = cases[name][0]
        mc = np.uint64(fpc_ref.max_hash(sk[1][3]))
        assert (sk[0][0] == mc).any() and (sk[1][0] == mc).any() and (sk[0][0] > mc).any() and (sk[0][0] < mc).any()
    r = fpc_ref.compare(cases["counts_max"][0], [(0, 1)])[0]
    assert int(r[3]) > 2 ** 32 and int(r[5]) > 2 ** 32 and int(r[5]) == int(r[3])


def test_compare_host_matches_reference(lib, cases):
    for name, (sk, pairs) in cases.items():
        want = fpc_ref.compare(sk, pairs)
        got = fpm.compare_host(sk, pairs)
        assert np.array_equal(got.records(), want), name
        # (j, i) is (i, j) with the a / b fields swapped
        rec = {p: r for p, r in zip(pairs, got.records())}
        for (i, j), r in rec.items():
            assert [int(x) for x in rec[(j, i)]] == [int(r[k]) for k in (1, 0, 2, 4, 3, 5)], (name, i, j)


def test_compare_host_many_pairs_and_threads(lib, T):
    sk = fpc_cases.many(T, n=12)
    pairs = fpc_ref.all_pairs(len(sk))
    want = fpc_ref.compare(sk, pairs)
    assert np.array_equal(fpm.compare_host(sk, pairs).records(), want)
    rng = np.random.default_rng(3)
    idx = rng.integers(0, len(pairs), size=100)
    assert np.array_equal(fpm.compare_host(sk, [pairs[i] for i in idx]).records(), want[idx])
    assert fpm.compare_host(sk, []).records().shape == (0, 6)


def test_ratios_nan_where_undefined(lib):
    e = (np.zeros(0, np.uint64), np.zeros(0, np.uint32), 31, 1000)
    one = (np.array([5], np.uint64), np.array([2], np.uint32), 31, 1000)
    r = fpm.compare_host([e, one], [(0, 0), (0, 1), (1, 1)])
    assert np.isnan(r.jaccard()[0]) and r.jaccard()[1] == 0.0 and r.jaccard()[2] == 1.0
    ca, cb = r.containment()
    assert np.isnan(ca[0]) and np.isnan(ca[1]) and cb[1] == 0.0 and ca[2] == 1.0
    assert np.isnan(r.weighted_jaccard()[0]) and r.weighted_jaccard()[2] == 1.0


def test_compare_host_refusals(lib):
    a = (np.array([1, 2, 3], np.uint64), np.array([1, 1, 1], np.uint32), 31, 1000)
    b = (np.array([1, 2, 3], np.uint64), np.array([1, 1, 1], np.uint32), 21, 1000)
    with pytest.raises(fpm.FingerprintError, match=r"pair 1 \(0, 1\): ksize 31 against ksize 21"):
        fpm.compare_host([a, b], [(0, 0), (0, 1)])
    with pytest.raises(fpm.FingerprintError, match="pair 0 .*out of range"):
        fpm.compare_host([a, b], [(0, 2)])
    with pytest.raises(fpm.FingerprintError, match="sketch 1: hashes are not strictly ascending at index 2"):
        fpm.compare_host([a, (np.array([1, 2, 2], np.uint64), a[1], 31, 1000)], [(0, 1)])
    with pytest.raises(fpm.FingerprintError, match="sketch 0: a count of 0 at index 1"):
        fpm.compare_host([(a[0], np.array([1, 0, 1], np.uint32), 31, 1000)], [(0, 0)])
    with pytest.raises(fpm.FingerprintError, match="index 0 is above max_hash"):
        fpm.compare_host([(np.array([2 ** 63], np.uint64), np.array([1], np.uint32), 31, 1000)], [(0, 0)])


def test_host_only_context(lib):
    with fpm.SketchSet(device=-1) as s:
        assert s.add(np.array([1, 5], np.uint64), np.array([1, 1], np.uint32)) == 0
        assert s.add(np.zeros(0, np.uint64), np.zeros(0, np.uint32)) == 1
        with pytest.raises(fpm.FingerprintError, match="index 1"):
            s.add(np.array([5, 5], np.uint64), np.array([1, 1], np.uint32))
        with pytest.raises(fpm.FingerprintError, match="count of 0 at index 0"):
            s.add(np.array([5], np.uint64), np.array([0], np.uint32))
        assert s.add(np.array([7], np.uint64), np.array([1], np.uint32)) == 2          # the refused ones took no id
        with pytest.raises(fpm.FingerprintError, match=r"\(-2\).*host-only"):
            s.compare([(0, 1)])


# ---- the file reader ----
def fp_text(r, k, scaled, region="full", mf=None, nl="\n", extra=()):
    head = [f"#ksize={k}", f"#scaled={scaled}", f"#region={region}"] + ([f"#max_frequency={mf}"] if mf is not None else []) + list(extra)
    return nl.join(head + [f"{int(h)}\t{int(c)}" for h, c in zip(r["hashes"], r["counts"])]) + nl


@pytest.fixture(scope="module")
def sketch():
    rng = np.random.default_rng(17)
    return fp_ref.sketch_seqs(fp_data.random_reads(60, rng, 40, 150, "ACGT"), 21, 20)


def test_file_round_trip(lib, tmp_path, sketch):
    """The format `fingerprint -o` writes (#ksize, #scaled, #region, optional #max_frequency, hash<TAB>count), restated here
    in fp_text() over the host restatement of the sketch: the real writer needs a device, and a file it wrote is read back
    in tests/test_gpu_fp_compare.py::test_command_line_end_to_end."""
    assert len(sketch["hashes"]) > 100
    for name, kw in (("a.fp", {}), ("crlf.fp", {"nl": "\r\n"}), ("mf.fp", {"mf": 7, "region": "chrM"}),
                     ("keys.fp", {"extra": ("#tool=other", "#comment without a value", "#date=2024-01-01")})):
        p = tmp_path / name
        p.write_bytes(fp_text(sketch, 21, 20, **kw).encode())
        s = fpm.read_fingerprint_file(p)
        assert (s.ksize, s.scaled, s.region, s.max_frequency) == (21, 20, kw.get("region", "full"), kw.get("mf")), name
        assert np.array_equal(s.hashes, sketch["hashes"]) and np.array_equal(s.counts, sketch["counts"]), name
        assert s.hashes.dtype == np.uint64 and s.counts.dtype == np.uint32
    # no final newline; an empty sketch with and without a final newline; the largest values
    p = tmp_path / "open.fp"
    p.write_bytes(fp_text(sketch, 21, 20).encode().rstrip(b"\n"))
    assert np.array_equal(fpm.read_fingerprint_file(p).hashes, sketch["hashes"])
    for text in (b"#ksize=31\n#scaled=1000\n#region=full\n", b"#ksize=31\n#scaled=1000", b"#scaled=1000\r\n#ksize=31\r\n"):
        p.write_bytes(text)
        s = fpm.read_fingerprint_file(p)
        assert (s.ksize, s.scaled, len(s.hashes), len(s.counts)) == (31, 1000, 0, 0)
    p.write_bytes(b"#ksize=64\n#scaled=1\n0\t1\n18446744073709551615\t4294967295\n")
    s = fpm.read_fingerprint_file(p)
    assert s.hashes.tolist() == [0, 2 ** 64 - 1] and s.counts.tolist() == [1, 2 ** 32 - 1]


REFUSALS = (
    (b"#ksize=31\n#scaled=1000\n5\t1\n7x\t1\n", 4, "hash"),
    (b"#ksize=31\n#scaled=1\n5\t1\n18446744073709551616\t1\n", 4, "overflowing hash"),
    (b"#ksize=31\n#scaled=1000\n5\t4294967296\n", 3, "overflowing count"),
    (b"#ksize=31\n#scaled=1000\n5\t-1\n", 3, "count"),
    (b"#ksize=31\n#scaled=1000\n5 1\n", 3, "expected hash<TAB>count"),
    (b"#ksize=31\n#scaled=1000\n5\t1\n\n6\t1\n", 4, "expected hash<TAB>count"),
    (b"#ksize=31\n#scaled=1000\n#region=full\n5\t1\n6\t0\n", 5, "count of 0"),
    (b"#ksize=31\n#scaled=1000\n5\t1\n5\t1\n", 4, "not strictly ascending"),
    (b"#ksize=31\n#scaled=1000\n9\t1\n5\t1\n", 4, "not strictly ascending"),
    (b"#ksize=31\r\n#scaled=1000\r\n5\t1\r\n18446744073709553\t1\r\n", 4, "above max_hash 18446744073709552"),
    (b"#ksize=31\n5\t1\n", 2, "missing #scaled="),
    (b"#scaled=10\n#region=full\n5\t1\n", 3, "missing #ksize="),
    (b"#region=full\n", 2, "missing #ksize="),
    (b"", 1, "missing #ksize="),
    (b"#ksize=0\n#scaled=1000\n", 1, "malformed ksize"),
    (b"#ksize=65\n#scaled=1000\n", 1, "malformed ksize"),
    (b"#ksize=31\n#scaled=1e3\n", 2, "malformed scaled"),
    (b"#ksize=31\n#scaled=1000\n#max_frequency=4294967296\n", 3, "malformed max_frequency"),
)


def test_file_refusals_name_the_line(lib, tmp_path):
    p = tmp_path / "bad.fp"
    for text, line, what in REFUSALS:
        p.write_bytes(text)
        with pytest.raises(fpm.FingerprintError) as e:
            fpm.read_fingerprint_file(p)
        assert str(e.value).startswith(f"{p}:{line}: ") and what in str(e.value), (text, str(e.value))
    # the last hash allowed by max_hash(1000) is accepted
    assert fpc_ref.max_hash(1000) == 18446744073709552
    p.write_bytes(b"#ksize=31\n#scaled=1000\n18446744073709552\t1\n")
    assert fpm.read_fingerprint_file(p).hashes.tolist() == [18446744073709552]
    with pytest.raises(fpm.FingerprintError, match="cannot open"):
        fpm.read_fingerprint_file(tmp_path / "missing.fp")


# ---- the writers ----
def _libc_file(path):
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    f = libc.fopen(str(path).encode(), b"wb")
    assert f
    return libc, f


def _write_table(lib, path, names, ksize, pairs, scaled, rec, min_jaccard=None):
    libc, f = _libc_file(path)
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    a = np.array([p[0] for p in pairs], np.uint32)
    b = np.array([p[1] for p in pairs], np.uint32)
    sc = np.array(scaled, np.uint64)
    rec = np.ascontiguousarray(rec, np.uint64)
    rc = lib.dut_fpc_write(f, arr, len(names), ksize, a.ctypes.data, b.ctypes.data, sc.ctypes.data, rec.ctypes.data, len(pairs),
                           0.0 if min_jaccard is None else min_jaccard, 0 if min_jaccard is None else 1)
    libc.fclose(f)
    assert rc == 0
    return open(path).read()


def test_writer_na_rules(lib, tmp_path):
    e = (np.zeros(0, np.uint64), np.zeros(0, np.uint32), 31, 1000)
    x = (np.array([5, 9, 11], np.uint64), np.array([2, 1, 4], np.uint32), 31, 3000)
    y = (np.array([5, 10, 11, 12], np.uint64), np.array([1, 1, 9, 1], np.uint32), 31, 1000)
    sk, names = [e, x, y], ["empty.fp", "dir/x.fp", "y.fp"]
    pairs = [(0, 0), (0, 1), (1, 0), (1, 2), (2, 2)]
    rec = fpc_ref.compare(sk, pairs)
    scaled = [fpc_ref.pair_scaled(sk[i], sk[j]) for i, j in pairs]
    assert scaled == [1000, 3000, 3000, 3000, 1000]
    got = _write_table(lib, tmp_path / "t.tsv", names, 31, pairs, scaled, rec)
    assert got == fpc_ref.table(names, sk, pairs, rec, 31)
    rows = [l.split("\t") for l in got.splitlines()[4:]]
    assert rows[0][7:10] == ["NA", "NA", "NA"] and rows[0][13] == "NA"              # empty against empty
    assert rows[1][7:10] == ["0.000000", "NA", "0.000000"] and rows[1][13] == "0.000000"
    assert rows[2][7:10] == ["0.000000", "0.000000", "NA"]
    assert rows[3][5:10] == ["2", "5", "0.400000", "0.666667", "0.500000"] and rows[3][10:] == ["7", "12", "5", "0.357143"]
    # --min-jaccard: lines below it (and NA) are left out, ##pairs= stays
    got = _write_table(lib, tmp_path / "t.tsv", names, 31, pairs, scaled, rec, min_jaccard=0.4)
    assert got == fpc_ref.table(names, sk, pairs, rec, 31, min_jaccard=0.4)
    assert got.splitlines()[1] == "##pairs=5" and len(got.splitlines()) == 4 + 2
    # the matrix: the diagonal is 1.000000, NA for the empty sketch
    allp = fpc_ref.all_pairs(3)
    rec = np.ascontiguousarray(fpc_ref.compare(sk, allp), np.uint64)
    libc, f = _libc_file(tmp_path / "m.tsv")
    arr = (C.c_char_p * 3)(*[n.encode() for n in names])
    ne = np.array([len(s[0]) for s in sk], np.uint64)
    assert lib.dut_fpc_write_matrix(f, arr, ne.ctypes.data, 3, rec.ctypes.data) == 0
    libc.fclose(f)
    got = open(tmp_path / "m.tsv").read()
    assert got == fpc_ref.matrix(names, sk)
    assert got.splitlines()[1].split("\t") == ["empty.fp", "NA", "0.000000", "0.000000"]
    assert got.splitlines()[2].split("\t") == ["dir/x.fp", "0.000000", "1.000000", "0.400000"]


# ---- the command line ----
def _cli(*args):
    return subprocess.run([_b.CLI, "fingerprint-compare"] + [str(a) for a in args], capture_output=True, text=True,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


def test_cli_argument_errors_exit_2_without_device(lib, tmp_path):
    a, b = tmp_path / "a.fp", tmp_path / "b.fp"
    for p in (a, b):
        p.write_bytes(b"#ksize=31\n#scaled=1000\n5\t1\n")
    out = tmp_path / "o.tsv"
    r = _cli(a, "-o", out)
    assert r.returncode == 2 and "at least two sketches" in r.stderr
    r = _cli("-o", out)
    assert r.returncode == 2 and "at least two sketches" in r.stderr
    r = _cli(a, b)
    assert r.returncode == 2 and "needs '-o <FILE>'" in r.stderr
    for x in ("x", "", "0.5x", "-0.1", "1.5", "nan"):
        r = _cli(a, b, "-o", out, "--min-jaccard", x)
        assert r.returncode == 2 and "--min-jaccard" in r.stderr, x
    r = _cli(a, b, "-o", out, "--query", a, "--matrix", tmp_path / "m.tsv")
    assert r.returncode == 2 and "--matrix" in r.stderr
    r = _cli(a, b, "-o", out, "--bogus")
    assert r.returncode == 2 and "unexpected argument" in r.stderr
    r = _cli("--help")
    assert r.returncode == 0 and "fingerprint-compare A.fp B.fp" in r.stderr
    assert not out.exists()
    # a list counts towards the two; a malformed file and mixed ksize exit 1 with the file (and line)
    lst = tmp_path / "list.txt"
    lst.write_text(f"{b}\r\n\n")
    bad = tmp_path / "bad.fp"
    bad.write_bytes(b"#ksize=31\n#scaled=1000\n5\t1\n4\t1\n")
    r = _cli(bad, "--list", lst, "-o", out)
    assert r.returncode == 1 and r.stderr.strip() == f"Error: {bad}:4: hashes are not strictly ascending"
    k21 = tmp_path / "k21.fp"
    k21.write_bytes(b"#ksize=21\n#scaled=1000\n5\t1\n")
    r = _cli(a, "--list", lst, k21, "-o", out)
    assert r.returncode == 1 and str(k21) in r.stderr and "ksize 21 against ksize 31" in r.stderr
    r = _cli(a, tmp_path / "missing.fp", "-o", out)
    assert r.returncode == 1 and "missing.fp: cannot open" in r.stderr
    r = _cli(a, "--list", tmp_path / "nolist.txt", "-o", out)
    assert r.returncode == 1 and "nolist.txt" in r.stderr
    assert not out.exists()
    r = subprocess.run([_b.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "fingerprint-compare" in r.stderr


# ---- fp_compare.h under the sanitizers ----
def _pack(sketches):
    out = [struct.pack("<Q", len(sketches))]
    for h, c, _, scaled in sketches:
        out += [struct.pack("<QQ", scaled, len(h)), np.asarray(h, "<u8").tobytes(), np.asarray(c, "<u4").tobytes()]
    return b"".join(out)


def test_fp_compare_header_under_sanitizers(tmp_path, T, cases, sketch):
    """The merge and the parser of csrc/fp_compare.h in tests/native/fp_compare_host.cpp, built with AddressSanitizer + UBSan
    and run directly: exact-size heap buffers for the seam, empty and cut cases; its numbers are the reference's and the
    sanitizers have nothing to say."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fp_compare_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(root, "tests", "native", "fp_compare_host.cpp"), "-o", exe]
    # a probe first: only a toolchain that cannot build an empty program with these flags skips; any other failure is one
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(cmd[:7] + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer runtimes not installed here: " + r.stderr[-300:])
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the sanitizer build failed:\n" + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1")
    for name in ("seam_0", "seam_-1", "seam_1", "seam_dense", "empty_empty", "empty_T+1", "one_equal", "one_unequal", "identical_2T+1",
                 "all_below", "unsigned_edges", "cut_1000_3000", "cut_1_7", "counts_max"):
        sk = cases[name][0]
        p = tmp_path / "m.bin"
        p.write_bytes(_pack(sk))
        r = subprocess.run([exe, "merge", str(p)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr[-3000:])
        got = {(int(v[0]), int(v[1])): [int(x) for x in v[2:]] for v in (l.split() for l in r.stdout.splitlines())}
        n = len(sk)
        want = fpc_ref.compare(sk, [(i, j) for i in range(n) for j in range(n)])
        assert [got[(i, j)] for i in range(n) for j in range(n)] == [[int(x) for x in w] for w in want], name
    p = tmp_path / "t.fp"
    for text, line, what in REFUSALS:
        p.write_bytes(text)
        r = subprocess.run([exe, "parse", str(p)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and r.stderr == "", (text, r.stderr[-3000:])
        assert r.stdout.startswith(f"error {line}: ") and what in r.stdout, (text, r.stdout)
    for text, want in ((fp_text(sketch, 21, 20, nl="\r\n", mf=3).encode(),
                        f"ok 21 20 {len(sketch['hashes'])} {int(sketch['hashes'].sum(dtype=np.uint64))} {int(sketch['counts'].sum())} full 3"),
                       (b"#ksize=31\n#scaled=1000", "ok 31 1000 0 0 0 - -"),
                       (b"#ksize=31\n#scaled=1000\n5\t1", "ok 31 1000 1 5 1 - -")):
        p.write_bytes(text)
        r = subprocess.run([exe, "parse", str(p)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.strip() == want, (r.stdout, r.stderr[-2000:])
