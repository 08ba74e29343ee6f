"""fingerprint-compare on the device against tests/fpc_ref.py, exactly: sizes around the tile, a common hash across every
tile seam (both ways round), degenerate merge paths, unsigned order, the cut between two `scaled` values, counts whose sums
pass 2^32, many pairs of very different tile counts in one launch, reuse of a context, sketches straight from the
`fingerprint` engine, and the command line end to end.  The inputs are tests/fpc_cases.py's; T is the kernel's tile."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fp_data
import fpc_cases
import fpc_ref
from decodingustools_amd import _lib, build as _b
from decodingustools_amd import fingerprint as fpm
from decodingustools_amd.fingerprint import Fingerprint, SketchSet

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    _b.build()


@pytest.fixture(scope="module")
def T():
    return fpm.tile_size()


@pytest.fixture(scope="module")
def cases(T):
    return fpc_cases.cases(T)


def device_records(sketches, pairs):
    with SketchSet() as s:
        for i, sk in enumerate(sketches):
            assert s.add(*sk) == i
        return s.compare(pairs)


def check_case(cases, name):
    sk, pairs = cases[name]
    got = device_records(sk, pairs)
    want = fpc_ref.compare(sk, pairs)
    for p, (g, w) in enumerate(zip(got.records(), want)):
        assert g.tolist() == w.tolist(), (name, pairs[p], dict(zip(fpc_ref.FIELDS, g.tolist())), dict(zip(fpc_ref.FIELDS, w.tolist())))
    return got, want


@pytest.mark.parametrize("which", ["T-1", "T", "T+1", "2T+1"])
def test_sizes_around_the_tile(cases, T, which):
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[which]
    got, _ = check_case(cases, f"both_{n}")
    assert got.n_tiles == sum(-(-(int(a) + int(b)) // T) for a, b in zip(got.n_a, got.n_b))
    assert got.bytes == 12 * int((got.n_a + got.n_b).sum()) and got.kernel_ms > 0


@pytest.mark.parametrize("name", ["mixed_3T+5_7", "mixed_T+1_2T-1", "empty_empty", "empty_T+1", "one_equal", "one_unequal"])
def test_mixed_and_tiny_sizes(cases, name):
    got, _ = check_case(cases, name)
    if name == "empty_empty":
        assert got.n_tiles == 0 and not got.records().any() and np.isnan(got.jaccard()).all()
    if name == "one_equal":
        assert got.n_common.tolist() == [1, 1, 1, 1] and got.sum_min.tolist() == [3, 3, 3, 7]


@pytest.mark.parametrize("name", ["seam_0", "seam_-1", "seam_1", "seam_dense"])
def test_match_across_a_tile_seam_counts_once(cases, T, name):
    """A common hash as the last element of a tile whose partner opens the next one, at every boundary of a 4-tile pair; pair
    (1, 0) is the mirror image (the roles exchanged, the seams at the same places)."""
    got, want = check_case(cases, name)
    assert got.n_tiles >= 2 * 4 and int(want[1][2]) >= 3


def test_every_element_common(cases, T):
    got, _ = check_case(cases, "identical_2T+1")
    n = 2 * T + 1
    assert got.n_common.tolist() == [n] * 4
    assert got.sum_min[0] == got.sum_a[0] == got.sum_b[0] and got.sum_min[1] == got.sum_a[1]


@pytest.mark.parametrize("name", ["all_below", "even_odd"])
def test_degenerate_merge_paths(cases, name):
    got, _ = check_case(cases, name)
    assert got.n_common[1] == 0 and got.n_common[2] == 0 and got.n_common[0] == got.n_a[0]


@pytest.mark.parametrize("name", ["unsigned_edges", "unsigned_random"])
def test_unsigned_order(cases, name):
    got, _ = check_case(cases, name)
    if name == "unsigned_edges":
        rec = dict(zip(cases[name][1], got.records().tolist()))
        assert rec[(0, 1)] == [5, 5, 5, 15, 15, 9] and rec[(0, 2)][:3] == [5, 2, 2] and rec[(3, 0)][:3] == [2, 5, 2]


@pytest.mark.parametrize("name", ["cut_1000_3000", "cut_1_7"])
def test_cut_between_two_scaled_values(cases, name):
    got, _ = check_case(cases, name)
    sk, pairs = cases[name]
    rec = dict(zip(pairs, got.records().tolist()))
    assert rec[(0, 1)][0] < len(sk[0][0]) and rec[(0, 0)][0] == len(sk[0][0]) and rec[(0, 2)][0] == len(sk[0][0])
    for (i, j), r in rec.items():
        assert rec[(j, i)] == [r[k] for k in (1, 0, 2, 4, 3, 5)], (i, j)


def test_counts_pass_32_bits(cases):
    got, _ = check_case(cases, "counts_max")
    assert int(got.sum_min[1]) > 2 ** 32 and int(got.sum_a[1]) > 2 ** 32


def test_refusals_leave_the_context_usable(cases):
    a, b = cases["one_equal"][0]
    with SketchSet() as s:
        s.add(*a)
        s.add(b[0], b[1], 21, 1000)
        s.add(*b)
        with pytest.raises(fpm.FingerprintError, match=r"pair 1 \(1, 0\): ksize 21 against ksize 31"):
            s.compare([(0, 2), (1, 0)])
        with pytest.raises(fpm.FingerprintError, match="out of range"):
            s.compare([(0, 3)])
        with pytest.raises(fpm.FingerprintError, match="index 1"):
            s.add(np.array([4, 4], np.uint64), np.array([1, 1], np.uint32))
        lib = _lib.load()
        out = C.c_void_p()
        assert lib.dut_fpc_compare(s._ctx, None, None, 1, C.byref(out)) == -1 and b"null pair arrays" in lib.dut_fpc_last_error(s._ctx)
        assert lib.dut_fpc_compare(s._ctx, None, None, 0, None) == -1 and b"null out" in lib.dut_fpc_last_error(s._ctx)
        assert lib.dut_fpc_compare(s._ctx, None, None, 0, C.byref(out)) == 0 and not out.value
        assert lib.dut_fpc_compare(s._ctx, None, None, (1 << 24) + 1, C.byref(out)) == -1
        assert b"DUT_FPC_MAX_PAIRS" in lib.dut_fpc_last_error(s._ctx)
        assert s.compare([(0, 2), (1, 1)]).records().tolist() == [[1, 1, 1, 3, 7, 3], [1, 1, 1, 7, 7, 7]]
        assert s.compare([]).records().shape == (0, 6)


def test_too_many_tiles_is_refused_before_a_launch(T):
    """2^24 pairs of 128 tiles each are 2^31 tiles: refused with the count, and the context goes on working."""
    rng = np.random.default_rng(5)
    big = fpc_cases.subset(rng, fpc_cases.universe(rng, 64 * T, fpc_ref.max_hash(1000)), 64 * T)
    with SketchSet() as s:
        s.add(*big)
        pairs = np.zeros((1 << 24, 2), np.uint32)
        with pytest.raises(fpm.FingerprintError, match=str(2 ** 31) + " tiles"):
            s.compare(pairs)
        assert s.compare([(0, 0)]).n_common.tolist() == [64 * T]


@pytest.fixture(scope="module")
def many(T):
    sk = fpc_cases.many(T)
    pairs = fpc_ref.all_pairs(len(sk))
    return sk, pairs, fpc_ref.compare(sk, pairs)


def test_many_pairs_one_launch(many):
    sk, pairs, want = many
    assert len(pairs) == 780
    with SketchSet() as s:
        for x in sk:
            s.add(*x)
        got = s.compare_all()
        assert np.array_equal(got.records(), want)
        # the same pairs shuffled, with repeats and some turned round: the records in the order given
        rng = np.random.default_rng(9)
        idx = np.concatenate([rng.permutation(len(pairs)), rng.integers(0, len(pairs), size=200)])
        flip = rng.random(idx.size) < 0.3
        asked = [(pairs[i][1], pairs[i][0]) if f else pairs[i] for i, f in zip(idx, flip)]
        expect = want[idx].copy()
        expect[flip] = expect[flip][:, [1, 0, 2, 4, 3, 5]]
        assert np.array_equal(s.compare(asked).records(), expect)


@pytest.mark.parametrize("grid_x", [1, 13, 1000])
def test_tiles_laid_out_in_grid_rows(many, monkeypatch, grid_x):
    """One launch takes fewer than 2^24 workgroups in x, so the tiles of a call lie in rows of DUT_FPC_GRID_X (default 2^22):
    rows of 1, 13 and 1000 tiles over the 780 pairs (3 031 tiles at T = 2 048), the last row short."""
    sk, pairs, want = many
    monkeypatch.setenv("DUT_FPC_GRID_X", str(grid_x))
    with SketchSet() as s:
        for x in sk:
            s.add(*x)
        got = s.compare_all()
    assert got.n_tiles > 1000 and (grid_x == 1 or got.n_tiles % grid_x) and np.array_equal(got.records(), want)


def test_two_to_the_24_tiles_in_one_call(T):
    """2^17 times the pair (0, 0) of a sketch of 64 T entries: 2^24 tiles, more than one grid row can hold."""
    rng = np.random.default_rng(6)
    big = fpc_cases.subset(rng, fpc_cases.universe(rng, 64 * T, fpc_ref.max_hash(1000)), 64 * T)
    with SketchSet() as s:
        s.add(*big)
        got = s.compare(np.zeros((1 << 17, 2), np.uint32))
    assert got.n_tiles == 1 << 24
    want = fpc_ref.compare([big], [(0, 0)])[0]
    assert (got.records() == want[None, :]).all()


def test_reuse_of_a_context(many):
    sk, pairs, want = many
    half = len(sk) // 2
    lib = _lib.load()
    with SketchSet() as s:
        for x in sk[:half]:
            s.add(*x)
        first = fpc_ref.all_pairs(half)
        a = np.array([p[0] for p in first], np.uint32)
        b = np.array([p[1] for p in first], np.uint32)
        raw = []
        for _ in range(2):
            out = C.c_void_p()
            assert lib.dut_fpc_compare(s._ctx, a.ctypes.data, b.ctypes.data, len(first), C.byref(out)) == 0
            raw.append(C.string_at(out, 48 * len(first)))
        assert raw[0] == raw[1]                                       # two calls: identical bytes
        assert raw[0] == fpc_ref.compare(sk, first).astype("<u8").tobytes()
        for x in sk[half:]:                                           # add after a compare, then compare again
            s.add(*x)
        assert np.array_equal(s.compare_all().records(), want)


def test_sketch_straight_from_the_engine():
    rng = np.random.default_rng(23)
    reads = fp_data.random_reads(400, rng, 60, 150, "ACGT")
    with Fingerprint(ksize=21, scaled=4) as fp:
        fp.push(reads)
        whole = fp.finish()
    with Fingerprint(ksize=21, scaled=4) as fp:
        fp.push(reads[:200])
        part = fp.finish()
    assert len(whole.hashes) > 4000 and 0 < len(part.hashes) < len(whole.hashes)
    sk = [(whole.hashes, whole.counts, 21, 4), (part.hashes, part.counts, 21, 4)]
    with SketchSet() as s:
        assert s.add(whole, ksize=21, scaled=4) == 0 and s.add(part, ksize=21, scaled=4) == 1
        got = s.compare([(0, 0), (0, 1)])
    assert np.array_equal(got.records(), fpc_ref.compare(sk, [(0, 0), (0, 1)]))
    assert got.jaccard()[0] == 1.0 and got.containment()[1][1] == 1.0 and got.n_common[1] == len(part.hashes)


def test_command_line_end_to_end(tmp_path):
    """`fingerprint -o` on small FASTQs, then `fingerprint-compare` with --matrix and with --query."""
    rng = np.random.default_rng(41)
    reads = fp_data.random_reads(300, rng, 50, 120, "ACGT")
    sets = {"a": reads[:200], "b": reads[100:], "c": [b"ACGTNN"]}                     # c: an empty sketch
    names = []
    for n, seqs in sets.items():
        fq, out = tmp_path / f"{n}.fq", tmp_path / f"{n}.fp"
        fp_data.write_fastq(fq, seqs)
        scaled = "6" if n == "b" else "2"
        r = subprocess.run([_b.CLI, "fingerprint", str(fq), "--ksize", "21", "--scaled", scaled, "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        names.append(str(out))
    files = [fpm.read_fingerprint_file(n) for n in names]
    sk = [(f.hashes, f.counts, f.ksize, f.scaled) for f in files]
    assert len(sk[0][0]) > 1000 and len(sk[2][0]) == 0 and [s[3] for s in sk] == [2, 6, 2]
    tsv, mat = tmp_path / "out.tsv", tmp_path / "m.tsv"
    r = subprocess.run([_b.CLI, "fingerprint-compare"] + names + ["-o", str(tsv), "--matrix", str(mat)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    pairs = fpc_ref.all_pairs(3)
    assert tsv.read_text() == fpc_ref.table(names, sk, pairs, fpc_ref.compare(sk, pairs), 21)
    assert mat.read_text() == fpc_ref.matrix(names, sk)
    assert tsv.read_text().splitlines()[4].split("\t")[2] == "6"                       # compared at the coarser scaled
    lst = tmp_path / "list.txt"
    lst.write_text(names[2] + "\n")
    r = subprocess.run([_b.CLI, "fingerprint-compare", "--query", names[1], names[0], "--list", str(lst), "-o", str(tsv), "--min-jaccard", "0.05"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    order = [names[1], names[0], names[2]]
    sk2 = [sk[1], sk[0], sk[2]]
    pairs = [(0, 1), (0, 2)]
    want = fpc_ref.table(order, sk2, pairs, fpc_ref.compare(sk2, pairs), 21, min_jaccard=0.05)
    assert tsv.read_text() == want and len(want.splitlines()) == 5 and "##pairs=2" in want
    assert fpm.compare_files(names, matrix=mat) == fpc_ref.table(names, sk, fpc_ref.all_pairs(3), fpc_ref.compare(sk, fpc_ref.all_pairs(3)), 21)
