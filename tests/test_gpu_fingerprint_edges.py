"""`fingerprint` on the device where its first tests do not reach, against tests/fp_ref.py and exactly: sequences of many
strips (a read that crosses waves and workgroups), window counts on the strip size, a special byte at every place around a
strip seam, batches cut at odd bases, batches that never reach the kernel or leave no survivor, counts that add up between the
table and a later batch with max_frequency on the sums, a context pushed and finished more than once, the caller's own
stream, and both readers on a read of more than a million bases.  The inputs are tests/fp_cases.py's."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import fp_cases as F
import fp_data
import fp_ref
from decodingustools_amd import _lib, build as _b
from decodingustools_amd.fingerprint import Fingerprint, fingerprint_file

pytestmark = pytest.mark.gpu

MIX_SEED = 7                                # (at cap 1001: 33 batches launched, 17 of them from an odd base, the N read a batch alone)


@pytest.fixture(scope="module", autouse=True)
def built():
    _b.build()


@functools.lru_cache(maxsize=None)
def ref(seqs, k, scaled, mf=None):
    return fp_ref.sketch(*fp_ref.pack(seqs), k, scaled, mf)


def same(r, want):
    assert r.processed == want["processed"]
    assert r.n_distinct == want["n_distinct"]
    assert np.array_equal(r.hashes, want["hashes"])
    assert np.array_equal(r.counts, want["counts"])
    assert r.hexdigest == want["hexdigest"]


def sketch(seqs, k, scaled, mf=None, seq4=False):
    """One context, one push -> (result, batches launched)."""
    with Fingerprint(k, scaled, mf) as fp:
        fp.push(F.seq4_of(seqs) if seq4 else list(seqs))
        return fp.finish(), fp.stats()["n_batches"]


def launched(seqs, cap, k):
    """The batches of the restated split rule that have a sequence of k bases: the ones `push` launches."""
    lens = [len(s) for s in seqs]
    return sum(1 for i0, i1 in F.split(lens, cap) if max(lens[i0:i1]) >= k)


@pytest.mark.parametrize("k", F.KS)
def test_edge_lengths_and_seam_bytes(k, monkeypatch):
    edges = F.edge_lengths(k)
    for cap in (None, 300):
        if cap:
            monkeypatch.setenv("DUT_FP_BATCH_BASES", str(cap))
        for seq4 in (False, True):
            for seqs in (edges, edges[::-1], F.seam_bytes(k, seq4)):
                for scaled in (1, 7):
                    r, n = sketch(seqs, k, scaled, seq4=seq4)
                    same(r, ref(seqs, k, scaled))
                    assert n == (launched(seqs, cap, k) if cap else 1), (cap, seq4, scaled)


@pytest.mark.parametrize("k", (1, 21, 32, 33, 64))
def test_long_read(k):
    seqs = (F.long_read(5),)
    assert (F.LONG - 64 + 1 + F.STRIP - 1) // F.STRIP > 2 * 256           # strips of three workgroups at every k
    for seq4 in (False, True):
        for scaled in (1, 1000):
            r, n = sketch(seqs, k, scaled, seq4=seq4)
            same(r, ref(seqs, k, scaled))
            assert n == 1


def test_homopolymer_whole_and_in_reads(monkeypatch):
    whole = (b"A" * F.LONG,)
    want = ref(whole, 31, 1)
    assert want["counts"].tolist() == [F.LONG - 30] == [32_970]
    for seq4 in (False, True):
        r, n = sketch(whole, 31, 1, seq4=seq4)
        same(r, want)
        assert n == 1
    reads = tuple(whole[0][i:i + 100] for i in range(0, F.LONG, 100))
    want = ref(reads, 31, 1)
    assert want["counts"].tolist() == [330 * 70] == [23_100]
    monkeypatch.setenv("DUT_FP_BATCH_BASES", "1000")
    for seq4 in (False, True):
        r, n = sketch(reads, 31, 1, seq4=seq4)
        same(r, want)
        assert n == 33                                                     # the one hash is in the table 32 times over


@pytest.mark.parametrize("k", (5, 31, 64))
def test_batch_seams(k, monkeypatch):
    cap = 1001
    seqs = F.batch_mix(MIX_SEED)
    B = F.batches(seqs, cap, k)
    up = [b for b in B if b["has_k"]]
    # what this input is for, by the restated split rule and the reference alone
    assert sum(b["first_base"] & 1 for b in up) >= 8
    assert any(not b["has_k"] for b in B)
    assert any(b["has_k"] and not b["has_clean_window"] for b in B[1:])
    assert any(b["i1"] - b["i0"] == 1 and len(seqs[b["i0"]]) == F.BIG for b in B)
    _, times = np.unique(np.concatenate([b["hashes"] for b in B]), return_counts=True)
    assert int((times >= 2).sum()) >= 100
    turned = F.batch_mix_n_first(MIX_SEED)
    T = F.batches(turned, cap, k)
    assert T[0]["has_k"] and not T[0]["has_clean_window"] and T[1]["has_k"] and T[1]["has_clean_window"]
    for seq4 in (False, True):
        for scaled in (1, 7):
            one, n = sketch(seqs, k, scaled, seq4=seq4)
            assert n == 1
            same(one, ref(seqs, k, scaled))
            monkeypatch.setenv("DUT_FP_BATCH_BASES", str(cap))
            many, n = sketch(seqs, k, scaled, seq4=seq4)
            assert n == len(up)
            same(many, ref(seqs, k, scaled))
            assert np.array_equal(many.hashes, one.hashes) and np.array_equal(many.counts, one.counts) and many.hexdigest == one.hexdigest
            # the batch without a survivor first: an empty table behind it, the second batch copied into it
            r, n = sketch(turned, k, scaled, seq4=seq4)
            assert n == sum(b["has_k"] for b in T)
            same(r, ref(turned, k, scaled))
            assert r.hexdigest == one.hexdigest
            monkeypatch.delenv("DUT_FP_BATCH_BASES")


def test_counts_across_batches_and_max_frequency(monkeypatch):
    k, cap = 31, 3100
    seqs = F.tandem(k)
    assert all(i1 - i0 == 3 for i0, i1 in F.split([len(s) for s in seqs], cap)[:-1])
    whole = ref(seqs, k, 1)
    classes = sorted(set(whole["counts"].tolist()))
    assert classes == [33, 34] and whole["n_distinct"] == 997            # so 32, 33 and 34 cut below, between and above
    for mf, left in ((None, 997), (0, 0), (32, 0), (33, int((whole["counts"] == 33).sum())), (34, 997)):
        want = ref(seqs, k, 1, mf)
        assert len(want["hashes"]) == left and want["n_distinct"] == 997 and 0 < int((whole["counts"] == 33).sum()) < 997
        for seq4 in (False, True):
            monkeypatch.setenv("DUT_FP_BATCH_BASES", str(cap))
            r, n = sketch(seqs, k, 1, mf, seq4=seq4)
            assert n == 12 and r.n_distinct == 997
            same(r, want)
            monkeypatch.delenv("DUT_FP_BATCH_BASES")
            r, n = sketch(seqs, k, 1, mf, seq4=seq4)
            assert n == 1 and r.n_distinct == 997
            same(r, want)


def test_context_life():
    k = 31
    A = F.edge_lengths(k) + F.seam_bytes(k)[:24]
    B = F.seam_bytes(k, seq4=True)[10:40] + F.edge_lengths(k)[3:]          # some of A again: keys the table holds
    Cs = (b"", b"ACGT", b"N" * 30, b"ACGTACGTACGTACGTACGTACGTACGTAC")
    assert set(A) & set(B) and all(len(s) < k for s in Cs)
    with Fingerprint(k, 1) as fp:
        fp.push(list(A))
        first = fp.finish()
        same(first, ref(A, k, 1))
        again = fp.finish()
        assert np.array_equal(again.hashes, first.hashes) and np.array_equal(again.counts, first.counts)
        assert (again.hexdigest, again.processed, again.n_distinct) == (first.hexdigest, first.processed, first.n_distinct)
        fp.push(F.seq4_of(B))
        fp.push([])
        fp.push((np.zeros(0, np.uint8), np.zeros(1, np.uint64)))
        fp.push(list(Cs))
        last = fp.finish()
        same(last, ref(A + B + Cs, k, 1))
        assert last.processed == sum(len(s) >= k for s in A + B + Cs) and last.n_distinct > first.n_distinct
    r, _ = sketch(A + B + Cs, k, 1)
    assert r.hexdigest == last.hexdigest and r.processed == last.processed


def test_empty_finishes():
    empty = fp_ref.digest([], [])
    for k, pushes in ((31, ()), (31, ([b"ACGT", b"", b"A" * 30],)), (64, ([], [b"C" * 63])), (1, ([b""],))):
        for mf in (None, 0):
            with Fingerprint(k, 1, mf) as fp:
                for p in pushes:
                    fp.push(p)
                for _ in range(2):
                    r = fp.finish()
                    assert (r.hexdigest, r.n_distinct, r.processed, len(r.hashes), len(r.counts)) == (empty, 0, 0, 0, 0)
                assert fp.stats()["n_batches"] == 0


def test_two_contexts_same_bytes(monkeypatch):
    seqs = F.batch_mix(MIX_SEED) + (F.long_read(6),)
    for cap in (None, 1001):
        if cap:
            monkeypatch.setenv("DUT_FP_BATCH_BASES", str(cap))
        a, _ = sketch(seqs, 21, 2, seq4=True)
        b, _ = sketch(seqs, 21, 2, seq4=True)
        assert a.hashes.tobytes() == b.hashes.tobytes() and a.counts.tobytes() == b.counts.tobytes() and a.hexdigest == b.hexdigest
        same(a, ref(seqs, 21, 2))


def test_callers_stream():
    import torch
    lib = _lib.load()
    k = 31
    seqs = F.edge_lengths(k) + (F.long_read(7),)
    data, off = fp_ref.pack(seqs)
    want = ref(seqs, k, 1, 5)
    stream = torch.cuda.Stream(device=0)
    opt = _lib.dut_fp_options()
    opt.ksize, opt.scaled, opt.has_max_frequency, opt.max_frequency = k, 1, 1, 5
    ctx = C.c_void_p()
    assert lib.dut_fp_create(C.byref(opt), 0, C.c_void_p(stream.cuda_stream), C.byref(ctx)) == 0
    try:
        assert lib.dut_fp_push_bytes(ctx, data.ctypes.data, off.ctypes.data, len(seqs)) == 0, lib.dut_fp_last_error(ctx)
        r = _lib.dut_fp_result()
        assert lib.dut_fp_finish(ctx, C.byref(r)) == 0, lib.dut_fp_last_error(ctx)
        n = int(r.n_entries)
        h = np.ctypeslib.as_array(C.cast(r.hashes, C.POINTER(C.c_uint64)), (n,)).copy()
        c = np.ctypeslib.as_array(C.cast(r.counts, C.POINTER(C.c_uint32)), (n,)).copy()
    finally:
        lib.dut_fp_destroy(ctx)
    assert (int(r.processed), int(r.n_distinct), r.hexdigest.decode()) == (want["processed"], want["n_distinct"], want["hexdigest"])
    assert np.array_equal(h, want["hashes"]) and np.array_equal(c, want["counts"])
    # the stream is the caller's: it works on behind the context
    with torch.cuda.stream(stream):
        total = torch.arange(1000, device="cuda:0", dtype=torch.int64).sum()
    stream.synchronize()
    assert int(total.item()) == 499_500


def test_long_read_files(tmp_path, monkeypatch):
    seqs = F.file_reads()
    k, scaled = 31, 1000
    bam, fq = tmp_path / "long.bam", tmp_path / "long.fq.gz"
    fp_data.write_reads_bam(bam, [s.decode() for s in seqs])
    fp_data.write_fastq(fq, list(seqs), gz=True, members=2)
    want = ref(seqs, k, scaled)
    text = fp_ref.file_text(k, scaled, "full", None, want["hashes"], want["counts"])
    monkeypatch.setenv("DUT_FP_BATCH_BASES", "20000")
    got = {}
    for path in (bam, fq):
        out = tmp_path / f"lib_{path.name}.txt"
        got[path] = fingerprint_file(path, k, scaled, output=out)
        assert got[path] == (want["processed"], want["hexdigest"])
        assert out.read_text() == text
        out = tmp_path / f"cli_{path.name}.txt"
        r = subprocess.run([_b.CLI, "fingerprint", str(path), "--ksize", str(k), "--scaled", str(scaled), "-o", str(out)],
                           capture_output=True, text=True, env=dict(os.environ, DUT_FP_BATCH_BASES="20000"))
        assert r.returncode == 0, r.stderr
        assert r.stdout == fp_ref.stdout_text(want["processed"], want["hexdigest"])
        assert out.read_text() == text
    assert got[bam] == got[fq]
