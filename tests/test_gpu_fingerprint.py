"""`fingerprint` on the device against tests/fp_ref.py: exact hashes, counts, processed, n_distinct and digest over
k, scaled, max_frequency and both input forms; many small batches; BAM vs FASTQ.gz; the command line end to end;
one case of more than 50 Mbases."""
import os
import subprocess

import numpy as np
import pytest

import fp_data
import fp_ref
from decodingustools_amd import build as _b
from decodingustools_amd.fingerprint import Fingerprint, fingerprint_file

pytestmark = pytest.mark.gpu

KS = (1, 2, 15, 16, 17, 21, 31, 32, 33, 51, 63, 64)
SCALED = (0, 1, 2, 7, 1000)


@pytest.fixture(scope="module")
def mixed():
    """Reads over BAM's 16 letters, ACGT reads with N, and reads with lower case and any byte."""
    _b.build()
    rng = np.random.default_rng(21)
    seqs = fp_data.random_reads(60, rng, 1, 200, "ACGT", n_rate=0.02)
    seqs += fp_data.random_reads(30, rng, 1, 200, fp_data.BAM_LETTERS)
    seqs += fp_data.random_reads(20, rng, 60, 200, "ACGTacgtRY=N", p=[.2, .2, .2, .2, .03, .03, .03, .03, .02, .02, .01, .01])
    seqs += [b"", b"A", b"ACGTACGTAC" * 7]
    return seqs


def _same(r, ref):
    assert r.processed == ref["processed"]
    assert r.n_distinct == ref["n_distinct"]
    assert np.array_equal(r.hashes, ref["hashes"])
    assert np.array_equal(r.counts, ref["counts"])
    assert r.hexdigest == ref["hexdigest"]


def test_bytes_against_reference(mixed):
    data, off = fp_ref.pack(mixed)
    for k in KS:
        for scaled in SCALED:
            for mf in (None, 1):
                with Fingerprint(k, scaled, mf) as fp:
                    fp.push(mixed)
                    _same(fp.finish(), fp_ref.sketch(data, off, k, scaled, mf))


def test_seq4_against_reference(mixed):
    seqs = [s for s in mixed if all(c in fp_ref.SEQ4_ALPHABET for c in s)]
    data, off = fp_ref.pack(seqs)
    s4 = fp_ref.encode_seq4(data)
    for k in KS:
        for scaled in (1, 7):
            with Fingerprint(k, scaled, 2 if k == 21 else None) as fp:
                fp.push((s4, off))
                _same(fp.finish(), fp_ref.sketch(data, off, k, scaled, 2 if k == 21 else None))


def test_offsets_are_checked():
    with Fingerprint(5, 1) as fp:
        with pytest.raises(RuntimeError, match="not ascending"):
            fp.push((np.zeros(8, np.uint8), np.array([0, 6, 3], np.uint64)))


def test_many_batches_equal_one(monkeypatch):
    data, off = fp_data.synthetic_reads(4000, 150, seed=4)
    ref = fp_ref.sketch(data, off, 31, 1)
    with Fingerprint(31, 1) as fp:
        fp.push((fp_ref.encode_seq4(data), off))
        one = fp.finish()
        assert fp.stats()["n_batches"] == 1
    _same(one, ref)
    monkeypatch.setenv("DUT_FP_BATCH_BASES", "2000")
    with Fingerprint(31, 1) as fp:
        fp.push((fp_ref.encode_seq4(data), off))
        many = fp.finish()
        assert fp.stats()["n_batches"] >= 300
    _same(many, ref)


def _cli(*args, env=None):
    return subprocess.run([_b.CLI, "fingerprint"] + [str(a) for a in args], capture_output=True, text=True, env=env)


def test_bam_and_fastq_cli(tmp_path):
    rng = np.random.default_rng(9)
    seqs = fp_data.random_reads(2000, rng, 10, 151, "ACGT", n_rate=0.01) + [b"ACG", b"A" * 20]
    bam, fq = tmp_path / "r.bam", tmp_path / "r.fq.gz"
    fp_data.write_reads_bam(bam, [s.decode() for s in seqs], block_every=13)
    fp_data.write_fastq(fq, seqs, gz=True, members=3)
    data, off = fp_ref.pack(seqs)
    for k, scaled, mf, region in ((31, 1000, None, "full"), (21, 2, 3, "chrY"), (5, 1, None, "chrM")):
        ref = fp_ref.sketch(data, off, k, scaled, mf)
        text = fp_ref.file_text(k, scaled, region, mf, ref["hashes"], ref["counts"])
        for path in (bam, fq):
            out = tmp_path / f"fp_{k}_{path.name}.txt"
            args = [path, "--ksize", k, "--scaled", scaled, "-o", out, "-R", region]
            if mf is not None:
                args += ["--max-frequency", mf]
            env = dict(os.environ, DUT_FP_BATCH_BASES="20000")
            r = _cli(*args, env=env)
            assert r.returncode == 0, r.stderr
            assert r.stdout == fp_ref.stdout_text(ref["processed"], ref["hexdigest"])
            assert out.read_text() == text
            if mf is not None:
                assert f"#max_frequency={mf}\n" in text
        assert fingerprint_file(bam, k, scaled, mf) == fingerprint_file(fq, k, scaled, mf)
    # defaults, no -o
    r = _cli(fq)
    ref = fp_ref.sketch(data, off, 31, 1000)
    assert r.returncode == 0 and r.stdout == fp_ref.stdout_text(ref["processed"], ref["hexdigest"])


def test_large_against_reference():
    n, L = 360_000, 150                                      # 54 Mbases
    data, off = fp_data.synthetic_reads(n, L, seed=77)
    ref = fp_ref.sketch(data, off, 31, 1000)
    with Fingerprint(31, 1000) as fp:
        fp.push((fp_ref.encode_seq4(data), off))
        _same(fp.finish(), ref)
