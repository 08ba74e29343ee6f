"""The pass-bit rows as the device holds them -- a row stack per SEGMENT of 256 positions, pass_rows.h:
rows_window_segments -- held against the one-stack-per-window builder (rows_window, cl_debug_pass_rows) through a
context without a device: the same column sum at every position, every segment exactly as high as its deepest column
asks for, and the equal-heights form (DUT_ROWS_UNIFORM=1) with the same sums."""
import numpy as np
import pytest

from decodingustools_amd import CallableOptions, synth
from decodingustools_amd.callable_loci import HostStage

T, S = 2048, 256


def stage(rec, L):
    """-> (groups per window and rows of the one-stack layout, heights, height words and units of the segments' layout)."""
    with HostStage(CallableOptions()) as st:
        st.contig_begin(0, L, None)
        st.push_reads(rec.pos, rec.mapq, rec.cigar_off, rec.cigar, rec.qual_off, rec.qual)
        ng, rows, _ = st.pass_rows()
        h, words, units = st.pass_rows_segments()
    return ng, rows, h, words, units


def sums_uniform(ng, rows):
    qc = np.zeros(ng.shape[0] * T, np.int64)
    off = 0
    for w, n in enumerate(int(x) for x in ng):
        if n:
            g = rows[off * 256:(off + n) * 256].reshape(n, 64, 4)                    # [group][block][row & 3]
            bits = np.unpackbits(g.view(np.uint8).reshape(n, 64, 4, 4), axis=-1, bitorder="little")
            qc[w * T:(w + 1) * T] = bits.reshape(n, 64, 4, 32).sum(axis=(0, 2)).reshape(T)
        off += n
    assert rows.shape[0] == off * 256
    return qc


def sums_segments(h, units):
    qc = np.zeros(h.shape[0] * T, np.int64)
    off = 0
    for w in range(h.shape[0]):
        for s in range(8):
            n = int(h[w, s])
            if n:
                g = units[off * 32:(off + n) * 32].reshape(n, 8, 4)                  # [unit][block & 7][row & 3]
                bits = np.unpackbits(g.view(np.uint8).reshape(n, 8, 4, 4), axis=-1, bitorder="little")
                qc[w * T + s * S:w * T + (s + 1) * S] = bits.reshape(n, 8, 4, 32).sum(axis=(0, 2)).reshape(S)
            off += n
    assert units.shape[0] == off * 32
    return qc


def row_reads(rec, opt):
    """(start, end, sparse) of the reads that get a row: mapq >= min, a quality string, a reference span."""
    ops, lens = rec.cigar & 15, (rec.cigar >> 4).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(np.where(np.isin(ops, (0, 2, 3, 7, 8)), lens, 0))])
    span = cs[rec.cigar_off[1:].astype(np.int64)] - cs[rec.cigar_off[:-1].astype(np.int64)]
    ql = (rec.qual_off[1:] - rec.qual_off[:-1]).astype(np.int64)
    nops = (rec.cigar_off[1:] - rec.cigar_off[:-1]).astype(np.int64)
    keep = (rec.mapq >= opt.min_mapping_quality) & (ql > 0) & (span > 0)
    pos = rec.pos.astype(np.int64)
    sparse = keep & (nops > 1) & (span > 4 * ql + 1024)
    return pos[keep], (pos + span)[keep], bool(sparse.any())


def deepest_per_segment(start, end, n_win):
    d = np.zeros(n_win * T + 1, np.int64)
    np.add.at(d, np.minimum(start, n_win * T), 1)
    np.add.at(d, np.minimum(end, n_win * T), -1)
    return np.cumsum(d)[:n_win * T].reshape(n_win, 8, S).max(axis=2)


def check(rec, L, monkeypatch):
    opt = CallableOptions()
    monkeypatch.delenv("DUT_ROWS_UNIFORM", raising=False)
    ng, rows, h, words, units = stage(rec, L)
    n_win = ng.shape[0]
    assert h.shape == (n_win, 8) and n_win >= 2
    want = sums_uniform(ng, rows)
    assert np.array_equal(sums_segments(h, units), want)
    start, end, any_sparse = row_reads(rec, opt)
    deepest = deepest_per_segment(start, end, n_win)
    if any_sparse:
        assert (h <= ng[:, None]).all()
    else:
        assert np.array_equal(h, (deepest + 3) // 4)
        assert np.array_equal(h.max(axis=1), ng)
    # the record's word: the eight heights as bytes, or 0 when a segment is beyond 255 units (then all are equal)
    for w in range(n_win):
        if int(h[w].max()) > 255 or int(h[w].max()) == 0:
            assert int(words[w]) == 0 and (h[w] == h[w].max()).all()
        else:
            assert [(int(words[w]) >> (8 * s)) & 0xFF for s in range(8)] == [int(x) for x in h[w]]
    # ... and the equal-heights form of every window
    monkeypatch.setenv("DUT_ROWS_UNIFORM", "1")
    ng2, rows2, hu, wu, uu = stage(rec, L)
    assert np.array_equal(ng2, ng) and np.array_equal(rows2, rows)
    assert (wu == 0).all() and (hu == hu[:, :1]).all()
    assert np.array_equal(hu[:, 0], h.max(axis=1))
    assert np.array_equal(sums_segments(hu, uu), want)
    return int(h.sum()), int(ng.sum()) * 8


@pytest.mark.parametrize("L,depth,seed", [(3 * T + 77, 30, 3), (6 * T, 12, 4), (2 * T - 1, 70, 5)])
def test_short_reads(L, depth, seed, monkeypatch):
    check(synth.short_read_contig(L, depth, synth.seed_for(2, seed)), L, monkeypatch)


@pytest.mark.parametrize("L,depth,seed", [(5 * T, 20, 23), (6 * T - 300, 50, 24)])
def test_long_reads_with_gaps(L, depth, seed, monkeypatch):
    check(synth.long_read_contig(L, depth, synth.seed_for(3, seed)), L, monkeypatch)


@pytest.mark.parametrize("deep", [False, True])
def test_adversarial(deep, monkeypatch):
    L = 4 * T + 13
    check(synth.adversarial_contig(L, 3000 if deep else 600, synth.seed_for(4, 7), deep=deep), L, monkeypatch)


def test_share_of_the_uniform_layout_chr21_model(monkeypatch, record_property):
    """The chr21 model of the benchmark, a 6 Mb stretch: what a stack per segment stores against a stack per window
    (about 0.85 expected: depth varies along 2048 positions).  The heights are the assertion (check); the share is
    recorded and follows from them."""
    L = 6_000_000
    units, uniform_units = check(synth.short_read_contig(L, 30, synth.seed_for(2, 20)), L, monkeypatch)
    share = units / uniform_units
    record_property("rows_share_of_uniform", round(share, 4))
    print(f"units {units} of {uniform_units} in the uniform layout: share {share:.4f}")
    assert share < 1.0
