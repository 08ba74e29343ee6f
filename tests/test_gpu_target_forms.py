"""k_target_depth and k_target_order on every form the residents of a run take (-m gpu): heads of 8 bytes, candidates from
the wide list (more of them than a workgroup has threads), spans cut into several heads, long reads, and 8, 16 and 32
counter planes under 8-byte heads.  The two kernels rebuild both depths with the code of k_depth_profile and k_depth_runs
(window_depths.hip.h), one instantiation per (counter planes, head form); tests/test_gpu_targets.py and
tests/test_gpu_target_order.py run them on short reads alone, which take the 4-byte heads.

Every case goes through the check of both of those files, unchanged: every set of target_sets and their union against
tests/targets_ref.py / tests/order_ref.py over the CPU oracle's per-position depths and over the engine's own dump, the
call repeated, interleaved with its siblings, the run repeated.  A third test per case shows which head form was
resident: the same input on a second engine with DUT_HEADS8 flipped, the bytes of the two compared.  Whole numbers:
everything is exact."""
import functools

import numpy as np
import pytest

import depth_contigs
import test_gpu_parity
import test_gpu_target_order
import test_gpu_targets
from test_gpu_targets import target_sets, union
from decodingustools_amd import CallableProfiler, ContigProfiler, Engine, process_single_contig, synth

pytestmark = pytest.mark.gpu
T = depth_contigs.T
HOOKS = ("DUT_HEADS8", "DUT_HEAD_SPAN", "DUT_QUAL_FORM", "DUT_ROWS_UNIFORM")   # (read when an engine is made)
DEEP_THR = ((255, 256), (32767, 32768), (65_999, 66_000, 66_001))


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)


class Case:
    """contig, o_res: what depth_contigs' builders give; env: the hooks the engines of the case are made under; heads:
    "forced" -- 4-byte heads but for DUT_HEADS8 -- or "own" -- 8-byte heads whatever DUT_HEADS8 says; planes: the counter
    planes the contig takes (None: not pinned); records: (lo, hi), bounds of the layout's n_records over the reads with a
    reference span"""
    def __init__(self, built, options, env=None, heads="own", planes=None, records=(None, None), thresholds=()):
        self.contig, self.o_res, self.extent, self.depths = built
        self.options, self.env, self.heads, self.planes, self.records = options, dict(env or {}), heads, planes, records
        self.thresholds = test_gpu_targets.THRESHOLDS + tuple(thresholds)


@functools.lru_cache(maxsize=None)
def _cut_spans():
    """57 long reads, 2 of them wide"""
    rec = synth.long_read_contig(60_000, 8, 17)
    span = depth_contigs.ref_spans(rec)
    assert rec.n == 57 and int((span > depth_contigs.WIDE_SPAN).sum()) == 2 and 37 < int(span.min()) and int(span.max()) < 70_000
    return depth_contigs._with_oracle(("chrL", 2, 60_000, synth.make_reference(60_000, 3), rec), None)


@functools.lru_cache(maxsize=None)
def _long_reads():
    """the indel-rich shape at 50x: every window has wide candidates, most of them tens"""
    L = 300_000
    rec = synth.long_read_contig(L, 50, synth.seed_for(3, 23))
    pos, span = rec.pos.astype(np.int64), depth_contigs.ref_spans(rec)
    wide = span > depth_contigs.WIDE_SPAN
    per_window = np.asarray([int(((pos[wide] < (w + 1) * T) & ((pos + span)[wide] > w * T)).sum()) for w in range(L // T)])
    assert per_window.min() >= 1 and int((per_window >= 10).sum()) > L // T // 2
    return depth_contigs._with_oracle(("chrY", 23, L, synth.make_reference(L, synth.seed_for(3, 23)), rec), {})


@functools.lru_cache(maxsize=None)
def _shapes():
    """leading clips, match runs beyond 65 535 bases (wide), quality strings cut short and absent"""
    L, rec, ref = test_gpu_parity.record_shapes_contig(L=20_000, seed=4242, n_plain=400, short_form=False)
    # (of the reads that start inside the contig: the product path hands the engine no other)
    assert int(((depth_contigs.ref_spans(rec) > 65_535) & (rec.pos < L)).sum()) >= 3
    return depth_contigs._with_oracle(("chrS", 4, L, ref, rec), {})


@functools.lru_cache(maxsize=None)
def _adversarial():
    """tests/test_gpu_targets.py, test_adversarial_contigs[True-True-6143]: no span beyond kWideSpan"""
    L = 6143
    rec = synth.adversarial_contig(L, 700, 2000 + L, max_len=300, deep=True, overhang=True)
    assert int(depth_contigs.ref_spans(rec).max()) <= depth_contigs.WIDE_SPAN
    return depth_contigs._with_oracle(("chrA", L % 3, L, synth.make_reference(L, 60 + L % 7, lowercase=(L % 2 == 0)), rec),
                                      dict(min_depth=2, min_depth_for_low_mapq=3))


@functools.lru_cache(maxsize=None)
def case(name):
    heads8 = dict(DUT_HEADS8="1")
    if name == "wide_only":
        built = depth_contigs.wide_list()
        depth_contigs.assert_wide_only_windows(built[0][4], built[3])
        return Case(built, depth_contigs.WIDE_OPTIONS)
    if name in ("wide_pile[150]", "wide_pile[300]"):
        # (300 wide reads 5 positions apart put 71 rows on a segment: the 16 planes take the 400 passing reads of n_deep)
        built = depth_contigs.wide_pile(150) if name == "wide_pile[150]" else depth_contigs.wide_pile(300, 400)
        assert len(depth_contigs.assert_wide_pile_windows(built[0][4], built[3])) >= 9
        return Case(built, depth_contigs.PILE_OPTIONS, planes=8 if name == "wide_pile[150]" else 16)
    if name == "cut_spans[37]":
        n = _cut_spans()[0][4].n
        return Case(_cut_spans(), None, env=dict(DUT_HEAD_SPAN="37"), records=(100 * n, None))
    if name == "cut_spans[70000]":
        return Case(_cut_spans(), None, env=dict(DUT_HEAD_SPAN="70000"), records=(None, _cut_spans()[0][4].n))
    if name == "long_reads":
        return Case(_long_reads(), {})
    if name == "shapes":
        return Case(_shapes(), {})
    if name == "heads8[8]":
        return Case(_adversarial(), dict(min_depth=2, min_depth_for_low_mapq=3), env=heads8, heads="forced", planes=8, thresholds=DEEP_THR[:2])
    if name in ("heads8[16]", "heads8[32]"):
        built = depth_contigs.deep_pile(300 if name == "heads8[16]" else 66_000)
        return Case(built, depth_contigs.DEEP_OPTIONS, env=heads8, heads="forced", planes=16 if name == "heads8[16]" else 32, thresholds=DEEP_THR)
    raise KeyError(name)


CASES = ["wide_only", "wide_pile[150]", "wide_pile[300]", "cut_spans[37]", "cut_spans[70000]", "long_reads", "shapes",
         "heads8[8]", "heads8[16]", "heads8[32]"]


def _setenv(monkeypatch, env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name", CASES)
def test_target_depth(name, tmp_path, monkeypatch):
    c = case(name)
    _setenv(monkeypatch, c.env)
    test_gpu_targets.check([c.contig], c.options, tmp_path, o_res=c.o_res, thresholds=c.thresholds)


@pytest.mark.parametrize("name", CASES)
def test_target_order(name, tmp_path, monkeypatch):
    c = case(name)
    _setenv(monkeypatch, c.env)
    test_gpu_target_order.check([c.contig], c.options, tmp_path, o_res=c.o_res)


def _resident(c, env, monkeypatch, tmp_path):
    """the case's contig on an engine made under env: (bytes of the heads and rows, layout, the records of target_stats
    and of target_order over the union of target_sets, as bytes)"""
    _setenv(monkeypatch, env)
    name, tid, length, ref, rec = c.contig
    opt = test_gpu_targets._opts(c.options)
    with Engine(opt, 0) as eng:
        counter = CallableProfiler(str(tmp_path / "g.bed"))
        process_single_contig(eng, counter, ContigProfiler(name, length), opt, tid, rec, ref)   # (as the two checks)
        counter.close()
        extent = int(eng.contig_collect().summary.extent)
        assert extent == c.extent
        ua, ub = union(target_sets(extent))
        return (eng.contig_bytes(), eng.contig_layout(), eng.target_stats(ua, ub, test_gpu_targets.EIGHT).records().tobytes(),
                eng.target_order(ua, ub).records().tobytes())


@pytest.mark.parametrize("name", CASES)
def test_head_form(name, monkeypatch, tmp_path):
    """Which head form the two tests above ran: the resident bytes under the case's hooks and with DUT_HEADS8 flipped.  A
    "forced" case takes 4 bytes more per head with the hook than without, and both forms give the same records; an "own"
    case has the same bytes either way, since its heads were of 8 bytes already."""
    c = case(name)
    flipped = {k: v for k, v in c.env.items() if k != "DUT_HEADS8"}
    if "DUT_HEADS8" not in c.env:
        flipped["DUT_HEADS8"] = "1"
    (nbytes, lay, st, od), (f_bytes, f_lay, f_st, f_od) = _resident(c, c.env, monkeypatch, tmp_path), _resident(c, flipped, monkeypatch, tmp_path)
    n_heads = lay["n_records"]
    assert n_heads == f_lay["n_records"] > 0
    if c.heads == "forced":
        assert nbytes[0] - f_bytes[0] == 4 * n_heads and nbytes[1] == f_bytes[1]
        assert lay["upload_h2d_bytes"] - f_lay["upload_h2d_bytes"] == 4 * (n_heads + 1)
    else:
        assert nbytes == f_bytes and lay["upload_h2d_bytes"] == f_lay["upload_h2d_bytes"]
    assert st == f_st and od == f_od
    if c.planes is not None:
        assert lay["counter_planes"] == f_lay["counter_planes"] == c.planes
    lo, hi = c.records
    assert (lo is None or n_heads >= lo) and (hi is None or n_heads <= hi)
