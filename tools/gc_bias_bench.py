#!/usr/bin/env python3
"""What the GC-bias profile costs on one GPU, on the chr21-shaped 30x resident contig of bench.py (same generator, seed).

  cl_contig_gc_bias for W = 100 and W = 1024 (K = 4): the kernel by device events, pack + upload of the reference's two
  bit planes by the host's clock, and call to return -- against the kernel of cl_contig_depth_profile(1001, 0) of the
  same run (the same residents, the same rebuild of both depths), the ordinary step of the same run, and the only other
  route to the same numbers: cl_debug_depths (raw + qc to the host) and the numpy restatement of the rule.  Same build,
  same process, alternating repetitions; medians and ranges.  Every repetition's record is compared with the restatement's.

    python tools/gc_bias_bench.py [--length 46709983] [--depth 30] [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from decodingustools_amd import (CallableOptions, CallableProfiler, ContigProfiler, Engine,  # noqa: E402
                                 process_single_contig, synth)

BINS = 101
WINDOWS = ((100, 4), (1024, 4))


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def restate(raw, qc, ref, window, max_invalid):
    """the rule of include/callable_loci.h in numpy (as tests/gc_ref.py: class tables, cumsum differences, bincount)"""
    is_gc = np.zeros(256, np.int64)
    is_valid = np.zeros(256, np.int64)
    for c in b"GCgc":
        is_gc[c] = 1
    for c in b"ACGTacgt":
        is_valid[c] = 1
    extent = raw.shape[0]
    before = window // 2
    n = extent + window
    gc = np.zeros(n, np.int64)
    inv = np.ones(n, np.int64)
    have = max(0, min(len(ref), n - before))
    gc[before:before + have] = is_gc[ref[:have]]
    inv[before:before + have] = 1 - is_valid[ref[:have]]
    cg = np.concatenate(([0], np.cumsum(gc)))
    ci = np.concatenate(([0], np.cumsum(inv)))
    g = cg[window:window + extent] - cg[:extent]
    v = ci[window:window + extent] - ci[:extent]
    ok = v <= max_invalid
    b = (100 * g[ok]) // (window - v[ok])
    r, q = raw[ok], qc[ok]
    return dict(n_skipped=int(extent - ok.sum()), positions=np.bincount(b, minlength=BINS).astype(np.uint64),
                sum_raw=np.bincount(b, weights=r.astype(np.float64), minlength=BINS).astype(np.uint64),
                sum_qc=np.bincount(b, weights=q.astype(np.float64), minlength=BINS).astype(np.uint64),
                zero_raw=np.bincount(b[r == 0], minlength=BINS).astype(np.uint64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=46_709_983)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_gc_bias.json"))
    a = ap.parse_args()
    L = a.length
    seed = synth.seed_for(2, 20)
    rec = synth.short_read_contig(L, a.depth, seed)
    ref = synth.make_reference(L, seed)
    opt = CallableOptions()
    tmpd = tempfile.mkdtemp()
    out = {"workload": f"synthetic chr21-shaped contig, {L} bp, {a.depth}x, {rec.n} reads (bench.py's generator and seed), resident on one GPU",
           "reps": a.reps}
    eng = Engine(opt, 0)
    counter = CallableProfiler(os.path.join(tmpd, "g.bed"))
    process_single_contig(eng, counter, ContigProfiler("chr21", L), opt, 20, rec, ref)
    counter.close()
    eng.set_profiling(True)
    s = eng.contig_collect().summary
    extent = int(s.extent)
    out["layout"] = eng.contig_layout()
    out["reference_bits_bytes"] = int((-(-extent // 2048) * 2048 + 1024) // 4)

    # the ordinary step of the same run: the yardstick
    for _ in range(3):
        eng.contig_run()
    eng.sync()
    eng.reset_kernel_ms()
    t0 = time.perf_counter()
    for _ in range(20):
        eng.contig_run()
    eng.sync()
    step_ms = (time.perf_counter() - t0) * 1e3 / 20
    ms, n = eng.kernel_ms()
    out["ordinary_step"] = {"what": "cl_contig_run x 20 + cl_sync, per step", "wall_ms": step_ms,
                            "kernels_ms_by_events": float(sum(ms.values())) / max(int(n), 1)}

    raw = np.zeros(extent, np.uint32)
    qc = np.zeros(extent, np.uint32)
    wall = {w: [] for w in WINDOWS}
    kern = {w: [] for w in WINDOWS}
    upl = {w: [] for w in WINDOWS}
    prof_kern, d_copy, d_np = [], [], {w: [] for w in WINDOWS}
    for w, k in WINDOWS:
        eng.gc_bias(ref, w, k)
    eng.depth_profile(1001, 0)
    for _ in range(a.reps):
        got = {}
        for w, k in WINDOWS:
            t0 = time.perf_counter()
            g = eng.gc_bias(ref, w, k)
            wall[(w, k)].append((time.perf_counter() - t0) * 1e3)
            kern[(w, k)].append(g.kernel_ms)
            upl[(w, k)].append(g.upload_ms)
            got[(w, k)] = g
        prof_kern.append(eng.depth_profile(1001, 0).kernel_ms)
        t0 = time.perf_counter()
        st = eng._lib.cl_debug_depths(eng._h, raw.ctypes.data_as(C.c_void_p), qc.ctypes.data_as(C.c_void_p), None, None, extent)
        assert st == 0
        d_copy.append((time.perf_counter() - t0) * 1e3)
        for w, k in WINDOWS:
            t0 = time.perf_counter()
            exp = restate(raw, qc, ref, w, k)
            d_np[(w, k)].append((time.perf_counter() - t0) * 1e3)
            g = got[(w, k)]
            assert g.n_skipped == exp["n_skipped"] and int(g.positions.sum()) + g.n_skipped == extent, (w, k)
            for f in ("positions", "sum_raw", "sum_qc", "zero_raw"):
                assert np.array_equal(getattr(g, f), exp[f]), (w, k, f)
    prof = statistics.median(prof_kern)
    out["depth_profile_1001_0_kernel_ms"] = spread(prof_kern)
    for w, k in WINDOWS:
        out[f"gc_bias_W{w}_K{k}"] = {"kernel_ms_by_events": spread(kern[(w, k)]), "pack_upload_ms": spread(upl[(w, k)]),
                                     "call_to_return_ms": spread(wall[(w, k)]),
                                     "kernel_over_depth_profile_kernel": statistics.median(kern[(w, k)]) / prof,
                                     "kernel_over_ordinary_step": statistics.median(kern[(w, k)]) / out["ordinary_step"]["kernels_ms_by_events"],
                                     "numpy_restatement_ms": spread(d_np[(w, k)])}
    out["debug_route"] = {"measured_against": "cl_debug_depths (raw + qc) + the numpy restatement of the rule, same process, alternating",
                          "cl_debug_depths_raw_qc_ms": spread(d_copy), "bytes_to_host": int(8 * extent)}
    out["results_equal_on_every_repetition"] = True
    eng.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
