#!/usr/bin/env python3
"""What the depth profile costs on one GPU, on the chr21-shaped 30x resident contig of bench.py (same generator, seed).

  1. cl_contig_depth_profile(1001, 500), call to return and its kernel by device events, against the only other route
     to the same numbers: cl_debug_depths (raw + qc to the host) and a numpy reduction.  Same build, same process,
     alternating repetitions; medians and ranges.  The ordinary step (cl_contig_run + sync) of the same run beside it.
  2. The kernel's time for a few other (n_bins, window).

    python tools/depth_profile_bench.py [--length 46709983] [--depth 30] [--reps 5] [--out FILE]
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


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def resident_engine(opt, rec, ref, L, tmpd):
    eng = Engine(opt, 0)
    counter = CallableProfiler(os.path.join(tmpd, "g.bed"))
    process_single_contig(eng, counter, ContigProfiler("chr21", L), opt, 20, rec, ref)
    counter.close()
    eng.set_profiling(True)
    return eng


def kernel_ms(eng, n_bins, window, reps):
    eng.depth_profile(n_bins, window)
    return [eng.depth_profile(n_bins, window).kernel_ms for _ in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=46_709_983)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_depth_profile.json"))
    a = ap.parse_args()
    L = a.length
    seed = synth.seed_for(2, 20)
    rec = synth.short_read_contig(L, a.depth, seed)
    ref = synth.make_reference(L, seed)
    opt = CallableOptions()
    tmpd = tempfile.mkdtemp()
    out = {"workload": f"synthetic chr21-shaped contig, {L} bp, {a.depth}x, {rec.n} reads (bench.py's generator and seed), resident on one GPU",
           "reps": a.reps}

    eng = resident_engine(opt, rec, ref, L, tmpd)
    s = eng.contig_collect().summary
    extent = int(s.extent)
    out["layout"] = eng.contig_layout()
    inb, outb = eng.contig_bytes()
    out["resident_input_bytes"] = int(inb)

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

    # 1. the profile against the debug route, alternating
    raw = np.zeros(extent, np.uint32)
    qc = np.zeros(extent, np.uint32)
    p_wall, p_kern, d_copy, d_reduce = [], [], [], []
    eng.depth_profile(1001, 500)
    for _ in range(a.reps):
        t0 = time.perf_counter()
        p = eng.depth_profile(1001, 500)
        p_wall.append((time.perf_counter() - t0) * 1e3)
        p_kern.append(p.kernel_ms)
        t0 = time.perf_counter()
        st = eng._lib.cl_debug_depths(eng._h, raw.ctypes.data_as(C.c_void_p), qc.ctypes.data_as(C.c_void_p), None, None, extent)
        assert st == 0
        t1 = time.perf_counter()
        starts = np.arange(0, extent, 500)
        ref_p = dict(hist_raw=np.bincount(np.minimum(raw, 1000), minlength=1001), hist_qc=np.bincount(np.minimum(qc, 1000), minlength=1001),
                     win_raw=np.add.reduceat(raw.astype(np.uint64), starts), win_qc=np.add.reduceat(qc.astype(np.uint64), starts))
        t2 = time.perf_counter()
        d_copy.append((t1 - t0) * 1e3)
        d_reduce.append((t2 - t1) * 1e3)
        for k, v in ref_p.items():
            assert np.array_equal(getattr(p, k), v.astype(np.uint64)), k
        assert p.sum_raw == s.summed_coverage and p.sum_qc == s.quality_bases
    out["depth_profile_1001_500"] = {"measured_against": "cl_debug_depths (raw + qc) + numpy bincount / add.reduceat, same process, alternating",
                                     "call_to_return_ms": spread(p_wall), "kernel_ms_by_events": spread(p_kern),
                                     "n_windows": int(p.n_windows), "result_bytes": int(8 * (2 + 2 * 1001 + 2 * p.n_windows))}
    out["debug_route"] = {"cl_debug_depths_raw_qc_ms": spread(d_copy), "numpy_reduction_ms": spread(d_reduce),
                          "total_ms": spread([x + y for x, y in zip(d_copy, d_reduce)]), "bytes_to_host": int(8 * extent)}
    out["kernel_over_ordinary_step"] = statistics.median(p_kern) / out["ordinary_step"]["kernels_ms_by_events"]
    shapes = {}
    for nb, S in ((1001, 0), (1001, 16), (1001, 2048), (17, 500), (4096, 500)):
        shapes[f"{nb},{S}"] = spread(kernel_ms(eng, nb, S, a.reps))
    out["kernel_ms_by_shape"] = {"measured_against": "each other: (n_bins, window)", **shapes}
    eng.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
