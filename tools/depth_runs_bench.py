#!/usr/bin/env python3
"""What the depth runs cost on one GPU, on the chr21-shaped 30x resident contig of bench.py (same generator, seed).

cl_contig_depth_runs, exact raw and quantized 1:4:100 -- call to return and its launches by device events --, against the
only other route to the same runs: cl_debug_depths (the raw array to the host) and a numpy run-length encoding.  Same
build, same process, alternating repetitions; medians and ranges.  The ordinary step (cl_contig_run + sync) of the same
run beside it.

    python tools/depth_runs_bench.py [--length 46709983] [--depth 30] [--reps 5] [--out FILE]
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

EDGES = [1, 4, 100]


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def rle(depth, edges):
    v = depth if not edges else np.searchsorted(np.asarray(edges, np.uint32), depth, side="right").astype(np.uint32)
    start = np.flatnonzero(np.concatenate(([True], v[1:] != v[:-1]))).astype(np.uint32)
    return start, v[start]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=46_709_983)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_depth_runs.json"))
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
    extent = int(eng.contig_collect().summary.extent)
    out["layout"] = eng.contig_layout()

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
    wall = {"exact": [], "quantized": []}
    kern = {"exact": [], "quantized": []}
    d_copy, d_rle = [], {"exact": [], "quantized": []}
    got = {}
    eng.depth_runs("raw")                                          # (the buffers' first allocation is not what is measured)
    eng.depth_runs("raw", EDGES)
    for _ in range(a.reps):
        for key, edges in (("exact", None), ("quantized", EDGES)):
            t0 = time.perf_counter()
            r = eng.depth_runs("raw", edges)
            wall[key].append((time.perf_counter() - t0) * 1e3)
            kern[key].append(r.kernel_ms)
            got[key] = r
        t0 = time.perf_counter()
        st = eng._lib.cl_debug_depths(eng._h, raw.ctypes.data_as(C.c_void_p), None, None, None, extent)
        assert st == 0
        d_copy.append((time.perf_counter() - t0) * 1e3)
        for key, edges in (("exact", None), ("quantized", EDGES)):
            t0 = time.perf_counter()
            s, v = rle(raw, edges)
            d_rle[key].append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(got[key].start, s) and np.array_equal(got[key].value, v), key
    for key in ("exact", "quantized"):
        out["depth_runs_raw_" + key] = {
            "edges": [] if key == "exact" else EDGES,
            "measured_against": "cl_debug_depths (raw) + numpy run-length encoding, same process, alternating",
            "call_to_return_ms": spread(wall[key]), "kernel_ms_by_events": spread(kern[key]),
            "n_runs": int(got[key].n_runs), "bytes_returned": int(8 * got[key].n_runs),
            "kernel_over_ordinary_step": statistics.median(kern[key]) / out["ordinary_step"]["kernels_ms_by_events"]}
        out["debug_route_" + key] = {"cl_debug_depths_raw_ms": spread(d_copy), "numpy_rle_ms": spread(d_rle[key]),
                                     "total_ms": spread([x + y for x, y in zip(d_copy, d_rle[key])]), "bytes_to_host": int(4 * extent)}
    # the other kind, for the record: the qc runs read the rows instead of the heads
    eng.depth_runs("qc")
    out["depth_runs_qc_exact_kernel_ms_by_events"] = spread([eng.depth_runs("qc").kernel_ms for _ in range(a.reps)])
    eng.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
