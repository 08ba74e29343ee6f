#!/usr/bin/env python3
"""What the per-target summaries cost on one GPU, on the chr21-shaped 30x resident contig of bench.py (same generator, seed).

cl_contig_targets for three target sets -- 10 000 seeded targets of about 200 bp (exome-like), 100-bp tiles over the whole
contig, one whole-contig target --: call to return, the three launches by device events apart and summed, bytes returned.
Against the only other route to the same figures: cl_debug_depths with states (the per-position arrays to the host) and
numpy add.reduceat, results asserted equal on every repetition.  Same build, same process, alternating repetitions; medians
and ranges.  The ordinary step (cl_contig_run + sync) and cl_contig_depth_profile(1001, 0) of the same run beside them.

    python tools/target_stats_bench.py [--length 46709983] [--depth 30] [--reps 5] [--out FILE] [--ab-lines FILE]

--ab-lines: the lines tools/ab_trees.sh wrote with AB_LINES (bench.py --gpus 1, parent against this tree); their ranges go
into the same JSON as "headline".
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

THR = (1, 10, 20, 30)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def by_reduceat(raw, qc, state, s, e, thr):
    """the figures of the targets [s, e) (ascending, disjoint, non-empty, inside the arrays) out of the per-position arrays"""
    idx = np.empty(2 * len(s), np.int64)
    idx[0::2] = s; idx[1::2] = e
    last = idx[-1] == len(raw)                                       # (reduceat takes no index at the end of the array)
    if last:
        idx = idx[:-1]

    def red(a):
        r = np.add.reduceat(a, idx)[0::2]
        return r
    out = {"sum_raw": red(raw.astype(np.uint64)), "sum_qc": red(qc.astype(np.uint64))}
    out["state"] = np.stack([red((state == k).astype(np.uint32)) for k in range(6)], axis=1)
    out["ge_raw"] = np.stack([red((raw >= t).astype(np.uint32)) for t in thr], axis=1)
    out["ge_qc"] = np.stack([red((qc >= t).astype(np.uint32)) for t in thr], axis=1)
    return out


def headline(path):
    sides = {"other": [], "this": []}
    for line in open(path):
        side, _, js = line.split(" ", 2)
        sides[side].append(json.loads(js))
    return {"what": "bench.py --gpus 1 --steps 40 --warmup 5, alternating rounds on one box (tools/ab_trees.sh); other = the parent commit",
            **{("parent" if k == "other" else "this_tree"): {"bases_per_s": spread([d["value"] for d in v]),
                                                              "ms_per_step": spread([d["ms_per_step"] for d in v if d.get("ms_per_step") is not None] or [0.0])}
               for k, v in sides.items() if v}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=46_709_983)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_target_stats.json"))
    ap.add_argument("--ab-lines", default=None)
    a = ap.parse_args()
    L = a.length
    seed = synth.seed_for(2, 20)
    rec = synth.short_read_contig(L, a.depth, seed)
    ref = synth.make_reference(L, seed)
    opt = CallableOptions()
    tmpd = tempfile.mkdtemp()
    out = {"workload": f"synthetic chr21-shaped contig, {L} bp, {a.depth}x, {rec.n} reads (bench.py's generator and seed), resident on one GPU",
           "reps": a.reps, "thresholds": list(THR)}

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
    eng.contig_collect()                                             # (the targets read the intervals of a collected run)

    rng = np.random.default_rng(25)
    s_ex = np.sort(rng.choice(extent // 4000, 10_000, replace=False)).astype(np.int64) * 4000 + rng.integers(0, 3000, 10_000)
    e_ex = s_ex + rng.integers(120, 280, 10_000)
    s_ti = np.arange(0, extent, 100, dtype=np.int64)
    e_ti = np.minimum(s_ti + 100, extent)
    cases = {"exome_like_10k": (s_ex, e_ex), "tiles_100bp": (s_ti, e_ti), "whole_contig": (np.array([0]), np.array([extent]))}

    raw = np.zeros(extent, np.uint32); qc = np.zeros(extent, np.uint32); state = np.zeros(extent, np.uint8)
    wall = {k: [] for k in cases}; kern = {k: [] for k in cases}; parts = {k: [] for k in cases}
    prof_ms, d_copy, d_np = [], [], {k: [] for k in cases}
    got = {}
    for k, (s, e) in cases.items():                                  # (the buffers' first allocation is not what is measured)
        eng.target_stats(s, e, THR)
    eng.depth_profile(1001, 0)
    for _ in range(a.reps):
        for k, (s, e) in cases.items():
            t0 = time.perf_counter()
            r = eng.target_stats(s, e, THR)
            wall[k].append((time.perf_counter() - t0) * 1e3)
            kern[k].append(r.kernel_ms); parts[k].append(r.launch_ms)
            got[k] = r
        prof_ms.append(eng.depth_profile(1001, 0).kernel_ms)
        t0 = time.perf_counter()
        st = eng._lib.cl_debug_depths(eng._h, raw.ctypes.data_as(C.c_void_p), qc.ctypes.data_as(C.c_void_p), None,
                                      state.ctypes.data_as(C.c_void_p), extent)
        assert st == 0
        d_copy.append((time.perf_counter() - t0) * 1e3)
        eng.contig_collect()                                         # (the dump re-ran the contig)
        for k, (s, e) in cases.items():
            t0 = time.perf_counter()
            exp = by_reduceat(raw, qc, state, s, e, THR)
            d_np[k].append((time.perf_counter() - t0) * 1e3)
            for f, v in exp.items():
                assert np.array_equal(np.asarray(getattr(got[k], f), np.uint64), v.astype(np.uint64)), (k, f)
            assert np.array_equal(got[k].len, (e - s).astype(np.uint32)), k
    out["depth_profile_1001_0_kernel_ms"] = spread(prof_ms)
    for k, (s, e) in cases.items():
        med = [statistics.median([p[i] for p in parts[k]]) for i in range(3)]
        out[k] = {"n_targets": int(len(s)), "mean_length": float((e - s).mean()),
                  "call_to_return_ms": spread(wall[k]), "kernel_ms_by_events": spread(kern[k]),
                  "k_target_depth_ms": spread([p[0] for p in parts[k]]), "k_target_scan_ms": spread([p[1] for p in parts[k]]),
                  "k_target_finish_ms": spread([p[2] for p in parts[k]]),
                  "bytes_returned": int(got[k].records().nbytes),
                  "k_target_depth_over_k_depth_profile": med[0] / statistics.median(prof_ms),
                  "kernel_over_ordinary_step": statistics.median(kern[k]) / out["ordinary_step"]["kernels_ms_by_events"],
                  "debug_route": {"measured_against": "cl_debug_depths (raw, qc, state) + numpy add.reduceat, same process, alternating, results asserted equal",
                                  "cl_debug_depths_ms": spread(d_copy), "numpy_ms": spread(d_np[k]),
                                  "total_ms": spread([x + y for x, y in zip(d_copy, d_np[k])]), "bytes_to_host": int(9 * extent)}}
    out["tiles_over_exome_like_kernel"] = out["tiles_100bp"]["kernel_ms_by_events"]["median"] / out["exome_like_10k"]["kernel_ms_by_events"]["median"]
    eng.close()
    if a.ab_lines and os.path.exists(a.ab_lines):
        out["headline"] = headline(a.ab_lines)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
