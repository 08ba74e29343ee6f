#!/usr/bin/env python3
"""What the per-target order statistics cost on one GPU, on the chr21-shaped 30x resident contig of bench.py (same generator,
seed).

cl_contig_target_order for three target sets -- 10 000 seeded targets of about 200 bp (exome-like), 100-bp tiles over the
whole contig, one whole-contig target --: bit rounds, pieces, all launches by device events, call to return, bytes returned.
Beside them, of the same run, cl_contig_targets and cl_contig_depth_profile(1001, 0) as yardsticks.  Against the only other
route to the same figures: cl_debug_depths (the per-position arrays to the host) and numpy order statistics, results
asserted equal on every repetition.  Same build, same process, alternating repetitions; medians and ranges.

    python tools/target_order_bench.py [--length 46709983] [--depth 30] [--reps 5] [--out FILE] [--ab-lines FILE]

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
T = 2048


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def ranks(length):
    return np.stack([np.zeros_like(length)] + [(j * length + 3) // 4 - 1 for j in (1, 2, 3)] + [length - 1], axis=1)


def by_numpy(d, s, e):
    """min, q1, median, q3, max of d over the targets [s, e) (non-empty, inside the array): targets of one length as the
    rows of one sorted matrix, the others one by one"""
    length = e - s
    out = np.zeros((len(s), 5), np.uint32)
    r = ranks(length)
    if len(s) > 1 and (length == length[0]).all() and (s[1:] == e[:-1]).all():
        m = np.sort(d[s[0]:e[-1]].reshape(len(s), int(length[0])), axis=1)
        return np.take_along_axis(m, r, axis=1).astype(np.uint32)
    for i in range(len(s)):
        out[i] = np.partition(d[s[i]:e[i]], np.unique(r[i]))[r[i]]
    return out


def pieces(s, e):
    return int(((e - 1) // T - s // T + 1)[e > s].sum())


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_target_order.json"))
    ap.add_argument("--ab-lines", default=None)
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

    rng = np.random.default_rng(25)
    s_ex = np.sort(rng.choice(extent // 4000, 10_000, replace=False)).astype(np.int64) * 4000 + rng.integers(0, 3000, 10_000)
    e_ex = s_ex + rng.integers(120, 280, 10_000)
    s_ti = np.arange(0, extent - extent % 100, 100, dtype=np.int64)   # (whole tiles: the host route sorts them as one matrix)
    e_ti = s_ti + 100
    cases = {"exome_like_10k": (s_ex, e_ex), "tiles_100bp": (s_ti, e_ti), "whole_contig": (np.array([0]), np.array([extent]))}

    raw = np.zeros(extent, np.uint32); qc = np.zeros(extent, np.uint32)
    wall = {k: [] for k in cases}; kern = {k: [] for k in cases}; tg_kern = {k: [] for k in cases}
    prof_ms, d_copy, d_np = [], [], {k: [] for k in cases}
    got = {}
    for k, (s, e) in cases.items():                                  # (the buffers' first allocation is not what is measured)
        eng.target_order(s, e)
        eng.target_stats(s, e, THR)
    eng.depth_profile(1001, 0)
    for _ in range(a.reps):
        for k, (s, e) in cases.items():
            t0 = time.perf_counter()
            r = eng.target_order(s, e)
            wall[k].append((time.perf_counter() - t0) * 1e3)
            kern[k].append(r.kernel_ms)
            got[k] = r
            tg_kern[k].append(eng.target_stats(s, e, THR).kernel_ms)
        prof_ms.append(eng.depth_profile(1001, 0).kernel_ms)
        t0 = time.perf_counter()
        st = eng._lib.cl_debug_depths(eng._h, raw.ctypes.data_as(C.c_void_p), qc.ctypes.data_as(C.c_void_p), None, None, extent)
        assert st == 0
        d_copy.append((time.perf_counter() - t0) * 1e3)
        eng.contig_collect()                                         # (the dump re-ran the contig)
        for k, (s, e) in cases.items():
            t0 = time.perf_counter()
            exp_raw, exp_qc = by_numpy(raw, s, e), by_numpy(qc, s, e)
            d_np[k].append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(got[k].raw, exp_raw) and np.array_equal(got[k].qc, exp_qc), k
            assert np.array_equal(got[k].len, (e - s).astype(np.uint32)), k
    out["depth_profile_1001_0_kernel_ms"] = spread(prof_ms)
    for k, (s, e) in cases.items():
        out[k] = {"n_targets": int(len(s)), "mean_length": float((e - s).mean()), "rounds": int(got[k].n_rounds), "pieces": pieces(s, e),
                  "largest_raw_depth": int(got[k].raw[:, 4].max()),
                  "call_to_return_ms": spread(wall[k]), "kernel_ms_by_events": spread(kern[k]),
                  "bytes_returned": int(got[k].records().nbytes),
                  "cl_contig_targets_kernel_ms": spread(tg_kern[k]),
                  "kernel_over_cl_contig_targets": statistics.median(kern[k]) / statistics.median(tg_kern[k]),
                  "kernel_over_k_depth_profile": statistics.median(kern[k]) / statistics.median(prof_ms),
                  "debug_route": {"measured_against": "cl_debug_depths (raw, qc) + numpy sort / partition per target, same process, alternating, results asserted equal",
                                  "cl_debug_depths_ms": spread(d_copy), "numpy_ms": spread(d_np[k]),
                                  "total_ms": spread([x + y for x, y in zip(d_copy, d_np[k])]), "bytes_to_host": int(8 * extent)}}
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
