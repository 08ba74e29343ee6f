#!/usr/bin/env python3
"""fingerprint-compare on one GPU against the host route.

Seeded synthetic sketches of the whole-genome shape (64 sketches of about 3 M entries out of one universe of 4.5 M hashes, so
any two share about half their union), resident in one SketchSet.  Medians and ranges of five alternating repetitions of
  1. all 2 016 pairs, the device time from events (k_fpc_tiles + k_fpc_sum),
  2. all 2 016 pairs, call to return,
  3. one against 63 (a query), call to return and by events,
  4. dut_fpc_compare_host on the query's 63 pairs: on the process's threads here, on one thread in a child process
     (DUT_THREADS is read once per process),
with the records asserted equal on every repetition (device against device, and against the host route on the query and,
once, on all pairs).  Also: the time to add the set, the bytes the pairs span (sum of 12 (n_a + n_b)), those bytes over the
kernel time beside the HBM peak, and tools/isa_stats.py's figures of the three kernels.

    python tools/fingerprint_compare_bench.py [--sketches 64] [--entries 3000000] [--reps 5] [--out profiles/r29_fingerprint_compare.json]
                                              [--ab-lines FILE]     # "<side> <round> <json>" lines of tools/ab_trees.sh (AB_LINES=FILE)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from decodingustools_amd import build as _b  # noqa: E402
from decodingustools_amd import fingerprint as fpm  # noqa: E402

HBM_PEAK_TBS = 8.0          # spec; about 6.3 TB/s is achievable by streaming reads
K, SCALED = 31, 1000


def make_sketches(n, entries, seed):
    rng = np.random.default_rng(seed)
    top = fpm.max_hash(SCALED)
    uni = np.unique(rng.integers(0, top, size=entries + entries // 2, dtype=np.uint64, endpoint=True))
    out = []
    for _ in range(n):
        h = uni[rng.random(uni.size) < entries / uni.size]
        out.append((h, rng.integers(1, 60, size=h.size, dtype=np.uint32), K, SCALED))
    return out


def spread(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "all": [round(x, digits) for x in v]}


def host_query_ms(sk, pairs, reps):
    ms, rec = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fpm.compare_host(sk, pairs).records()
        ms.append((time.perf_counter() - t0) * 1e3)
        assert rec is None or np.array_equal(rec, r)
        rec = r
    return ms, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=64)
    ap.add_argument("--entries", type=int, default=3_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=29)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_fingerprint_compare.json"))
    ap.add_argument("--ab-lines", default=None)
    ap.add_argument("--host-child", action="store_true", help="internal: the one-thread host run, JSON on stdout")
    a = ap.parse_args()
    _b.build()
    sk = make_sketches(a.sketches, a.entries, a.seed)
    query = [(0, j) for j in range(1, a.sketches)]
    if a.host_child:
        ms, rec = host_query_ms(sk, query, a.reps)
        print(json.dumps({"ms": ms, "sum": int(rec.sum(dtype=np.uint64))}))
        return
    allp = [(i, j) for i in range(a.sketches) for j in range(i + 1, a.sketches)]
    res = {"sketches": a.sketches, "entries_mean": int(np.mean([len(s[0]) for s in sk])), "pairs": len(allp), "ksize": K, "scaled": SCALED,
           "tile": fpm.tile_size(), "threads": int(os.environ.get("DUT_THREADS") or 0) or "process default"}
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--host-child", "--sketches", str(a.sketches), "--entries", str(a.entries),
                              "--reps", str(a.reps), "--seed", str(a.seed)], stdout=subprocess.PIPE, text=True, env=dict(os.environ, DUT_THREADS="1"))
    child_out = child.communicate()[0]                      # before the device is timed: the two do not share the CPUs
    assert child.returncode == 0
    one = json.loads(child_out.strip().splitlines()[-1])
    with fpm.SketchSet() as s:
        t0 = time.perf_counter()
        for x in sk:
            s.add(*x)
        res["add_set_s"] = round(time.perf_counter() - t0, 3)
        s.compare_all(), s.compare(query)                   # warm-up: code objects, the tables' buffers
        ev_all, wall_all, ev_q, wall_q, host_thr = [], [], [], [], []
        rec_all = rec_q = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = s.compare_all()
            wall_all.append((time.perf_counter() - t0) * 1e3)
            ev_all.append(r.kernel_ms)
            assert rec_all is None or np.array_equal(rec_all, r.records())
            rec_all, tiles, nbytes = r.records(), r.n_tiles, r.bytes
            t0 = time.perf_counter()
            q = s.compare(query)
            wall_q.append((time.perf_counter() - t0) * 1e3)
            ev_q.append(q.kernel_ms)
            assert rec_q is None or np.array_equal(rec_q, q.records())
            rec_q, q_bytes = q.records(), q.bytes
            ms, hrec = host_query_ms(sk, query, 1)
            host_thr += ms
            assert np.array_equal(hrec, rec_q)
        assert np.array_equal(rec_q, rec_all[:a.sketches - 1])
    assert one["sum"] == int(rec_q.sum(dtype=np.uint64))
    t0 = time.perf_counter()
    assert np.array_equal(fpm.compare_host(sk, allp).records(), rec_all)
    res["host_all_pairs_threads_s"] = round(time.perf_counter() - t0, 3)
    res.update({"all_pairs_kernel_ms": spread(ev_all), "all_pairs_call_ms": spread(wall_all), "query_kernel_ms": spread(ev_q),
                "query_call_ms": spread(wall_q), "host_query_threads_ms": spread(host_thr), "host_query_one_thread_ms": spread(one["ms"]),
                "tiles_all_pairs": tiles, "bytes_all_pairs": nbytes, "bytes_query": q_bytes})
    tbs = nbytes / (statistics.median(ev_all) * 1e-3) / 1e12
    res["all_pairs_tb_per_s_kernel"] = round(tbs, 3)
    res["hbm_peak_tb_per_s"] = HBM_PEAK_TBS
    res["fraction_of_hbm_peak"] = round(tbs / HBM_PEAK_TBS, 3)
    res["query_tb_per_s_kernel"] = round(q_bytes / (statistics.median(ev_q) * 1e-3) / 1e12, 3)
    res["query_device_call_over_host_threads"] = round(statistics.median(host_thr) / statistics.median(wall_q), 1)
    res["query_device_call_over_host_one_thread"] = round(statistics.median(one["ms"]) / statistics.median(wall_q), 1)
    res["all_pairs_device_call_over_host_threads"] = round(res["host_all_pairs_threads_s"] * 1e3 / statistics.median(wall_all), 1)
    res["isa"] = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), "k_fpc_"], capture_output=True, text=True).stdout
    if a.ab_lines and os.path.exists(a.ab_lines):
        sides = {}
        for line in open(a.ab_lines):
            side, _, js = line.split(" ", 2)
            d = json.loads(js)
            sides.setdefault(side, []).append((d["value"], d.get("ms_per_step")))
        res["bench_py_gpus_1_ab"] = {("parent" if k == "other" else "this"): {"value": spread([v[0] for v in rows], 0),
                                                                             "ms_per_step": spread([v[1] for v in rows if v[1] is not None] or [0], 6)}
                                     for k, rows in sides.items()}
    # blocks of an earlier file that this run does not measure (comparisons with kernel forms that are no longer in the
    # tree, recorded when they were: profiles/README.md) are carried over
    if os.path.exists(a.out):
        try:
            res.update({k: v for k, v in json.load(open(a.out)).items() if k not in res})
        except ValueError:
            pass
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
