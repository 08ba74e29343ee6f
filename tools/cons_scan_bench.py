#!/usr/bin/env python3
"""What the consensus scan (cl_site_scan_consensus) costs on one GPU, what it saves and what it leaves alone, on the
config-5 tile of bench.py that tools/ins_scan_bench.py uses (same generator, seed, flags and quality mix), tile resident,
attachment on.

Per repetition, alternating in one process on the same resident tile:
  cl_site_scan, cl_site_scan_ex and the filtered cl_site_scan_dels of the parent commit's library (--parent-lib FILE)
  the same three of this build
  cl_site_scan_consensus, unfiltered and filtered, over the whole contig (one byte per position comes back)
  the route without it over the first --route-positions positions, in chunks of CL_SCAN_MAX_DENSE: cl_site_scan_counts_ex,
  cl_site_scan_dels at (min_depth, 1, 1), then the rule in numpy -- its bytes asserted equal to the consensus scan's
Kernel time by events and call to return, medians and ranges.  Equal results are asserted on every repetition.

    python tools/cons_scan_bench.py --parent-lib FILE [--length 57227415] [--reps 7] [--bench-note FILE] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from filtered_scan_bench import OtherLib, spread  # noqa: E402
from ins_scan_bench import other_dels  # noqa: E402
from decodingustools_amd import CallableOptions, Engine, _lib, synth  # noqa: E402


def numpy_rule(counts9, n_del, md, cnt, per):
    """The consensus bytes from the nine dense counters and the deletion counts of a chunk: the rule of
    cl_site_scan_consensus in whole columns, int64."""
    q = counts9[:, 0:8:2].astype(np.int64) + counts9[:, 1:8:2]
    depth = counts9[:, 8].astype(np.int64)
    span = depth + n_del
    m = q.max(1)
    base = np.frombuffer(b"ACGT", np.uint8)[q.argmax(1)]
    low1 = span < md
    gone = ~low1 & (n_del >= cnt) & (10000 * n_del >= per * span)
    low = low1 | (~gone & (depth < md))
    called = ~low & ~gone & (10 * m >= 7 * depth)
    out = np.full(depth.shape[0], ord("N"), np.uint8)
    out[called] = base[called]
    out[low] = ord("n")
    out[gone] = ord("-")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=57_227_415)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-depth", type=int, default=10)
    ap.add_argument("--min-quality", type=int, default=20)
    ap.add_argument("--min-base-quality", type=int, default=20)
    ap.add_argument("--exclude-flags", type=lambda s: int(s, 0), default=0x704)
    ap.add_argument("--min-del-count", type=int, default=3)
    ap.add_argument("--min-del-per-10k", type=int, default=7000)
    ap.add_argument("--route-positions", type=int, default=4 << 20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_consensus.json"))
    a = ap.parse_args()
    L = a.length
    seed = synth.seed_for(5, 23)
    t0 = time.perf_counter()
    ref = synth.make_reference(L, seed)
    rec = synth.short_read_contig(L, 40, seed, with_seq=True, ref=ref, max_live_assert=0)
    rec.flag = rec.flag | (np.random.default_rng(11).integers(0, 2, rec.n).astype(np.uint16) << np.uint16(4))
    rng = np.random.default_rng(7)
    scan_ref = ref.copy()
    planted = rng.choice(L, L // 1000, replace=False)
    scan_ref[planted] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, planted.shape[0])]
    gen = time.perf_counter() - t0
    mq, md, ex, cnt, per = a.min_quality, a.min_depth, a.exclude_flags, a.min_del_count, a.min_del_per_10k
    route_n = min(a.route_positions, L)
    chunk = _lib.CL_SCAN_MAX_DENSE
    out = {"workload": f"synthetic chrY-shaped contig, {L} bp, 40x, {rec.n} reads with bases (bench.py's config-5 generator and seed, "
                       f"0x10 on a seeded half of the reads, quality mix 2/12/23/37), tile resident on one GPU, attachment at base quality "
                       f">= {a.min_base_quality}; filter: exclude 0x{ex:04x}; rule: min_depth {md}, deletion count >= {cnt}, {per} per 10 000",
           "generate_s": gen, "reps": a.reps, "min_depth": md, "min_quality": mq, "route_positions": route_n}
    forms = ("scan", "scan_ex", "dels_filtered")
    cons_keys = ("consensus", "consensus_filtered")
    T = {k: {"call_ms": [], "kernel_ms": []} for k in forms + tuple("parent_" + f for f in forms) + cons_keys}
    route = {"call_ms": [], "kernel_ms": [], "counts_ms": [], "dels_ms": [], "numpy_ms": []}

    def timed(key, fn):
        t0 = time.perf_counter()
        r = fn()
        T[key]["call_ms"].append((time.perf_counter() - t0) * 1e3)
        T[key]["kernel_ms"].append(eng.site_scan_stats()[0])
        return r

    def the_route():
        """The bytes of [0, route_n) without the consensus scan, and what each part took."""
        parts = []
        t = dict(counts=0.0, dels=0.0, numpy=0.0, kernel=0.0)
        t_all = time.perf_counter()
        for s in range(0, route_n, chunk):
            e = min(s + chunk, route_n)
            t0 = time.perf_counter()
            c9 = eng.site_scan_counts_ex(mq, s, e, ex, True)
            t["counts"] += time.perf_counter() - t0; t["kernel"] += eng.site_scan_stats()[0]
            t0 = time.perf_counter()
            d = eng.site_scan_dels(mq, md, 1, 1, scan_ref, s, e, filter=(ex, True))       # every position of span >= min_depth with a deletion
            t["dels"] += time.perf_counter() - t0; t["kernel"] += eng.site_scan_stats()[0]
            t0 = time.perf_counter()
            n_del = np.zeros(e - s, np.int64)
            n_del[d.candidates["pos"].astype(np.int64) - 1 - s] = d.candidates["del"]
            parts.append(numpy_rule(c9, n_del, md, cnt, per))
            t["numpy"] += time.perf_counter() - t0
        route["call_ms"].append((time.perf_counter() - t_all) * 1e3)
        route["kernel_ms"].append(t["kernel"])
        for k in ("counts", "dels", "numpy"):
            route[k + "_ms"].append(t[k] * 1e3)
        return np.concatenate(parts)

    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, a.min_base_quality)
        first = eng.site_scan(mq, md, scan_ref)                                    # builds the per-window read index as well
        first_f = eng.site_scan_ex(mq, md, scan_ref, ex, True)
        first_d = eng.site_scan_dels(mq, md, cnt, per, scan_ref, filter=(ex, True))
        first_c = {"consensus": eng.site_scan_consensus(mq, md, cnt, per, scan_ref),
                   "consensus_filtered": eng.site_scan_consensus(mq, md, cnt, per, scan_ref, filter=(ex, True))}
        assert first_c["consensus_filtered"].deleted == first_d.deleted
        other = OtherLib(a.parent_lib, rec, L) if a.parent_lib else None
        if other:
            assert other.filtered and hasattr(other.lib, "cl_site_scan_dels"), "the parent library has no cl_site_scan_ex / cl_site_scan_dels"
            other.attach(rec, a.min_base_quality)
            assert other.scan(mq, md, scan_ref)[2] == first.variant and other.scan(mq, md, scan_ref, ex)[2] == first_f.variant
        for _ in range(a.reps):
            if other:
                for key, flt in (("parent_scan", None), ("parent_scan_ex", ex)):
                    c, k, nv = other.scan(mq, md, scan_ref, flt)
                    T[key]["call_ms"].append(c); T[key]["kernel_ms"].append(k)
                    assert nv == (first.variant if flt is None else first_f.variant)
                c, k, nd = other_dels(other, mq, md, cnt, per, scan_ref, ex)
                T["parent_dels_filtered"]["call_ms"].append(c); T["parent_dels_filtered"]["kernel_ms"].append(k)
                assert nd == first_d.deleted
            u = timed("scan", lambda: eng.site_scan(mq, md, scan_ref))
            f = timed("scan_ex", lambda: eng.site_scan_ex(mq, md, scan_ref, ex, True))
            d = timed("dels_filtered", lambda: eng.site_scan_dels(mq, md, cnt, per, scan_ref, filter=(ex, True)))
            assert np.array_equal(u.candidates, first.candidates) and np.array_equal(f.candidates, first_f.candidates)
            assert np.array_equal(d.candidates, first_d.candidates)
            r = timed("consensus", lambda: eng.site_scan_consensus(mq, md, cnt, per, scan_ref))
            assert np.array_equal(r.cons, first_c["consensus"].cons)
            r = timed("consensus_filtered", lambda: eng.site_scan_consensus(mq, md, cnt, per, scan_ref, filter=(ex, True)))
            assert np.array_equal(r.cons, first_c["consensus_filtered"].cons)
            assert np.array_equal(the_route(), r.cons[:route_n]), "the route without the consensus scan gives other bytes"
        if other:
            other.close()
    for k, v in T.items():
        if v["call_ms"]:
            out[k] = {q: spread(x) for q, x in v.items()}
    out["route_without_consensus"] = {q: spread(x) for q, x in route.items()}
    out["route_without_consensus"]["what"] = (f"first {route_n} positions in chunks of {chunk}: cl_site_scan_counts_ex, cl_site_scan_dels at "
                                              f"({md}, 1, 1) under the same filter, the rule in numpy; bytes asserted equal on every repetition")
    out["scan"]["variants"] = int(first.variant); out["scan_ex"]["variants"] = int(first_f.variant); out["dels_filtered"]["deleted"] = int(first_d.deleted)
    for k, r in first_c.items():
        out[k]["classes"] = {"low_depth": r.low_depth, "deleted": r.deleted, "no_call": r.no_call, "ref": r.ref, "alt": r.alt}
        out[k]["bytes_back"] = int(r.cons.shape[0])
    out["kernel_ratio_consensus_over_scan"] = out["consensus"]["kernel_ms"]["median"] / out["scan"]["kernel_ms"]["median"]
    out["kernel_ratio_consensus_filtered_over_scan_ex"] = out["consensus_filtered"]["kernel_ms"]["median"] / out["scan_ex"]["kernel_ms"]["median"]
    # call to return per position: the route over its positions against the filtered consensus scan over the whole contig
    out["speedup_call_per_position_over_route"] = ((out["route_without_consensus"]["call_ms"]["median"] / route_n)
                                                   / (out["consensus_filtered"]["call_ms"]["median"] / L))
    out["speedup_kernel_per_position_over_route"] = ((out["route_without_consensus"]["kernel_ms"]["median"] / route_n)
                                                     / (out["consensus_filtered"]["kernel_ms"]["median"] / L))
    if a.parent_lib:
        out["parent_library"] = os.path.basename(a.parent_lib)
        # the yardstick of a change that must cost the existing scans nothing: this build's median within the parent's own range
        out["median_within_parent_max"] = {f"{form}_{q}": bool(out[form][q]["median"] <= out[f"parent_{form}"][q]["max"])
                                           for form in forms for q in ("kernel_ms", "call_ms")}
    if a.bench_note:
        out.update(json.load(open(a.bench_note)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("workload",)}))


if __name__ == "__main__":
    main()
