#!/usr/bin/env python3
"""What the minor-allele scan (cl_site_scan_minor) costs on one GPU, and what it leaves alone, on the config-5 tile of
bench.py that tools/filtered_scan_bench.py uses (same generator, seed, flags and quality mix), tile resident, attachment on.

Per repetition, alternating in one process on the same resident tile:
  cl_site_scan and cl_site_scan_ex of the parent commit's library (--parent-lib FILE)     the shared counting phase, before
  cl_site_scan and cl_site_scan_ex of this build                                          ... and after
  cl_site_scan_minor, unfiltered and filtered, whole contig
  the route without the feature: cl_site_scan_counts_ex over the first 4 Mb in pieces of 2^20 positions (36 bytes per
  position to the host) and the numpy rule of tests/minor_ref.py over them
Equal candidate lists are asserted on every repetition: the two libraries' variants, the minor scan's two calls against
the first one, and the filtered minor scan's candidates below 4 Mb against the numpy route's.

    python tools/minor_scan_bench.py --parent-lib FILE [--length 57227415] [--reps 7] [--bench-note FILE] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import minor_ref as M  # noqa: E402
from filtered_scan_bench import OtherLib, spread  # noqa: E402
from decodingustools_amd import CallableOptions, Engine, synth  # noqa: E402
from decodingustools_amd._lib import CL_SCAN_MAX_DENSE  # noqa: E402

ROUTE_LEN = 4 << 20


def numpy_route(eng, mq, ex, md, cnt, per, end):
    """(positions 1-based, major, minor, c2, depth of the candidates of [0, end), seconds in the engine, seconds in numpy)."""
    t_dev = t_np = 0.0
    out = []
    for a in range(0, end, CL_SCAN_MAX_DENSE):
        b = min(end, a + CL_SCAN_MAX_DENSE)
        t0 = time.perf_counter()
        c9 = eng.site_scan_counts_ex(mq, a, b, ex, True)
        t1 = time.perf_counter()
        acgt = c9[:, 0:8:2].astype(np.int64) + c9[:, 1:8:2]
        cls, mi, ni = M.classify_arrays(acgt, c9[:, 8], md, cnt, per)
        hit = np.nonzero(cls == M.MINOR)[0]
        out.append(np.stack([hit + a + 1, mi[hit], ni[hit], acgt[hit, ni[hit]], c9[hit, 8].astype(np.int64)], 1))
        t_dev += t1 - t0
        t_np += time.perf_counter() - t1
    return np.concatenate(out), t_dev, t_np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=57_227_415)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-depth", type=int, default=10)
    ap.add_argument("--min-quality", type=int, default=20)
    ap.add_argument("--min-base-quality", type=int, default=20)
    ap.add_argument("--exclude-flags", type=lambda s: int(s, 0), default=0x704)
    ap.add_argument("--min-minor-count", type=int, default=3)
    ap.add_argument("--min-minor-per-10k", type=int, default=500)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_minor_scan.json"))
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
    mq, md, ex, cnt, per = a.min_quality, a.min_depth, a.exclude_flags, a.min_minor_count, a.min_minor_per_10k
    route_end = min(L, ROUTE_LEN)
    out = {"workload": f"synthetic chrY-shaped contig, {L} bp, 40x, {rec.n} reads with bases (bench.py's config-5 generator and seed, "
                       f"0x10 on a seeded half of the reads, quality mix 2/12/23/37), tile resident on one GPU, attachment at base quality "
                       f">= {a.min_base_quality}; filter: exclude 0x{ex:04x}; minor rule: min_depth {md}, count >= {cnt}, {per} per 10 000",
           "generate_s": gen, "reps": a.reps, "min_depth": md, "min_quality": mq, "route_without_positions": route_end}
    T = {k: {"call_ms": [], "kernel_ms": []} for k in ("scan", "scan_ex", "parent_scan", "parent_scan_ex", "minor", "minor_filtered")}
    route = {"total_ms": [], "engine_ms": [], "numpy_ms": []}

    def timed(key, fn):
        t0 = time.perf_counter()
        r = fn()
        T[key]["call_ms"].append((time.perf_counter() - t0) * 1e3)
        T[key]["kernel_ms"].append(eng.site_scan_stats()[0])
        return r

    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, a.min_base_quality)
        first = eng.site_scan(mq, md, scan_ref)                                    # builds the per-window read index as well
        first_f = eng.site_scan_ex(mq, md, scan_ref, ex, True)
        first_m = eng.site_scan_minor(mq, md, cnt, per, scan_ref)
        first_mf = eng.site_scan_minor(mq, md, cnt, per, scan_ref, filter=(ex, True))
        other = OtherLib(a.parent_lib, rec, L) if a.parent_lib else None
        if other:
            assert other.filtered, "the parent library has no cl_site_scan_ex"
            other.attach(rec, a.min_base_quality)
            assert other.scan(mq, md, scan_ref)[2] == first.variant and other.scan(mq, md, scan_ref, ex)[2] == first_f.variant
        for _ in range(a.reps):
            if other:
                for key, flt in (("parent_scan", None), ("parent_scan_ex", ex)):
                    c, k, nv = other.scan(mq, md, scan_ref, flt)
                    T[key]["call_ms"].append(c); T[key]["kernel_ms"].append(k)
                    assert nv == (first.variant if flt is None else first_f.variant)
            u = timed("scan", lambda: eng.site_scan(mq, md, scan_ref))
            f = timed("scan_ex", lambda: eng.site_scan_ex(mq, md, scan_ref, ex, True))
            m = timed("minor", lambda: eng.site_scan_minor(mq, md, cnt, per, scan_ref))
            mf = timed("minor_filtered", lambda: eng.site_scan_minor(mq, md, cnt, per, scan_ref, filter=(ex, True)))
            assert np.array_equal(u.candidates, first.candidates) and np.array_equal(f.candidates, first_f.candidates)
            assert np.array_equal(m.candidates, first_m.candidates) and np.array_equal(mf.candidates, first_mf.candidates)
            t0 = time.perf_counter()
            got, t_dev, t_np = numpy_route(eng, mq, ex, md, cnt, per, route_end)
            route["total_ms"].append((time.perf_counter() - t0) * 1e3); route["engine_ms"].append(t_dev * 1e3); route["numpy_ms"].append(t_np * 1e3)
            c = mf.candidates[mf.candidates["pos"] <= route_end]
            acgt = np.stack([c["a"], c["c"], c["g"], c["t"]], 1).astype(np.int64)
            idx = {ord(ch): i for i, ch in enumerate("ACGT")}
            ni = np.array([idx[x] for x in c["minor"]], np.int64)
            mine = np.stack([c["pos"].astype(np.int64), np.array([idx[x] for x in c["major"]], np.int64), ni,
                             acgt[np.arange(c.shape[0]), ni], c["depth"].astype(np.int64)], 1)
            assert np.array_equal(mine, got), "the minor scan and the numpy route disagree"
        if other:
            other.close()
    for k, v in T.items():
        if v["call_ms"]:
            out[k] = {"call_ms": spread(v["call_ms"]), "kernel_ms": spread(v["kernel_ms"])}
    out["scan"]["variants"] = int(first.variant); out["scan_ex"]["variants"] = int(first_f.variant)
    for k, r in (("minor", first_m), ("minor_filtered", first_mf)):
        out[k]["classes"] = {"low_depth": r.low_depth, "single": r.single, "minor": r.minor}
    out["route_without"] = {k: spread(v) for k, v in route.items()}
    out["route_without"]["candidates"] = int(got.shape[0])
    # the new scan's kernel against cl_site_scan_ex of the same run; the whole-contig call against the route without the
    # feature scaled from its 4 Mb to the contig
    out["kernel_ratio_minor_filtered_over_scan_ex"] = out["minor_filtered"]["kernel_ms"]["median"] / out["scan_ex"]["kernel_ms"]["median"]
    out["kernel_ratio_minor_over_scan"] = out["minor"]["kernel_ms"]["median"] / out["scan"]["kernel_ms"]["median"]
    per_pos = out["route_without"]["total_ms"]["median"] / route_end
    out["speedup_over_route_without"] = per_pos * L / out["minor_filtered"]["call_ms"]["median"]
    out["speedup_over_route_without_same_range_note"] = "route: median ms per position over its positions, times the contig's length, over the median whole-contig call of the filtered minor scan"
    if a.parent_lib:
        out["parent_library"] = os.path.basename(a.parent_lib)
        # the gate of a change that must cost the existing scans nothing: this build's median within the parent's own range
        out["median_within_parent_max"] = {f"{form}_{q}": bool(out[form][q]["median"] <= out[f"parent_{form}"][q]["max"])
                                           for form in ("scan", "scan_ex") for q in ("kernel_ms", "call_ms")}
    if a.bench_note:
        out.update(json.load(open(a.bench_note)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("workload",)}))


if __name__ == "__main__":
    main()
