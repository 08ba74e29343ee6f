#!/usr/bin/env python3
"""What the dense site scan (cl_site_scan) costs on one GPU, on the config-5 input of bench.py (chrY-shaped, 40x, 150-bp
reads with bases, same generator and seed), tile resident (cl_site_upload).

  1. cl_site_scan over the whole contig: kernel by device events and call to return.
  2. The route without it, on the same resident tile of the same build, over a prefix of the contig both routes cover:
     cl_site_run with a site at every position of the prefix, dut_call_sites on the histogram and the comparison of the
     calls with the reference on the host -- against cl_site_scan of the same prefix.  Alternating repetitions, medians
     and ranges; the two routes must find the same variants.

    python tools/variant_scan_bench.py [--length 57227415] [--prefix 4000000] [--reps 5] [--out FILE]

The flagship benchmark beside it (bench.py --gpus 1 on the parent commit and on this one, alternating) is run with
tools/ab_trees.sh on a built checkout of the parent; --bench-note FILE merges its figures (a JSON object) into the output."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from decodingustools_amd import CallableOptions, Engine, _lib, synth  # noqa: E402

SNP_CALL = np.dtype([("position", np.uint32), ("depth", np.uint32), ("freq", np.float64), ("base", "S1"), ("pad", "V7")])


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def old_route(eng, lib, sites, ref, min_quality, min_depth):
    """cl_site_run at every position, dut_call_sites, the called bases against the reference: (variant positions, stage seconds)."""
    t0 = time.perf_counter()
    hist = eng.site_run(min_quality, sites)
    t1 = time.perf_counter()
    cp, n = C.c_void_p(), C.c_size_t()
    st = lib.dut_call_sites(sites.ctypes.data, None, hist.ctypes.data, sites.shape[0], min_depth, C.byref(cp), C.byref(n))
    assert st == 0
    try:
        calls = np.frombuffer(C.string_at(cp.value, n.value * SNP_CALL.itemsize), SNP_CALL) if n.value else np.zeros(0, SNP_CALL)
    finally:
        lib.dut_free(cp)
    t2 = time.perf_counter()
    base = calls["base"].view(np.uint8)
    rb = ref[calls["position"] - 1] & np.uint8(0xDF)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    var = np.isin(base, acgt) & np.isin(rb, acgt) & (base != rb)
    pos = calls["position"][var]
    t3 = time.perf_counter()
    return pos, {"site_run_s": t1 - t0, "call_sites_s": t2 - t1, "compare_s": t3 - t2, "hist_bytes": int(hist.nbytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=57_227_415)
    ap.add_argument("--prefix", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-depth", type=int, default=10)
    ap.add_argument("--min-quality", type=int, default=20)
    ap.add_argument("--bench-note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_variant_scan.json"))
    a = ap.parse_args()
    assert SNP_CALL.itemsize == C.sizeof(_lib.dut_snp_call)
    L = a.length
    P = min(a.prefix, L)
    seed = synth.seed_for(5, 23)
    t0 = time.perf_counter()
    ref = synth.make_reference(L, seed)
    rec = synth.short_read_contig(L, 40, seed, with_seq=True, ref=ref, max_live_assert=0)
    # the sample differs from the reference it is scanned against at one position in 1000 (the reads follow `ref`)
    rng = np.random.default_rng(7)
    scan_ref = ref.copy()
    planted = rng.choice(L, L // 1000, replace=False)
    scan_ref[planted] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, planted.shape[0])]
    gen = time.perf_counter() - t0
    lib = _lib.load()
    out = {"workload": f"synthetic chrY-shaped contig, {L} bp, 40x, {rec.n} reads with bases (bench.py's config-5 generator and seed), "
                       f"tile resident on one GPU; scanned against a reference with {planted.shape[0]} substitutions",
           "generate_s": gen, "reps": a.reps, "min_depth": a.min_depth, "min_quality": a.min_quality, "prefix": P}
    sites = np.arange(1, P + 1, dtype=np.uint32)
    with Engine(CallableOptions(), 0) as eng:
        t0 = time.perf_counter()
        eng.site_upload(L, L, rec)
        out["site_upload_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        first = eng.site_scan(a.min_quality, a.min_depth, scan_ref)              # builds the per-window read index as well
        out["first_scan_s"] = time.perf_counter() - t0
        whole_call, whole_kernel, pre_scan, pre_scan_kernel, pre_old, stages = [], [], [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = eng.site_scan(a.min_quality, a.min_depth, scan_ref)
            whole_call.append((time.perf_counter() - t0) * 1e3)
            ms, nbytes = eng.site_scan_stats()
            whole_kernel.append(ms)
            t0 = time.perf_counter()
            old_pos, st = old_route(eng, lib, sites, scan_ref, a.min_quality, a.min_depth)
            pre_old.append((time.perf_counter() - t0) * 1e3)
            stages.append(st)
            t0 = time.perf_counter()
            pres = eng.site_scan(a.min_quality, a.min_depth, scan_ref, 0, P)
            pre_scan.append((time.perf_counter() - t0) * 1e3)
            pre_scan_kernel.append(eng.site_scan_stats()[0])
            assert np.array_equal(pres.candidates["pos"], old_pos), "the two routes disagree"
        assert res.variant == first.variant
        out["whole_contig"] = {"call_ms": spread(whole_call), "kernel_ms": spread(whole_kernel), "algorithmic_bytes": int(nbytes),
                               "classes": {"low_depth": res.low_depth, "mixed": res.mixed, "uncomparable": res.uncomparable,
                                           "match": res.match, "variant": res.variant},
                               "candidate_bytes": int(res.variant) * 28, "reference_bytes_in": L}
        out["prefix_scan"] = {"call_ms": spread(pre_scan), "kernel_ms": spread(pre_scan_kernel), "variants": int(pres.variant)}
        out["prefix_existing_route"] = {"call_ms": spread(pre_old), "variants": int(old_pos.shape[0]),
                                        "stages_median_ms": {k: statistics.median(s[k] for s in stages) * 1e3 for k in
                                                             ("site_run_s", "call_sites_s", "compare_s")},
                                        "histogram_bytes_to_host": stages[0]["hist_bytes"]}
        out["prefix_ratio_existing_over_scan"] = out["prefix_existing_route"]["call_ms"]["median"] / out["prefix_scan"]["call_ms"]["median"]
    if a.bench_note:
        out.update(json.load(open(a.bench_note)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("whole_contig", "prefix_scan", "prefix_existing_route", "prefix_ratio_existing_over_scan")}))


if __name__ == "__main__":
    main()
