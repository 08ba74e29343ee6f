#!/usr/bin/env python3
"""What the deletion scan (cl_site_scan_dels) costs on one GPU, and what it leaves alone, on the config-5 tile of bench.py
that tools/minor_scan_bench.py uses (same generator, seed, flags and quality mix), tile resident, attachment on.

Per repetition, alternating in one process on the same resident tile:
  cl_site_scan, cl_site_scan_ex and cl_site_scan_minor of the parent commit's library (--parent-lib FILE)
  the same three of this build
  cl_site_scan_dels, unfiltered and filtered, whole contig, at (min_depth, min_del_count, min_del_per_10k)
Kernel time by events and call to return, medians and ranges.  Equal results are asserted on every repetition: the two
libraries' variant and minor counts, every call's candidate list against the first one's.  The launches of a deletion scan
are counted from its candidates: one, and one more when they exceed the first buffer of max(65 536, positions / 64) entries.

    python tools/del_scan_bench.py --parent-lib FILE [--length 57227415] [--reps 7] [--bench-note FILE] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from filtered_scan_bench import OtherLib, spread  # noqa: E402
from decodingustools_amd import CallableOptions, Engine, _lib, synth, variants as V  # noqa: E402


def other_minor(other, mq, md, cnt, per, ref, exclude_flags):
    """(call ms, kernel ms, minor positions) of the other library's filtered cl_site_scan_minor."""
    fn = other.lib.cl_site_scan_minor
    fn.argtypes = [C.c_void_p, C.c_uint8, C.POINTER(_lib.cl_scan_filter), C.POINTER(_lib.cl_minor_params), C.c_void_p, C.c_uint64, C.c_uint32,
                   C.c_uint32, C.POINTER(_lib.cl_minor_result)]
    r = _lib.cl_minor_result()
    f = _lib.cl_scan_filter(exclude_flags, 1, 0)
    prm = _lib.cl_minor_params(md, cnt, per)
    t0 = time.perf_counter()
    assert fn(other.h, mq, C.byref(f), C.byref(prm), ref.ctypes.data, ref.shape[0], 0, ref.shape[0], C.byref(r)) == 0
    call = (time.perf_counter() - t0) * 1e3
    ms = C.c_double(); b = C.c_uint64()
    other.lib.cl_site_scan_stats(other.h, C.byref(ms), C.byref(b))
    return call, ms.value, int(r.n_minor)


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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_del_scan.json"))
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
    mcnt, mper = 3, 500                                                   # the minor scan's default rule
    out = {"workload": f"synthetic chrY-shaped contig, {L} bp, 40x, {rec.n} reads with bases (bench.py's config-5 generator and seed, "
                       f"0x10 on a seeded half of the reads, quality mix 2/12/23/37), tile resident on one GPU, attachment at base quality "
                       f">= {a.min_base_quality}; filter: exclude 0x{ex:04x}; deletion rule: min_depth {md}, count >= {cnt}, {per} per 10 000",
           "generate_s": gen, "reps": a.reps, "min_depth": md, "min_quality": mq}
    keys = ("scan", "scan_ex", "minor_filtered", "parent_scan", "parent_scan_ex", "parent_minor_filtered", "dels", "dels_filtered", "dels_every", "dels_every_filtered")
    T = {k: {"call_ms": [], "kernel_ms": []} for k in keys}

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
        first_m = eng.site_scan_minor(mq, md, mcnt, mper, scan_ref, filter=(ex, True))
        first_d = eng.site_scan_dels(mq, md, cnt, per, scan_ref)
        first_df = eng.site_scan_dels(mq, md, cnt, per, scan_ref, filter=(ex, True))
        first_e = eng.site_scan_dels(mq, 1, 1, 1, scan_ref)                        # every position with a counted deletion
        first_ef = eng.site_scan_dels(mq, 1, 1, 1, scan_ref, filter=(ex, True))
        other = OtherLib(a.parent_lib, rec, L) if a.parent_lib else None
        if other:
            assert other.filtered and hasattr(other.lib, "cl_site_scan_minor"), "the parent library has no cl_site_scan_ex / cl_site_scan_minor"
            other.attach(rec, a.min_base_quality)
            assert other.scan(mq, md, scan_ref)[2] == first.variant and other.scan(mq, md, scan_ref, ex)[2] == first_f.variant
        for _ in range(a.reps):
            if other:
                for key, flt in (("parent_scan", None), ("parent_scan_ex", ex)):
                    c, k, nv = other.scan(mq, md, scan_ref, flt)
                    T[key]["call_ms"].append(c); T[key]["kernel_ms"].append(k)
                    assert nv == (first.variant if flt is None else first_f.variant)
                c, k, nm = other_minor(other, mq, md, mcnt, mper, scan_ref, ex)
                T["parent_minor_filtered"]["call_ms"].append(c); T["parent_minor_filtered"]["kernel_ms"].append(k)
                assert nm == first_m.minor
            u = timed("scan", lambda: eng.site_scan(mq, md, scan_ref))
            f = timed("scan_ex", lambda: eng.site_scan_ex(mq, md, scan_ref, ex, True))
            m = timed("minor_filtered", lambda: eng.site_scan_minor(mq, md, mcnt, mper, scan_ref, filter=(ex, True)))
            d = timed("dels", lambda: eng.site_scan_dels(mq, md, cnt, per, scan_ref))
            df = timed("dels_filtered", lambda: eng.site_scan_dels(mq, md, cnt, per, scan_ref, filter=(ex, True)))
            e = timed("dels_every", lambda: eng.site_scan_dels(mq, 1, 1, 1, scan_ref))
            ef = timed("dels_every_filtered", lambda: eng.site_scan_dels(mq, 1, 1, 1, scan_ref, filter=(ex, True)))
            assert np.array_equal(u.candidates, first.candidates) and np.array_equal(f.candidates, first_f.candidates)
            assert np.array_equal(m.candidates, first_m.candidates)
            assert np.array_equal(d.candidates, first_d.candidates) and np.array_equal(df.candidates, first_df.candidates)
            assert np.array_equal(e.candidates, first_e.candidates) and np.array_equal(ef.candidates, first_ef.candidates)
        if other:
            other.close()
    for k, v in T.items():
        if v["call_ms"]:
            out[k] = {"call_ms": spread(v["call_ms"]), "kernel_ms": spread(v["kernel_ms"])}
    out["scan"]["variants"] = int(first.variant); out["scan_ex"]["variants"] = int(first_f.variant); out["minor_filtered"]["minor"] = int(first_m.minor)
    first_buffer = max(65536, L // 64)
    for k, r in (("dels", first_d), ("dels_filtered", first_df), ("dels_every", first_e), ("dels_every_filtered", first_ef)):
        out[k]["classes"] = {"low_depth": r.low_depth, "kept": r.kept, "deleted": r.deleted}
        out[k]["events"] = len(V.del_events(r.candidates))
        out[k]["launches_per_call"] = 1 if r.deleted <= first_buffer else 2
    out["dels_every"]["rule"] = out["dels_every_filtered"]["rule"] = "min_depth 1, count >= 1, 1 per 10 000: every position with a counted deletion"
    # the new scan's kernel against the calling scan's of the same run, form by form
    out["kernel_ratio_dels_over_scan"] = out["dels"]["kernel_ms"]["median"] / out["scan"]["kernel_ms"]["median"]
    out["kernel_ratio_dels_filtered_over_scan_ex"] = out["dels_filtered"]["kernel_ms"]["median"] / out["scan_ex"]["kernel_ms"]["median"]
    if a.parent_lib:
        out["parent_library"] = os.path.basename(a.parent_lib)
        # the gate of a change that must cost the existing scans nothing: this build's median within the parent's own range
        out["median_within_parent_max"] = {f"{form}_{q}": bool(out[form][q]["median"] <= out[f"parent_{form}"][q]["max"])
                                           for form in ("scan", "scan_ex", "minor_filtered") for q in ("kernel_ms", "call_ms")}
    if a.bench_note:
        out.update(json.load(open(a.bench_note)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("workload",)}))


if __name__ == "__main__":
    main()
