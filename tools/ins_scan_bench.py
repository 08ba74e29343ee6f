#!/usr/bin/env python3
"""What the insertion scan (cl_site_scan_ins) costs on one GPU, and what it leaves alone, on the config-5 tile of bench.py
that tools/del_scan_bench.py uses (same generator, seed, flags and quality mix), tile resident, attachment on.

Per repetition, alternating in one process on the same resident tile:
  cl_site_scan, cl_site_scan_ex, cl_site_scan_minor and cl_site_scan_dels of the parent commit's library (--parent-lib FILE)
  the same four of this build
  cl_site_scan_ins, unfiltered and filtered, whole contig, at (min_depth, min_ins_count, min_ins_per_10k) and at (1, 1, 1):
  its window scan and its allele launch apart, candidates and observations counted
Kernel time by events and call to return, medians and ranges.  Equal results are asserted on every repetition: the two
libraries' variant, minor and deleted counts, every call's candidates and observations against the first one's.

    python tools/ins_scan_bench.py --parent-lib FILE [--length 57227415] [--reps 7] [--bench-note FILE] [--out FILE]
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

from del_scan_bench import other_minor  # noqa: E402
from filtered_scan_bench import OtherLib, spread  # noqa: E402
from decodingustools_amd import CallableOptions, Engine, _lib, synth, variants as V  # noqa: E402


def other_dels(other, mq, md, cnt, per, ref, exclude_flags):
    """(call ms, kernel ms, deleted positions) of the other library's filtered cl_site_scan_dels."""
    fn = other.lib.cl_site_scan_dels
    fn.argtypes = [C.c_void_p, C.c_uint8, C.POINTER(_lib.cl_scan_filter), C.POINTER(_lib.cl_del_params), C.c_void_p, C.c_uint64, C.c_uint32,
                   C.c_uint32, C.POINTER(_lib.cl_del_result)]
    r = _lib.cl_del_result()
    f = _lib.cl_scan_filter(exclude_flags, 1, 0)
    prm = _lib.cl_del_params(md, cnt, per)
    t0 = time.perf_counter()
    assert fn(other.h, mq, C.byref(f), C.byref(prm), ref.ctypes.data, ref.shape[0], 0, ref.shape[0], C.byref(r)) == 0
    call = (time.perf_counter() - t0) * 1e3
    ms = C.c_double(); b = C.c_uint64()
    other.lib.cl_site_scan_stats(other.h, C.byref(ms), C.byref(b))
    return call, ms.value, int(r.n_deleted)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=57_227_415)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-depth", type=int, default=10)
    ap.add_argument("--min-quality", type=int, default=20)
    ap.add_argument("--min-base-quality", type=int, default=20)
    ap.add_argument("--exclude-flags", type=lambda s: int(s, 0), default=0x704)
    ap.add_argument("--min-ins-count", type=int, default=3)
    ap.add_argument("--min-ins-per-10k", type=int, default=7000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_ins_scan.json"))
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
    mq, md, ex, cnt, per = a.min_quality, a.min_depth, a.exclude_flags, a.min_ins_count, a.min_ins_per_10k
    mcnt, mper, dcnt, dper = 3, 500, 3, 7000                              # the minor and the deletion scan's default rules
    out = {"workload": f"synthetic chrY-shaped contig, {L} bp, 40x, {rec.n} reads with bases (bench.py's config-5 generator and seed, "
                       f"0x10 on a seeded half of the reads, quality mix 2/12/23/37), tile resident on one GPU, attachment at base quality "
                       f">= {a.min_base_quality}; filter: exclude 0x{ex:04x}; insertion rule: min_depth {md}, count >= {cnt}, {per} per 10 000",
           "generate_s": gen, "reps": a.reps, "min_depth": md, "min_quality": mq}
    forms = ("scan", "scan_ex", "minor_filtered", "dels_filtered")
    ins_keys = ("ins", "ins_filtered", "ins_every", "ins_every_filtered")
    T = {k: {"call_ms": [], "kernel_ms": []} for k in forms + tuple("parent_" + f for f in forms) + ins_keys}
    for k in ins_keys:
        T[k]["scan_kernel_ms"] = []; T[k]["alleles_kernel_ms"] = []

    def timed(key, fn):
        t0 = time.perf_counter()
        r = fn()
        T[key]["call_ms"].append((time.perf_counter() - t0) * 1e3)
        T[key]["kernel_ms"].append(eng.site_scan_stats()[0])
        if key in ins_keys:
            s, al = eng.site_scan_ins_stats()
            T[key]["scan_kernel_ms"].append(s); T[key]["alleles_kernel_ms"].append(al)
        return r

    def ins_calls():
        return {"ins": lambda: eng.site_scan_ins(mq, md, cnt, per, scan_ref),
                "ins_filtered": lambda: eng.site_scan_ins(mq, md, cnt, per, scan_ref, filter=(ex, True)),
                "ins_every": lambda: eng.site_scan_ins(mq, 1, 1, 1, scan_ref),              # every position with a counted insertion
                "ins_every_filtered": lambda: eng.site_scan_ins(mq, 1, 1, 1, scan_ref, filter=(ex, True))}

    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        eng.site_attach_quals(rec, a.min_base_quality)
        first = eng.site_scan(mq, md, scan_ref)                                    # builds the per-window read index as well
        first_f = eng.site_scan_ex(mq, md, scan_ref, ex, True)
        first_m = eng.site_scan_minor(mq, md, mcnt, mper, scan_ref, filter=(ex, True))
        first_d = eng.site_scan_dels(mq, md, dcnt, dper, scan_ref, filter=(ex, True))
        first_i = {k: fn() for k, fn in ins_calls().items()}
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
                c, k, nm = other_minor(other, mq, md, mcnt, mper, scan_ref, ex)
                T["parent_minor_filtered"]["call_ms"].append(c); T["parent_minor_filtered"]["kernel_ms"].append(k)
                assert nm == first_m.minor
                c, k, nd = other_dels(other, mq, md, dcnt, dper, scan_ref, ex)
                T["parent_dels_filtered"]["call_ms"].append(c); T["parent_dels_filtered"]["kernel_ms"].append(k)
                assert nd == first_d.deleted
            u = timed("scan", lambda: eng.site_scan(mq, md, scan_ref))
            f = timed("scan_ex", lambda: eng.site_scan_ex(mq, md, scan_ref, ex, True))
            m = timed("minor_filtered", lambda: eng.site_scan_minor(mq, md, mcnt, mper, scan_ref, filter=(ex, True)))
            d = timed("dels_filtered", lambda: eng.site_scan_dels(mq, md, dcnt, dper, scan_ref, filter=(ex, True)))
            assert np.array_equal(u.candidates, first.candidates) and np.array_equal(f.candidates, first_f.candidates)
            assert np.array_equal(m.candidates, first_m.candidates) and np.array_equal(d.candidates, first_d.candidates)
            for key, fn in ins_calls().items():
                r = timed(key, fn)
                assert np.array_equal(r.candidates, first_i[key].candidates) and np.array_equal(r.observations, first_i[key].observations), key
        if other:
            other.close()
    for k, v in T.items():
        if v["call_ms"]:
            out[k] = {q: spread(x) for q, x in v.items()}
    out["scan"]["variants"] = int(first.variant); out["scan_ex"]["variants"] = int(first_f.variant); out["minor_filtered"]["minor"] = int(first_m.minor)
    out["dels_filtered"]["deleted"] = int(first_d.deleted)
    first_buffer = max(65536, L // 64)
    for k, r in first_i.items():
        out[k]["classes"] = {"low_depth": r.low_depth, "kept": r.kept, "inserted": r.inserted}
        out[k]["observations"] = int(r.observations.shape[0])
        out[k]["alleles"] = len(V.ins_alleles(r.observations))
        out[k]["scan_launches_per_call"] = 1 if r.inserted <= first_buffer else 2
    out["ins_every"]["rule"] = out["ins_every_filtered"]["rule"] = "min_depth 1, count >= 1, 1 per 10 000: every position with a counted insertion"
    # the new scan's window kernel against the deletion scan's of the same run, and what the allele launch adds to it
    out["kernel_ratio_ins_filtered_scan_over_dels_filtered"] = out["ins_filtered"]["scan_kernel_ms"]["median"] / out["dels_filtered"]["kernel_ms"]["median"]
    out["alleles_share_of_ins_every_filtered_kernel"] = out["ins_every_filtered"]["alleles_kernel_ms"]["median"] / out["ins_every_filtered"]["kernel_ms"]["median"]
    out["alleles_share_of_ins_every_kernel"] = out["ins_every"]["alleles_kernel_ms"]["median"] / out["ins_every"]["kernel_ms"]["median"]
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
