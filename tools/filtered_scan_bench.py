#!/usr/bin/env python3
"""What the filtered, strand-aware site scan (cl_site_scan_ex) costs on one GPU, on the config-5 tile of bench.py that
tools/variant_scan_bench.py uses (chrY-shaped, 40x, 150-bp reads with bases, same generator and seed; the generator's
own flags plus a seeded 0x10 on half of the reads, and its config-2 quality mix), tile resident (cl_site_upload).

  1. cl_site_scan_ex (exclude 0x704, Q20) against the unfiltered cl_site_scan on the same tile, alternating repetitions:
     kernel by device events and call to return, medians and ranges.
  2. The attachment (cl_site_attach_quals: host pass-bit pack + upload of bits and flags), call to return.
  3. With --parent-lib: the unfiltered cl_site_scan of another build of the library (the parent commit's) on the same
     tile in the same process, alternating with this build's.  That library is loaded beside this one and only the
     calls both have are bound (cl_create, cl_site_upload, cl_site_scan, cl_site_scan_stats, cl_destroy) -- and, when it
     exports them, cl_site_attach_quals and cl_site_scan_ex: its filtered scan is then timed in the same loop too.

    python tools/filtered_scan_bench.py [--length 57227415] [--reps 5] [--parent-lib FILE] [--bench-note FILE] [--out FILE]
"""
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
from decodingustools_amd.callable_loci import _site_quals  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


class OtherLib:
    """The scans of another build of the library: the unfiltered one through the calls every build has, the filtered
    one when that build exports it."""

    def __init__(self, path, rec, L):
        self.lib = lib = C.CDLL(path)
        lib.cl_create.argtypes = [C.POINTER(_lib.cl_options), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        lib.cl_site_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(_lib.cl_site_tile)]
        lib.cl_site_scan.argtypes = [C.c_void_p, C.c_uint8, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                     C.POINTER(_lib.cl_scan_result)]
        lib.cl_site_scan_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        lib.cl_destroy.argtypes = [C.c_void_p]
        lib.cl_destroy.restype = None
        self.h = C.c_void_p()
        opt = CallableOptions().to_c()
        assert lib.cl_create(C.byref(opt), 0, None, C.byref(self.h)) == 0
        t = _lib.cl_site_tile()
        t.n_reads = rec.n
        for f in ("pos", "mapq", "cigar_off", "cigar", "seq_off", "seq4"):
            setattr(t, f, getattr(rec, f).ctypes.data)
        assert lib.cl_site_upload(self.h, L, L, C.byref(t)) == 0
        self.filtered = hasattr(lib, "cl_site_attach_quals") and hasattr(lib, "cl_site_scan_ex")
        if self.filtered:
            lib.cl_site_attach_quals.argtypes = [C.c_void_p, C.POINTER(_lib.cl_site_quals), C.c_uint8]
            lib.cl_site_scan_ex.argtypes = [C.c_void_p, C.c_uint8, C.c_uint32, C.POINTER(_lib.cl_scan_filter), C.c_void_p, C.c_uint64,
                                            C.c_uint32, C.c_uint32, C.POINTER(_lib.cl_scan_result_ex)]

    def attach(self, rec, min_base_quality):
        q = _site_quals(rec)
        assert self.lib.cl_site_attach_quals(self.h, C.byref(q), min_base_quality) == 0

    def scan(self, mq, md, ref, exclude_flags=None):
        """(call ms, kernel ms, variants) of cl_site_scan, or of cl_site_scan_ex (exclude_flags given; base quality on)."""
        if exclude_flags is None:
            r = _lib.cl_scan_result()
            t0 = time.perf_counter()
            assert self.lib.cl_site_scan(self.h, mq, md, ref.ctypes.data, ref.shape[0], 0, ref.shape[0], C.byref(r)) == 0
        else:
            r = _lib.cl_scan_result_ex()
            f = _lib.cl_scan_filter(exclude_flags, 1, 0)
            t0 = time.perf_counter()
            assert self.lib.cl_site_scan_ex(self.h, mq, md, C.byref(f), ref.ctypes.data, ref.shape[0], 0, ref.shape[0], C.byref(r)) == 0
        call = (time.perf_counter() - t0) * 1e3
        ms = C.c_double(); b = C.c_uint64()
        self.lib.cl_site_scan_stats(self.h, C.byref(ms), C.byref(b))
        return call, ms.value, int(r.n_variant)

    def close(self):
        self.lib.cl_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=57_227_415)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-depth", type=int, default=10)
    ap.add_argument("--min-quality", type=int, default=20)
    ap.add_argument("--min-base-quality", type=int, default=20)
    ap.add_argument("--exclude-flags", type=lambda s: int(s, 0), default=0x704)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_scan_unified.json"))
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
    mq, md, ex = a.min_quality, a.min_depth, a.exclude_flags
    out = {"workload": f"synthetic chrY-shaped contig, {L} bp, 40x, {rec.n} reads with bases (bench.py's config-5 generator and seed, "
                       f"0x10 on a seeded half of the reads, quality mix 2/12/23/37), tile resident on one GPU; scanned against a "
                       f"reference with {planted.shape[0]} substitutions; filter: exclude 0x{ex:04x}, base quality >= {a.min_base_quality}",
           "generate_s": gen, "reps": a.reps, "min_depth": md, "min_quality": mq}
    with Engine(CallableOptions(), 0) as eng:
        eng.site_upload(L, L, rec)
        first = eng.site_scan(mq, md, scan_ref)                                    # builds the per-window read index as well
        attach = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            eng.site_attach_quals(rec, a.min_base_quality)
            attach.append((time.perf_counter() - t0) * 1e3)
        first_f = eng.site_scan_ex(mq, md, scan_ref, ex, True)
        other = OtherLib(a.parent_lib, rec, L) if a.parent_lib else None
        if other:
            assert other.scan(mq, md, scan_ref)[2] == first.variant
            if other.filtered:
                other.attach(rec, a.min_base_quality)
                assert other.scan(mq, md, scan_ref, ex)[2] == first_f.variant
        f_call, f_kern, u_call, u_kern, p_call, p_kern, pf_call, pf_kern = [], [], [], [], [], [], [], []
        for _ in range(a.reps):
            if other:
                c, k, nv = other.scan(mq, md, scan_ref)
                p_call.append(c); p_kern.append(k)
                assert nv == first.variant
                if other.filtered:
                    c, k, nv = other.scan(mq, md, scan_ref, ex)
                    pf_call.append(c); pf_kern.append(k)
                    assert nv == first_f.variant
            t0 = time.perf_counter()
            u = eng.site_scan(mq, md, scan_ref)
            u_call.append((time.perf_counter() - t0) * 1e3)
            u_kern.append(eng.site_scan_stats()[0])
            t0 = time.perf_counter()
            f = eng.site_scan_ex(mq, md, scan_ref, ex, True)
            f_call.append((time.perf_counter() - t0) * 1e3)
            ms, fbytes = eng.site_scan_stats()
            f_kern.append(ms)
        off = eng.site_scan_ex(mq, md, scan_ref, 0, False)
        assert off.variant == u.variant and np.array_equal(off.candidates["pos"], u.candidates["pos"])
        out["attach_ms"] = spread(attach)
        out["attach_bytes"] = (int(rec.seq_off[-1]) + 7) // 8 + 2 * rec.n
        out["unfiltered_scan"] = {"call_ms": spread(u_call), "kernel_ms": spread(u_kern), "variants": int(u.variant)}
        out["filtered_scan"] = {"call_ms": spread(f_call), "kernel_ms": spread(f_kern), "variants": int(f.variant), "algorithmic_bytes": int(fbytes),
                                "classes": {"low_depth": f.low_depth, "mixed": f.mixed, "uncomparable": f.uncomparable, "match": f.match,
                                            "variant": f.variant}}
        out["kernel_ratio_filtered_over_unfiltered"] = out["filtered_scan"]["kernel_ms"]["median"] / out["unfiltered_scan"]["kernel_ms"]["median"]
        if other:
            out["parent_unfiltered_scan"] = {"call_ms": spread(p_call), "kernel_ms": spread(p_kern), "library": os.path.basename(a.parent_lib)}
            out["kernel_ratio_filtered_over_parent"] = out["filtered_scan"]["kernel_ms"]["median"] / out["parent_unfiltered_scan"]["kernel_ms"]["median"]
            pk, uk = out["parent_unfiltered_scan"]["kernel_ms"], out["unfiltered_scan"]["kernel_ms"]
            out["unfiltered_ranges_overlap_parent"] = bool(uk["min"] <= pk["max"] and pk["min"] <= uk["max"])
            if other.filtered:
                out["parent_filtered_scan"] = {"call_ms": spread(pf_call), "kernel_ms": spread(pf_kern)}
            # the gate of a change that must cost nothing: this build's median within the parent's own observed range
            out["median_within_parent_max"] = {
                f"{form}_{q}": bool(out[f"{form}_scan"][q]["median"] <= out[f"parent_{form}_scan"][q]["max"])
                for form in ("unfiltered", "filtered") if f"parent_{form}_scan" in out for q in ("kernel_ms", "call_ms")}
            other.close()
    if a.bench_note:
        out.update(json.load(open(a.bench_note)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("workload",)}))


if __name__ == "__main__":
    main()
