#!/usr/bin/env python3
"""What the error profile (cl_site_error_profile) costs on one GPU, what the route without its kernels costs, and what it
leaves alone, on the config-5 tile of bench.py that tools/str_scan_bench.py uses (same generator, seed, flags and quality
mix), tile resident, attachment on, filter 0x704 with the base-quality bit, min_quality 20, C = 50 and C = 256.

Per repetition, alternating in one process on the same resident tile:
  cl_site_scan, cl_site_scan_ex, the filtered cl_site_scan_dels and cl_site_str_lengths of the parent commit's library
  (--parent-lib FILE), then the same four of this build, both through bare ctypes calls on a context of their own
  cl_site_error_profile at each C: both launches by events (cl_site_error_profile_stats), the call to return
  dut_error_profile_measure over the same host arrays, the route without the kernels: on one thread (a second copy of this
  build's library whose thread pool was started with DUT_THREADS=1) and on the process's DUT_THREADS threads -- its tables
  asserted equal to the device's on every repetition
Medians and ranges.  No ratio is fixed in advance: the file records what came out.

    python tools/error_profile_bench.py --parent-lib FILE [--length 57227415] [--reps 7] [--bench-note FILE] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from filtered_scan_bench import OtherLib, spread  # noqa: E402
from ins_scan_bench import other_dels  # noqa: E402
from decodingustools_amd import CallableOptions, Engine, ErrorProfile, _lib, synth  # noqa: E402


def other_str(other, mq, flank, loci, exclude_flags):
    """(call ms, kernel ms, spanning reads) of the other library's filtered cl_site_str_lengths."""
    fn = other.lib.cl_site_str_lengths
    fn.argtypes = [C.c_void_p, C.c_uint8, C.POINTER(_lib.cl_scan_filter), C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(_lib.cl_str_result)]
    r = _lib.cl_str_result()
    f = _lib.cl_scan_filter(exclude_flags, 0, 0)
    t0 = time.perf_counter()
    assert fn(other.h, mq, C.byref(f), flank, loci.ctypes.data, loci.shape[0], C.byref(r)) == 0
    call = (time.perf_counter() - t0) * 1e3
    ms = C.c_double(); b = C.c_uint64()
    other.lib.cl_site_scan_stats(other.h, C.byref(ms), C.byref(b))
    return call, ms.value, int(np.ctypeslib.as_array(r.hist, shape=(loci.shape[0] * 2 * _lib.CL_STR_BINS,)).sum())


class HostRoute:
    """dut_error_profile_measure of a library handle over one set of records."""

    def __init__(self, lib, rec, L, ref):
        self.fn = lib.dut_error_profile_measure
        self.fn.argtypes = dict((n, a) for n, _r, a in _lib.SYMBOLS)["dut_error_profile_measure"]
        self.fn.restype = C.c_int
        self.rec, self.L, self.ref = rec, L, ref
        self.reads = _lib.dut_ep_reads(rec.n, *[a.ctypes.data for a in (rec.pos, rec.flag, rec.mapq, rec.cigar_off, rec.cigar, rec.seq_off, rec.seq4,
                                                                          rec.qual_off, rec.qual)])

    def run(self, n_cycles, mq, exclude_flags, min_base_quality, end=None):
        opt = _lib.dut_ep_options(mq, 1, exclude_flags, 1, min_base_quality, n_cycles)
        tables = np.zeros(36 * n_cycles, np.uint64)
        r = _lib.cl_ep_result()
        t0 = time.perf_counter()
        st = self.fn(C.byref(self.reads), self.L, self.ref.ctypes.data, self.ref.shape[0], 0, self.L if end is None else end, C.byref(opt), tables.ctypes.data, C.byref(r))
        ms = (time.perf_counter() - t0) * 1e3
        assert st == 0
        return ms, ErrorProfile.from_c(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=57_227_415)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cycles", type=int, nargs="+", default=[50, 256])
    ap.add_argument("--min-depth", type=int, default=10)
    ap.add_argument("--min-quality", type=int, default=20)
    ap.add_argument("--min-base-quality", type=int, default=20)
    ap.add_argument("--exclude-flags", type=lambda s: int(s, 0), default=0x704)
    ap.add_argument("--loci", type=int, default=50_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_error_profile.json"))
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
    lrng = np.random.default_rng(17)
    spans = lrng.integers(8, 121, a.loci)
    starts = (lrng.random(a.loci) * (L - spans)).astype(np.int64)
    loci = np.ascontiguousarray(np.stack([starts, starts + spans], 1), np.uint32)
    gen = time.perf_counter() - t0
    mq, md, ex, bq = a.min_quality, a.min_depth, a.exclude_flags, a.min_base_quality
    out = {"workload": f"synthetic chrY-shaped contig, {L} bp, 40x, {rec.n} reads with bases (bench.py's config-5 generator and seed, 0x10 on a seeded "
                       f"half of the reads), tile resident on one GPU, attachment at base quality >= {bq}; filter: exclude 0x{ex:04x} with the "
                       f"base-quality bit; min_quality {mq}; C in {a.cycles}; the str catalogue of tools/str_scan_bench.py ({a.loci} loci, flank 5)",
           "generate_s": gen, "reps": a.reps, "cycles": a.cycles, "min_quality": mq, "host_threads": None}
    forms = ("scan", "scan_ex", "dels_filtered", "str_lengths_filtered")
    ep_keys = tuple(f"error_profile_c{c}" for c in a.cycles)
    T = {k: {"call_ms": [], "kernel_ms": []} for k in forms + tuple("parent_" + f for f in forms)}
    T.update({k: {"call_ms": [], "kernel_ms": [], "table_kernel_ms": [], "sum_kernel_ms": []} for k in ep_keys})
    H = {f"host_{who}_c{c}_ms": [] for who in ("1_thread", "threads") for c in a.cycles}

    def timed(key, fn):
        t0 = time.perf_counter()
        r = fn()
        T[key]["call_ms"].append((time.perf_counter() - t0) * 1e3)
        T[key]["kernel_ms"].append(eng.site_scan_stats()[0])
        return r

    tmp = tempfile.mkdtemp()
    try:
        with Engine(CallableOptions(), 0) as eng:
            eng.site_upload(L, L, rec)
            eng.site_attach_quals(rec, bq)
            first = eng.site_scan(mq, md, scan_ref)
            first_f = eng.site_scan_ex(mq, md, scan_ref, ex, True)
            first_d = eng.site_scan_dels(mq, md, 3, 7000, scan_ref, filter=(ex, True))
            first_s = eng.site_str_lengths(loci, 5, mq, filter=(ex, False))
            first_e = {c: eng.site_error_profile(c, mq, scan_ref, filter=(ex, True)) for c in a.cycles}
            # the host route: this process's pool, and a second copy of the library whose pool starts with one thread
            many = HostRoute(eng._lib, rec, L, scan_ref)
            one_path = os.path.join(tmp, "libcallable_hip_one_thread.so")
            shutil.copy(_lib.lib_path(), one_path)
            keep = os.environ.get("DUT_THREADS")
            os.environ["DUT_THREADS"] = "1"
            one = HostRoute(C.CDLL(one_path), rec, L, scan_ref)
            one.run(a.cycles[0], mq, ex, bq, end=4096)                        # (its pool's size is taken here)
            if keep is None:
                del os.environ["DUT_THREADS"]
            else:
                os.environ["DUT_THREADS"] = keep
            out["host_threads"] = int(keep) if keep else "the library's default for this process"
            other = OtherLib(a.parent_lib, rec, L) if a.parent_lib else None
            mine = OtherLib(_lib.lib_path(), rec, L)
            mine.attach(rec, bq)
            if other:
                assert other.filtered and hasattr(other.lib, "cl_site_str_lengths"), "the parent library lacks a call this file times"
                assert not hasattr(other.lib, "cl_site_error_profile"), "--parent-lib is not the parent: it has cl_site_error_profile"
                other.attach(rec, bq)
            for _ in range(a.reps):
                # the existing calls, parent's library then this build's, each through the same bare ctypes route on a context of its own
                for side, lib in (("parent_", other), ("", mine)):
                    if lib is None:
                        continue
                    for key, flt in (("scan", None), ("scan_ex", ex)):
                        c, k, nv = lib.scan(mq, md, scan_ref, flt)
                        T[side + key]["call_ms"].append(c); T[side + key]["kernel_ms"].append(k)
                        assert nv == (first.variant if flt is None else first_f.variant)
                    c, k, nd = other_dels(lib, mq, md, 3, 7000, scan_ref, ex)
                    T[side + "dels_filtered"]["call_ms"].append(c); T[side + "dels_filtered"]["kernel_ms"].append(k)
                    assert nd == first_d.deleted
                    c, k, ns = other_str(lib, mq, 5, loci, ex)
                    T[side + "str_lengths_filtered"]["call_ms"].append(c); T[side + "str_lengths_filtered"]["kernel_ms"].append(k)
                    assert ns == int(first_s.hist.sum())
                for c, key in zip(a.cycles, ep_keys):
                    r = timed(key, lambda: eng.site_error_profile(c, mq, scan_ref, filter=(ex, True)))
                    tk, sk = eng.site_error_profile_stats()
                    T[key]["table_kernel_ms"].append(tk); T[key]["sum_kernel_ms"].append(sk)
                    assert r.tables_equal(first_e[c]), "two calls gave other tables"
                    for name, route in (("host_1_thread", one), ("host_threads", many)):
                        ms, prof = route.run(c, mq, ex, bq)
                        H[f"{name}_c{c}_ms"].append(ms)
                        assert prof.tables_equal(r), "the host route gives other tables"
            mine.close()
            if other:
                other.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for k, v in T.items():
        if v["call_ms"]:
            out[k] = {q: spread(x) for q, x in v.items()}
    for k, v in H.items():
        out[k] = spread(v)
    for c, key in zip(a.cycles, ep_keys):
        e = first_e[c]
        out[key].update(reads=e.reads, bases=e.bases, uncomparable=e.uncomparable, mismatches=e.bases - int(e.total.trace()), insertions=e.ins, deletions=e.dels,
                        bytes_back=8 * (36 * c + 22))
        out[f"speedup_call_over_host_1_thread_c{c}"] = out[f"host_1_thread_c{c}_ms"]["median"] / out[key]["call_ms"]["median"]
        out[f"speedup_call_over_host_threads_c{c}"] = out[f"host_threads_c{c}_ms"]["median"] / out[key]["call_ms"]["median"]
        out[f"kernel_over_scan_ex_kernel_c{c}"] = out[key]["kernel_ms"]["median"] / out["scan_ex"]["kernel_ms"]["median"]
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
