#!/usr/bin/env python3
"""What the repeat-length call (cl_site_str_lengths) costs on one GPU, what the route without its kernel costs, and what it
leaves alone, on the config-5 tile of bench.py that tools/cons_scan_bench.py uses (same generator, seed, flags and quality
mix), tile resident, attachment on.  The catalogue: --loci seeded loci of span 8..120 at uniform starts, flank 5.

Per repetition, alternating in one process on the same resident tile:
  cl_site_scan, cl_site_scan_ex, the filtered cl_site_scan_dels and the filtered cl_site_scan_consensus of the parent
  commit's library (--parent-lib FILE), then the same four of this build
  cl_site_str_lengths, unfiltered and filtered, over the whole catalogue (kernel by events, call to return)
  dut_str_measure over the same host arrays, the route without the kernel: on one thread (a second copy of this build's
  library whose thread pool was started with DUT_THREADS=1) and on the process's DUT_THREADS threads -- its histograms and
  partial counts asserted equal to the device's on every repetition
Medians and ranges.  No ratio is fixed in advance: the file records what came out.

    python tools/str_scan_bench.py --parent-lib FILE [--length 57227415] [--loci 50000] [--reps 7] [--bench-note FILE] [--out FILE]
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

from filtered_scan_bench import OtherLib, spread  # noqa: E402
from ins_scan_bench import other_dels  # noqa: E402
from decodingustools_amd import CallableOptions, Engine, _lib, synth, variants as V  # noqa: E402


def other_cons(other, mq, md, cnt, per, ref, exclude_flags):
    """(call ms, kernel ms, deleted positions) of the other library's filtered cl_site_scan_consensus."""
    fn = other.lib.cl_site_scan_consensus
    fn.argtypes = [C.c_void_p, C.c_uint8, C.POINTER(_lib.cl_scan_filter), C.POINTER(_lib.cl_cons_params), C.c_void_p, C.c_uint64, C.c_uint32,
                   C.c_uint32, C.POINTER(_lib.cl_cons_result)]
    r = _lib.cl_cons_result()
    f = _lib.cl_scan_filter(exclude_flags, 1, 0)
    prm = _lib.cl_cons_params(md, cnt, per)
    t0 = time.perf_counter()
    assert fn(other.h, mq, C.byref(f), C.byref(prm), ref.ctypes.data, ref.shape[0], 0, ref.shape[0], C.byref(r)) == 0
    call = (time.perf_counter() - t0) * 1e3
    ms = C.c_double(); b = C.c_uint64()
    other.lib.cl_site_scan_stats(other.h, C.byref(ms), C.byref(b))
    return call, ms.value, int(r.n_deleted)


class HostRoute:
    """dut_str_measure of a library handle over one set of records and loci."""

    def __init__(self, lib, rec, L, loci, flank):
        self.fn = lib.dut_str_measure
        self.fn.argtypes = dict((n, a) for n, _r, a in _lib.SYMBOLS)["dut_str_measure"]
        self.fn.restype = C.c_int
        self.rec, self.L, self.loci, self.flank = rec, L, loci, flank

    def run(self, mq, exclude_flags):
        strands = 1 if exclude_flags is None else 2
        hist = np.zeros((self.loci.shape[0], strands, _lib.CL_STR_BINS), np.uint32)
        partial = np.zeros(self.loci.shape[0], np.uint32)
        r = self.rec
        t0 = time.perf_counter()
        st = self.fn(r.pos.ctypes.data, r.flag.ctypes.data, r.mapq.ctypes.data, r.cigar_off.ctypes.data, r.cigar.ctypes.data, r.n, self.L, mq,
                     exclude_flags or 0, self.flank, self.loci.ctypes.data, self.loci.shape[0], hist.ctypes.data, partial.ctypes.data, strands)
        ms = (time.perf_counter() - t0) * 1e3
        assert st == 0
        return ms, hist, partial


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=57_227_415)
    ap.add_argument("--loci", type=int, default=50_000)
    ap.add_argument("--flank", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-depth", type=int, default=10)
    ap.add_argument("--min-quality", type=int, default=20)
    ap.add_argument("--min-base-quality", type=int, default=20)
    ap.add_argument("--exclude-flags", type=lambda s: int(s, 0), default=0x704)
    ap.add_argument("--min-del-count", type=int, default=3)
    ap.add_argument("--min-del-per-10k", type=int, default=7000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_str_scan.json"))
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
    mq, md, ex, cnt, per = a.min_quality, a.min_depth, a.exclude_flags, a.min_del_count, a.min_del_per_10k
    out = {"workload": f"synthetic chrY-shaped contig, {L} bp, 40x, {rec.n} reads with bases (bench.py's config-5 generator and seed, 0x10 on a seeded "
                       f"half of the reads), tile resident on one GPU, attachment at base quality >= {a.min_base_quality}; catalogue: {a.loci} seeded loci, "
                       f"spans 8..120, uniform starts, flank {a.flank}; filter: exclude 0x{ex:04x}; min_quality {mq}",
           "generate_s": gen, "reps": a.reps, "loci": a.loci, "flank": a.flank, "min_quality": mq, "host_threads": None}
    forms = ("scan", "scan_ex", "dels_filtered", "consensus_filtered")
    str_keys = ("str_lengths", "str_lengths_filtered")
    T = {k: {"call_ms": [], "kernel_ms": []} for k in forms + tuple("parent_" + f for f in forms) + str_keys}
    H = {k: [] for k in ("host_1_thread_ms", "host_1_thread_filtered_ms", "host_threads_ms", "host_threads_filtered_ms")}

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
            eng.site_attach_quals(rec, a.min_base_quality)
            first = eng.site_scan(mq, md, scan_ref)
            first_f = eng.site_scan_ex(mq, md, scan_ref, ex, True)
            first_d = eng.site_scan_dels(mq, md, cnt, per, scan_ref, filter=(ex, True))
            first_c = eng.site_scan_consensus(mq, md, cnt, per, scan_ref, filter=(ex, True))
            first_s = {"str_lengths": eng.site_str_lengths(loci, a.flank, mq), "str_lengths_filtered": eng.site_str_lengths(loci, a.flank, mq, filter=(ex, False))}
            # the host route: this process's pool, and a second copy of the library whose pool starts with one thread
            many = HostRoute(eng._lib, rec, L, loci, a.flank)
            one_path = os.path.join(tmp, "libcallable_hip_one_thread.so")
            shutil.copy(_lib.lib_path(), one_path)
            keep = os.environ.get("DUT_THREADS")
            os.environ["DUT_THREADS"] = "1"
            one = HostRoute(C.CDLL(one_path), rec, L, loci[:64], a.flank)
            one.run(mq, None)                                                 # (its pool's size is taken here)
            one.loci = loci
            if keep is None:
                del os.environ["DUT_THREADS"]
            else:
                os.environ["DUT_THREADS"] = keep
            out["host_threads"] = int(keep) if keep else "the library's default for this process"
            other = OtherLib(a.parent_lib, rec, L) if a.parent_lib else None
            if other:
                assert other.filtered and hasattr(other.lib, "cl_site_scan_consensus"), "the parent library lacks a scan this file times"
                assert not hasattr(other.lib, "cl_site_str_lengths"), "--parent-lib is not the parent: it has cl_site_str_lengths"
                other.attach(rec, a.min_base_quality)
            for _ in range(a.reps):
                if other:
                    for key, flt in (("parent_scan", None), ("parent_scan_ex", ex)):
                        c, k, nv = other.scan(mq, md, scan_ref, flt)
                        T[key]["call_ms"].append(c); T[key]["kernel_ms"].append(k)
                        assert nv == (first.variant if flt is None else first_f.variant)
                    c, k, nd = other_dels(other, mq, md, cnt, per, scan_ref, ex)
                    T["parent_dels_filtered"]["call_ms"].append(c); T["parent_dels_filtered"]["kernel_ms"].append(k)
                    assert nd == first_d.deleted
                    c, k, nd = other_cons(other, mq, md, cnt, per, scan_ref, ex)
                    T["parent_consensus_filtered"]["call_ms"].append(c); T["parent_consensus_filtered"]["kernel_ms"].append(k)
                    assert nd == first_c.deleted
                u = timed("scan", lambda: eng.site_scan(mq, md, scan_ref))
                f = timed("scan_ex", lambda: eng.site_scan_ex(mq, md, scan_ref, ex, True))
                d = timed("dels_filtered", lambda: eng.site_scan_dels(mq, md, cnt, per, scan_ref, filter=(ex, True)))
                c = timed("consensus_filtered", lambda: eng.site_scan_consensus(mq, md, cnt, per, scan_ref, filter=(ex, True)))
                assert np.array_equal(u.candidates, first.candidates) and np.array_equal(f.candidates, first_f.candidates)
                assert np.array_equal(d.candidates, first_d.candidates) and np.array_equal(c.cons, first_c.cons)
                for key, flt, exf in (("str_lengths", None, None), ("str_lengths_filtered", (ex, False), ex)):
                    r = timed(key, lambda: eng.site_str_lengths(loci, a.flank, mq, filter=flt))
                    assert np.array_equal(r.hist, first_s[key].hist) and np.array_equal(r.partial, first_s[key].partial)
                    sfx = "_filtered_ms" if flt else "_ms"
                    for name, route in (("host_1_thread", one), ("host_threads", many)):
                        ms, hist, partial = route.run(mq, exf)
                        H[name + sfx].append(ms)
                        assert np.array_equal(hist, r.hist) and np.array_equal(partial, r.partial), "the host route gives other histograms"
            if other:
                other.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for k, v in T.items():
        if v["call_ms"]:
            out[k] = {q: spread(x) for q, x in v.items()}
    for k, v in H.items():
        out[k] = spread(v)
    for key, r in first_s.items():
        n = r.hist.sum(axis=(1, 2))
        calls = [V.str_call(h[0], h[1] if h.shape[0] == 2 else None, md, 7000)["status"] for h in r.hist]
        out[key].update(spanning_reads=int(n.sum()), partial_reads=int(r.partial.sum()), other_bin=int(r.hist[:, :, 127].sum()),
                        reads_per_locus_median=float(np.median(n + r.partial)),
                        status={s: calls.count(i) for i, s in enumerate(V.STR_STATUS_NAMES)}, bytes_back=int(r.hist.nbytes + r.partial.nbytes))
    out["speedup_call_over_host_1_thread"] = out["host_1_thread_filtered_ms"]["median"] / out["str_lengths_filtered"]["call_ms"]["median"]
    out["speedup_call_over_host_threads"] = out["host_threads_filtered_ms"]["median"] / out["str_lengths_filtered"]["call_ms"]["median"]
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
