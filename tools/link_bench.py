#!/usr/bin/env python3
"""What the linked-sites call (cl_site_link_counts) costs on one GPU, what the route without its kernel costs, and what it
leaves alone, on the config-5 tile of bench.py that tools/str_scan_bench.py uses (same generator, seed, flags and quality
mix), tile resident, attachment on.  The sites: the positions cl_site_scan lists as variants on that tile; max_partners 4,
max_dist 1000.

Per repetition, alternating in one process on the same resident tile:
  cl_site_scan, cl_site_scan_ex and the filtered cl_site_scan_dels of the parent commit's library (--parent-lib FILE), then
  the same three of this build
  cl_site_link_counts, unfiltered and filtered, over all sites (kernel by events, call to return)
  dut_link_measure over the same host arrays, the route without the kernel: on one thread (a second copy of this build's
  library whose thread pool was started with DUT_THREADS=1) and on the process's DUT_THREADS threads -- its first, tables and
  site counts asserted equal to the device's on every repetition
Medians and ranges.  No ratio is fixed in advance: the file records what came out.

    python tools/link_bench.py --parent-lib FILE [--length 57227415] [--reps 7] [--bench-note FILE] [--out FILE]
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


class HostRoute:
    """dut_link_measure of a library handle over one set of records and sites."""

    def __init__(self, lib, rec, L, sites, max_dist, max_partners):
        protos = dict((n, a) for n, _r, a in _lib.SYMBOLS)
        self.fn, self.offsets = lib.dut_link_measure, lib.dut_link_pair_offsets
        self.fn.argtypes, self.fn.restype = protos["dut_link_measure"], C.c_int
        self.offsets.argtypes, self.offsets.restype = protos["dut_link_pair_offsets"], C.c_int
        self.rec, self.L, self.sites, self.D, self.K = rec, L, sites, max_dist, max_partners
        r = rec
        self.keep = [r.pos, r.flag, r.mapq, r.cigar_off, r.cigar, r.seq_off, r.seq4, r.qual_off, r.qual]
        self.reads = _lib.dut_ep_reads(r.n, *[x.ctypes.data if x.shape[0] else None for x in self.keep])

    def run(self, mq, exclude_flags, min_base_quality):
        n = self.sites.shape[0]
        n_pairs = C.c_uint64()
        assert self.offsets(self.sites.ctypes.data, n, self.D, self.K, None, C.byref(n_pairs)) == 0
        first = np.zeros(n + 1, np.uint32)
        tables = np.zeros((n_pairs.value, 6, 6), np.uint32)
        counts = np.zeros((n, 6), np.uint32)
        opt = _lib.dut_link_options(1, mq, 0 if exclude_flags is None else 1, exclude_flags or 0, 0 if min_base_quality is None else 1, min_base_quality or 0,
                                    self.D, self.K, 1, 0)
        t0 = time.perf_counter()
        st = self.fn(C.byref(self.reads), self.L, C.byref(opt), self.sites.ctypes.data, n, first.ctypes.data, tables.ctypes.data, counts.ctypes.data)
        ms = (time.perf_counter() - t0) * 1e3
        assert st == 0
        return ms, first, tables, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=57_227_415)
    ap.add_argument("--max-dist", type=int, default=1000)
    ap.add_argument("--max-partners", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-depth", type=int, default=10)
    ap.add_argument("--min-quality", type=int, default=20)
    ap.add_argument("--min-base-quality", type=int, default=20)
    ap.add_argument("--exclude-flags", type=lambda s: int(s, 0), default=0x704)
    ap.add_argument("--min-del-count", type=int, default=3)
    ap.add_argument("--min-del-per-10k", type=int, default=7000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_link_counts.json"))
    a = ap.parse_args()
    L, D, K = a.length, a.max_dist, a.max_partners
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
    mq, md, ex, cnt, per, mbq = a.min_quality, a.min_depth, a.exclude_flags, a.min_del_count, a.min_del_per_10k, a.min_base_quality
    out = {"workload": f"synthetic chrY-shaped contig, {L} bp, 40x, {rec.n} reads with bases (bench.py's config-5 generator and seed, 0x10 on a seeded "
                       f"half of the reads), tile resident on one GPU, attachment at base quality >= {mbq}; sites: the positions cl_site_scan lists as "
                       f"variants at min_depth {md}; max_dist {D}, max_partners {K}; filter: exclude 0x{ex:04x} with the pass bits; min_quality {mq}",
           "generate_s": gen, "reps": a.reps, "max_dist": D, "max_partners": K, "min_quality": mq, "host_threads": None}
    forms = ("scan", "scan_ex", "dels_filtered")
    link_keys = ("link_counts", "link_counts_filtered")
    T = {k: {"call_ms": [], "kernel_ms": []} for k in forms + tuple("parent_" + f for f in forms) + link_keys}
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
            eng.site_attach_quals(rec, mbq)
            first = eng.site_scan(mq, md, scan_ref)
            first_f = eng.site_scan_ex(mq, md, scan_ref, ex, True)
            first_d = eng.site_scan_dels(mq, md, cnt, per, scan_ref, filter=(ex, True))
            sites = np.ascontiguousarray(first.candidates["pos"].astype(np.uint32) - 1)          # candidates carry 1-based positions, ascending
            assert sites.shape[0] > 0 and np.all(np.diff(sites.astype(np.int64)) > 0)
            out["sites"] = int(sites.shape[0])
            first_l = {"link_counts": eng.site_link_counts(sites, D, K, mq), "link_counts_filtered": eng.site_link_counts(sites, D, K, mq, filter=(ex, True))}
            # the host route: this process's pool, and a second copy of the library whose pool starts with one thread
            many = HostRoute(eng._lib, rec, L, sites, D, K)
            one_path = os.path.join(tmp, "libcallable_hip_one_thread.so")
            shutil.copy(_lib.lib_path(), one_path)
            keep = os.environ.get("DUT_THREADS")
            os.environ["DUT_THREADS"] = "1"
            one = HostRoute(C.CDLL(one_path), rec, L, sites[:64], D, K)
            one.run(mq, None, None)                                           # (its pool's size is taken here)
            one.sites = sites
            if keep is None:
                del os.environ["DUT_THREADS"]
            else:
                os.environ["DUT_THREADS"] = keep
            out["host_threads"] = int(keep) if keep else "the library's default for this process"
            other = OtherLib(a.parent_lib, rec, L) if a.parent_lib else None
            if other:
                assert other.filtered and hasattr(other.lib, "cl_site_scan_dels"), "the parent library lacks a scan this file times"
                assert not hasattr(other.lib, "cl_site_link_counts"), "--parent-lib is not the parent: it has cl_site_link_counts"
                other.attach(rec, mbq)
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
                for key, flt, exf, bqf in (("link_counts", None, None, None), ("link_counts_filtered", (ex, True), ex, mbq)):
                    r = timed(key, lambda: eng.site_link_counts(sites, D, K, mq, filter=flt))
                    z = first_l[key]
                    assert np.array_equal(r.first, z.first) and np.array_equal(r.tables, z.tables) and np.array_equal(r.site_counts, z.site_counts)
                    sfx = "_filtered_ms" if flt else "_ms"
                    for name, route in (("host_1_thread", one), ("host_threads", many)):
                        ms, h_first, h_tables, h_counts = route.run(mq, exf, bqf)
                        H[name + sfx].append(ms)
                        assert np.array_equal(h_first, r.first) and np.array_equal(h_tables, r.tables) and np.array_equal(h_counts, r.site_counts), \
                            "the host route gives other counts"
            if other:
                other.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for k, v in T.items():
        if v["call_ms"]:
            out[k] = {q: spread(x) for q, x in v.items()}
    for k, v in H.items():
        out[k] = spread(v)
    for key, r in first_l.items():
        n_part = np.diff(r.first.astype(np.int64))
        status = [0, 0, 0, 0]
        for i in range(sites.shape[0]):
            for p in range(int(r.first[i]), int(r.first[i + 1])):
                status[V.link_summarise(r.site_counts[i], r.site_counts[i + 1 + p - int(r.first[i])], r.tables[p], md, 3, 500)["status"]] += 1
        out[key].update(pairs=int(r.first[-1]), anchors_without_partners=int((n_part == 0).sum()), most_partners=int(n_part.max()),
                        reads_in_tables=int(r.tables.astype(np.uint64).sum()), reads_per_site_median=float(np.median(r.site_counts.sum(1))),
                        status={s: status[i] for i, s in enumerate(V.LINK_STATUS_NAMES)},
                        bytes_back=int(r.first.nbytes + r.tables.nbytes + r.site_counts.nbytes))
    out["speedup_call_over_host_1_thread"] = out["host_1_thread_filtered_ms"]["median"] / out["link_counts_filtered"]["call_ms"]["median"]
    out["speedup_call_over_host_threads"] = out["host_threads_filtered_ms"]["median"] / out["link_counts_filtered"]["call_ms"]["median"]
    out["speedup_kernel_over_host_1_thread"] = out["host_1_thread_filtered_ms"]["median"] / out["link_counts_filtered"]["kernel_ms"]["median"]
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
