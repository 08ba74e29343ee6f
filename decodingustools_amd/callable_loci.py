"""Host-side mirror of the reference's `callable_loci` module (src/callable_loci/) on the
MI355X engine.  Names follow the reference:

    CallableOptions          options.rs:2-38 (CLI defaults cli.rs:34-60)
    CalledState              types.rs:36-43
    CallableProfiler         profilers/callable_profiler.rs:11-160
    ContigProfiler           profilers/contig_profiler.rs:7-158
    process_single_contig    mod.rs:44-147

Everything numeric happens in libcallable_hip.so (HIP kernels + C++ host mirror); this file is
a thin ctypes layer over include/callable_loci.h and include/dut_coverage.h.
"""
import ctypes as C
import enum
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib
from .records import ContigRecords


class CalledState(enum.IntEnum):
    REF_N = 0
    CALLABLE = 1
    NO_COVERAGE = 2
    LOW_COVERAGE = 3
    EXCESSIVE_COVERAGE = 4
    POOR_MAPPING_QUALITY = 5


class EngineError(RuntimeError):
    """Box<dyn Error> of the reference, with the engine's status code."""

    def __init__(self, status, message):
        super().__init__(f"{message} (cl_status {status})")
        self.status = status


@dataclass
class CallableOptions:
    """options.rs:2-11; defaults are the CLI's (cli.rs:34-60)."""
    min_depth: int = 4
    max_depth: int = 500
    min_mapping_quality: int = 10
    min_base_quality: int = 20
    min_depth_for_low_mapq: int = 10
    max_low_mapq: int = 1
    max_low_mapq_fraction: float = 0.1
    selected_contigs: Optional[List[str]] = None

    def with_contigs(self, contigs):
        self.selected_contigs = list(contigs) if contigs is not None else None
        return self

    def to_c(self):
        return _lib.cl_options(self.min_depth, self.max_depth, self.min_mapping_quality,
                               self.min_base_quality, self.min_depth_for_low_mapq, self.max_low_mapq,
                               float(self.max_low_mapq_fraction))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _records_c(rec: ContigRecords):
    r = _lib.dut_records()
    r.n = rec.n
    r.pos = _ptr(rec.pos); r.flag = _ptr(rec.flag); r.mapq = _ptr(rec.mapq)
    r.cigar_off = _ptr(rec.cigar_off); r.cigar = _ptr(rec.cigar)
    r.qual_off = _ptr(rec.qual_off); r.qual = _ptr(rec.qual)
    r.qname_off = _ptr(rec.qname_off); r.qname = _ptr(rec.qname)
    return r


def _site_quals(rec: ContigRecords):
    q = _lib.cl_site_quals()
    q.n_reads = rec.n
    q.flag = _ptr(rec.flag); q.qual_off = _ptr(rec.qual_off); q.qual = _ptr(rec.qual); q.seq_off = _ptr(rec.seq_off)
    return q


def _filter_ref(filter):
    """filter=(exclude_flags, use_base_quality) of a scan mode as the cl_scan_filter argument; None: the unfiltered form."""
    return None if filter is None else C.byref(_lib.cl_scan_filter(int(filter[0]), 1 if filter[1] else 0, 0))


def site_pass_bits(rec: ContigRecords, min_base_quality) -> np.ndarray:
    """cl_debug_site_pass_bits (host only): the attachment's pass bits as uint64 words, bit i of word w <-> base 64 w + i
    in the numbering of rec.seq_off."""
    n_words = (int(rec.seq_off[-1]) + 63) // 64
    out = np.zeros(n_words, np.uint64)
    q = _site_quals(rec)
    st = _lib.load().cl_debug_site_pass_bits(C.byref(q), int(min_base_quality), _ptr(out), n_words)
    if st != 0:
        raise EngineError(st, "invalid attachment")
    return out


class Engine:
    """One device context (cl_ctx): one per GPU, driven by one host thread."""

    def __init__(self, options: CallableOptions, device_id: int = 0, stream: int = 0):
        self._lib = _lib.load()
        self.options = options
        self._opt_c = options.to_c()
        h = C.c_void_p()
        st = self._lib.cl_create(C.byref(self._opt_c), device_id, C.c_void_p(stream) if stream else None,
                                 C.byref(h))
        if st != 0:
            raise EngineError(st, "cl_create failed: no usable HIP device (the engine has no CPU fallback)")
        self._h = h
        self.device_id = device_id
        self._keep = []

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st):
        if st != 0:
            raise EngineError(st, self._lib.cl_last_error(self._h).decode())

    # ---- the C ABI, one to one ----
    def contig_begin(self, tid, contig_len, ref: Optional[np.ndarray]):
        ref = np.ascontiguousarray(ref, dtype=np.uint8) if ref is not None else np.zeros(0, np.uint8)
        self._check(self._lib.cl_contig_begin(self._h, tid, contig_len, _ptr(ref), ref.shape[0]))

    def contig_reserve(self, n_reads, n_cigar_ops, n_qual_bytes):
        self._check(self._lib.cl_contig_reserve(self._h, n_reads, n_cigar_ops, n_qual_bytes))

    def push_reads(self, pos, mapq, cigar_off, cigar, qual_off, qual):
        t = _lib.cl_read_tile()
        arrs = [np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(mapq, np.uint8),
                np.ascontiguousarray(cigar_off, np.uint32), np.ascontiguousarray(cigar, np.uint32),
                np.ascontiguousarray(qual_off, np.uint64), np.ascontiguousarray(qual, np.uint8)]
        t.n_reads = arrs[0].shape[0]
        t.pos, t.mapq, t.cigar_off, t.cigar, t.qual_off, t.qual = [_ptr(a) for a in arrs]
        self._check(self._lib.cl_push_reads(self._h, C.byref(t)))

    def push_reads_bits(self, pos, mapq, cigar_off, cigar, qual_off, pass_bits, pass_sum):
        """cl_push_reads_bits: the packed pass-bitmask variant (the caller has taken the base-quality test)."""
        t = _lib.cl_read_tile_bits()
        arrs = [np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(mapq, np.uint8),
                np.ascontiguousarray(cigar_off, np.uint32), np.ascontiguousarray(cigar, np.uint32),
                np.ascontiguousarray(qual_off, np.uint64), np.ascontiguousarray(pass_bits, np.uint64),
                np.ascontiguousarray(pass_sum, np.uint32)]
        t.n_reads = arrs[0].shape[0]
        t.pos, t.mapq, t.cigar_off, t.cigar, t.qual_off, t.pass_bits, t.pass_sum = [_ptr(a) for a in arrs]
        self._check(self._lib.cl_push_reads_bits(self._h, C.byref(t)))

    def contig_abort(self):
        self._check(self._lib.cl_contig_abort(self._h))

    def contig_upload(self):
        self._check(self._lib.cl_contig_upload(self._h))

    def contig_run(self):
        self._check(self._lib.cl_contig_run(self._h))

    def sync(self):
        self._check(self._lib.cl_sync(self._h))

    def _result(self, s, iv, n):
        n = n.value
        if n:
            arr = np.ctypeslib.as_array(C.cast(iv, C.POINTER(C.c_uint32)), shape=(n, 3)).copy()
        else:
            arr = np.zeros((0, 3), dtype=np.uint32)
        return ContigResult(summary=s, intervals=arr)

    def contig_collect(self):
        s = _lib.cl_contig_summary(); iv = C.POINTER(_lib.cl_interval)(); n = C.c_size_t()
        self._check(self._lib.cl_contig_collect(self._h, C.byref(s), C.byref(iv), C.byref(n)))
        return self._result(s, iv, n)

    def contig_finish(self):
        s = _lib.cl_contig_summary(); iv = C.POINTER(_lib.cl_interval)(); n = C.c_size_t()
        self._check(self._lib.cl_contig_finish(self._h, C.byref(s), C.byref(iv), C.byref(n)))
        return self._result(s, iv, n)

    def device_summary(self):
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._lib.cl_device_summary(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_profiling(self, on=True):
        self._check(self._lib.cl_set_profiling(self._h, 1 if on else 0))

    def kernel_ms(self):
        ms = (C.c_double * _lib.CL_K_COUNT)(); n = C.c_uint64()
        self._check(self._lib.cl_get_kernel_ms(self._h, ms, C.byref(n)))
        return dict(zip(_lib.CL_K_NAMES, list(ms))), n.value

    def reset_kernel_ms(self):
        self._check(self._lib.cl_reset_kernel_ms(self._h))

    def contig_bytes(self):
        a = C.c_uint64(); b = C.c_uint64()
        self._check(self._lib.cl_contig_bytes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def contig_layout(self):
        """What is resident for the uploaded contig (cl_layout_info as a dict)."""
        li = _lib.cl_layout_info()
        self._check(self._lib.cl_contig_layout(self._h, C.byref(li)))
        return {k: int(getattr(li, k)) for k, _ in li._fields_}

    def debug_depths(self, extent):
        raw = np.zeros(extent, np.uint32); qc = np.zeros(extent, np.uint32)
        low = np.zeros(extent, np.uint32); st = np.zeros(extent, np.uint8)
        self._check(self._lib.cl_debug_depths(self._h, _ptr(raw), _ptr(qc), _ptr(low), _ptr(st), extent))
        return raw, qc, low, st

    def site_pileup(self, min_quality, contig_len, ref_len, rec: ContigRecords, sites):
        sites = np.ascontiguousarray(sites, np.uint32)
        hist = np.zeros((sites.shape[0], 16), np.uint32)
        t = _lib.cl_site_tile()
        t.n_reads = rec.n
        t.pos = _ptr(rec.pos); t.mapq = _ptr(rec.mapq); t.cigar_off = _ptr(rec.cigar_off)
        t.cigar = _ptr(rec.cigar); t.seq_off = _ptr(rec.seq_off); t.seq4 = _ptr(rec.seq4)
        self._check(self._lib.cl_site_pileup(self._h, min_quality, contig_len, ref_len, C.byref(t),
                                             _ptr(sites), sites.shape[0], _ptr(hist)))
        return hist

    def _site_tile(self, rec: ContigRecords):
        t = _lib.cl_site_tile()
        t.n_reads = rec.n
        t.pos = _ptr(rec.pos); t.mapq = _ptr(rec.mapq); t.cigar_off = _ptr(rec.cigar_off)
        t.cigar = _ptr(rec.cigar); t.seq_off = _ptr(rec.seq_off); t.seq4 = _ptr(rec.seq4)
        return t

    def site_upload(self, contig_len, ref_len, rec: ContigRecords):
        """The tile goes to HBM once and stays resident for any number of site_run calls."""
        t = self._site_tile(rec)
        self._check(self._lib.cl_site_upload(self._h, contig_len, ref_len, C.byref(t)))

    def site_run(self, min_quality, sites):
        sites = np.ascontiguousarray(sites, np.uint32)
        hist = np.zeros((sites.shape[0], 16), np.uint32)
        self._check(self._lib.cl_site_run(self._h, min_quality, _ptr(sites), sites.shape[0], _ptr(hist)))
        return hist

    def site_pileup_stats(self):
        """(kernel milliseconds, algorithmic bytes) of the last site_pileup."""
        ms = C.c_double(); b = C.c_uint64()
        self._check(self._lib.cl_site_pileup_stats(self._h, C.byref(ms), C.byref(b)))
        return ms.value, b.value

    def _site_scan_mode(self, fn, head, ref, start, end, result_type, dtype, n_field):
        """A compacting scan of the resident tile: fn(ctx, *head, ref, ref_len, start, end, out) -- head: what the entry point
        takes in front of the reference.  (the C result, its n_field candidates as a structured array of dtype, a copy)."""
        ref = np.ascontiguousarray(ref, np.uint8) if ref is not None else np.zeros(0, np.uint8)
        if end is None:
            end = ref.shape[0]
        r = result_type()
        self._check(fn(self._h, *head, _ptr(ref), ref.shape[0], int(start), int(end), C.byref(r)))
        n = int(getattr(r, n_field))
        cand = np.zeros(n, dtype)
        if n:
            C.memmove(cand.ctypes.data, r.candidates, n * dtype.itemsize)
        return r, cand

    def _site_scan(self, fn, head, ref, start, end, result_type, dtype):
        r, cand = self._site_scan_mode(fn, head, ref, start, end, result_type, dtype, "n_variant")
        return ScanResult(start=int(r.start), end=int(r.end), low_depth=int(r.n_low_depth), mixed=int(r.n_mixed),
                          uncomparable=int(r.n_uncomparable), match=int(r.n_match), variant=cand.shape[0], candidates=cand)

    def site_scan(self, min_quality, min_depth, ref, start=0, end=None):
        """cl_site_scan over [start, end) of the resident tile (end=None: the length of `ref`, which must be the ref_len
        given to site_upload): a ScanResult with the five class counts and the candidates as a structured array."""
        return self._site_scan(self._lib.cl_site_scan, (int(min_quality), int(min_depth)), ref, start, end, _lib.cl_scan_result, SCAN_CANDIDATE)

    def site_scan_counts(self, min_quality, start, end):
        """cl_site_scan_counts: (end - start, 5) uint32 -- A, C, G, T, depth -- for at most CL_SCAN_MAX_DENSE positions."""
        counts = np.zeros((max(int(end) - int(start), 0), 5), np.uint32)
        self._check(self._lib.cl_site_scan_counts(self._h, int(min_quality), int(start), int(end), _ptr(counts)))
        return counts

    def site_attach_quals(self, rec: ContigRecords, min_base_quality):
        """cl_site_attach_quals: the flags and, per base, (qual >= min_base_quality) of `rec` -- the records the resident
        tile was uploaded from -- for site_scan_ex / site_scan_counts_ex.  Replaces an earlier attachment."""
        q = _site_quals(rec)
        self._check(self._lib.cl_site_attach_quals(self._h, C.byref(q), int(min_base_quality)))

    def site_scan_ex(self, min_quality, min_depth, ref, exclude_flags=0, use_base_quality=False, start=0, end=None):
        """cl_site_scan_ex: site_scan under a flag mask and (use_base_quality) the attachment's pass bits; the candidates
        (SCAN_CANDIDATE_EX) also carry alt_fwd, alt_rev, ref_fwd, ref_rev."""
        filt = _lib.cl_scan_filter(int(exclude_flags), 1 if use_base_quality else 0, 0)
        return self._site_scan(self._lib.cl_site_scan_ex, (int(min_quality), int(min_depth), C.byref(filt)), ref, start, end, _lib.cl_scan_result_ex,
                               SCAN_CANDIDATE_EX)

    def site_scan_counts_ex(self, min_quality, start, end, exclude_flags=0, use_base_quality=False):
        """cl_site_scan_counts_ex: (end - start, 9) uint32 -- A+ A- C+ C- G+ G- T+ T- depth (+ forward, - reverse)."""
        counts = np.zeros((max(int(end) - int(start), 0), 9), np.uint32)
        f = _lib.cl_scan_filter(int(exclude_flags), 1 if use_base_quality else 0, 0)
        self._check(self._lib.cl_site_scan_counts_ex(self._h, int(min_quality), C.byref(f), int(start), int(end), _ptr(counts)))
        return counts

    def site_scan_minor(self, min_quality, min_depth, min_minor_count, min_minor_per_10k, ref, start=0, end=None, filter=None):
        """cl_site_scan_minor over [start, end) of the resident tile: positions where a second base of A C G T stands beside
        the most frequent one.  filter: None for the unfiltered form, else (exclude_flags, use_base_quality) of the
        attachment.  A MinorResult: the three class counts, the candidates (MINOR_CANDIDATE) and the kernel's milliseconds."""
        prm = _lib.cl_minor_params(int(min_depth), int(min_minor_count), int(min_minor_per_10k))
        r, cand = self._site_scan_mode(self._lib.cl_site_scan_minor, (int(min_quality), _filter_ref(filter), C.byref(prm)), ref, start, end,
                                       _lib.cl_minor_result, MINOR_CANDIDATE, "n_minor")
        return MinorResult(start=int(r.start), end=int(r.end), low_depth=int(r.n_low_depth), single=int(r.n_single), minor=cand.shape[0],
                           candidates=cand, kernel_ms=self.site_scan_stats()[0])

    def site_scan_dels(self, min_quality, min_depth, min_del_count, min_del_per_10k, ref, start=0, end=None, filter=None):
        """cl_site_scan_dels over [start, end) of the resident tile: positions that the reads delete (a D operation over
        them), beside the scan's depth.  filter: None for the unfiltered form, else (exclude_flags, use_base_quality) of the
        attachment.  A DelResult: the three class counts, the candidates (DEL_CANDIDATE) and the kernel's milliseconds."""
        prm = _lib.cl_del_params(int(min_depth), int(min_del_count), int(min_del_per_10k))
        r, cand = self._site_scan_mode(self._lib.cl_site_scan_dels, (int(min_quality), _filter_ref(filter), C.byref(prm)), ref, start, end,
                                       _lib.cl_del_result, DEL_CANDIDATE, "n_deleted")
        return DelResult(start=int(r.start), end=int(r.end), low_depth=int(r.n_low_depth), kept=int(r.n_kept), deleted=cand.shape[0],
                         candidates=cand, kernel_ms=self.site_scan_stats()[0])

    def site_scan_ins(self, min_quality, min_depth, min_ins_count, min_ins_per_10k, ref, start=0, end=None, filter=None):
        """cl_site_scan_ins over [start, end) of the resident tile: positions behind whose base the reads insert something
        (an I operation anchored there), beside the scan's depth, and what they insert.  filter: None for the unfiltered
        form, else (exclude_flags, use_base_quality) of the attachment.  An InsResult: the three class counts, the
        candidates (INS_CANDIDATE), one observation per counting insertion at a candidate (INS_OBS, by pos, len, key,
        strand) and the milliseconds of both launches."""
        prm = _lib.cl_ins_params(int(min_depth), int(min_ins_count), int(min_ins_per_10k))
        r, cand = self._site_scan_mode(self._lib.cl_site_scan_ins, (int(min_quality), _filter_ref(filter), C.byref(prm)), ref, start, end,
                                       _lib.cl_ins_result, INS_CANDIDATE, "n_inserted")
        obs = np.zeros(int(r.n_obs), INS_OBS)
        if obs.shape[0]:
            C.memmove(obs.ctypes.data, r.obs, obs.shape[0] * INS_OBS.itemsize)
        return InsResult(start=int(r.start), end=int(r.end), low_depth=int(r.n_low_depth), kept=int(r.n_kept), inserted=cand.shape[0],
                         candidates=cand, observations=obs, kernel_ms=self.site_scan_stats()[0])

    def site_scan_consensus(self, min_quality, min_depth, min_del_count, min_del_per_10k, ref, start=0, end=None, filter=None):
        """cl_site_scan_consensus over [start, end) of the resident tile: one byte per position -- the called base, '-' where
        the deletion rule holds, 'N' for a mixed column, 'n' for a shallow one.  filter: None for the unfiltered form, else
        (exclude_flags, use_base_quality) of the attachment.  There is no limit on end - start.  A ConsResult: the five class
        counts, the bytes as a uint8 array (a copy) and the kernel's milliseconds."""
        prm = _lib.cl_cons_params(int(min_depth), int(min_del_count), int(min_del_per_10k))
        ref = np.ascontiguousarray(ref, np.uint8) if ref is not None else np.zeros(0, np.uint8)
        if end is None:
            end = ref.shape[0]
        r = _lib.cl_cons_result()
        self._check(self._lib.cl_site_scan_consensus(self._h, int(min_quality), _filter_ref(filter), C.byref(prm), _ptr(ref), ref.shape[0], int(start),
                                                     int(end), C.byref(r)))
        n = int(r.end) - int(r.start)
        cons = np.zeros(n, np.uint8)
        if n:
            C.memmove(cons.ctypes.data, r.cons, n)
        return ConsResult(start=int(r.start), end=int(r.end), low_depth=int(r.n_low_depth), deleted=int(r.n_deleted), no_call=int(r.n_no_call),
                          ref=int(r.n_ref), alt=int(r.n_alt), cons=cons, kernel_ms=self.site_scan_stats()[0])

    def site_str_lengths(self, loci, flank, min_quality, filter=None):
        """cl_site_str_lengths over the resident tile: per locus [start, end) of `loci` (an (n, 2) array, 0-based half open,
        in any order) the histogram of delta = bases between the two flanks of `flank` matched bases - (end - start) over the
        reads that span it, and the reads that take part without spanning it.  filter: None for one strand, else
        (exclude_flags, False) of the attachment -- base qualities take no part.  A StrResult: hist of shape
        (n, strands, 128), partial (n), copies, and the kernel's milliseconds."""
        loci = np.ascontiguousarray(loci, np.uint32).reshape(-1, 2)
        r = _lib.cl_str_result()
        self._check(self._lib.cl_site_str_lengths(self._h, int(min_quality), _filter_ref(filter), int(flank), _ptr(loci) if loci.shape[0] else None,
                                                  loci.shape[0], C.byref(r)))
        n, strands = int(r.n_loci), int(r.strands)
        hist = np.zeros((n, strands, _lib.CL_STR_BINS), np.uint32)
        partial = np.zeros(n, np.uint32)
        if n:
            C.memmove(hist.ctypes.data, r.hist, hist.nbytes)
            C.memmove(partial.ctypes.data, r.partial, partial.nbytes)
        return StrResult(hist=hist, partial=partial, kernel_ms=self.site_scan_stats()[0])

    def site_error_profile(self, n_cycles, min_quality, ref, start=0, end=None, filter=None):
        """cl_site_error_profile over [start, end) of the resident tile: substitutions by reference base and read base, the
        same by distance from either end of the read, and insertion and deletion events by the same distances.  filter:
        None for the unfiltered form (every read forward), else (exclude_flags, use_base_quality) of the attachment.  An
        ErrorProfile of numpy uint64 arrays (copies), the scalars and the two launches' milliseconds."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        end = ref.shape[0] if end is None else end
        r = _lib.cl_ep_result()
        self._check(self._lib.cl_site_error_profile(self._h, int(min_quality), _filter_ref(filter), int(n_cycles), _ptr(ref), ref.shape[0], int(start), int(end),
                                                    C.byref(r)))
        return ErrorProfile.from_c(r, kernel_ms=self.site_scan_stats()[0])

    def site_link_counts(self, sites, max_dist, max_partners, min_quality, filter=None):
        """cl_site_link_counts over the resident tile: for `sites` (0-based positions, strictly ascending) the pair set --
        anchor i with the next sites, at most max_partners of them, no further than max_dist away -- and per pair the 6 x 6
        table of the classes A C G T del other that one read observes at both sites; per site its six counts.  filter: None
        for the unfiltered form, else (exclude_flags, use_base_quality) of the attachment.  A LinkResult of numpy uint32
        arrays (copies) and the kernel's milliseconds."""
        sites = np.ascontiguousarray(sites, np.uint32).reshape(-1)
        r = _lib.cl_link_result()
        self._check(self._lib.cl_site_link_counts(self._h, int(min_quality), _filter_ref(filter), _ptr(sites) if sites.shape[0] else None, sites.shape[0],
                                                  int(max_dist), int(max_partners), C.byref(r)))
        n, n_pairs = int(r.n_sites), int(r.n_pairs)
        first = np.zeros(n + 1, np.uint32)
        tables = np.zeros((n_pairs, _lib.CL_LINK_CLASSES, _lib.CL_LINK_CLASSES), np.uint32)
        site_counts = np.zeros((n, _lib.CL_LINK_CLASSES), np.uint32)
        C.memmove(first.ctypes.data, r.first, first.nbytes)
        if n_pairs:
            C.memmove(tables.ctypes.data, r.tables, tables.nbytes)
        if n:
            C.memmove(site_counts.ctypes.data, r.site_counts, site_counts.nbytes)
        return LinkResult(first=first, tables=tables, site_counts=site_counts, kernel_ms=self.site_scan_stats()[0])

    def site_error_profile_stats(self):
        """(table kernel milliseconds, slice sum milliseconds) of the last site_error_profile."""
        a = C.c_double(); b = C.c_double()
        self._check(self._lib.cl_site_error_profile_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def site_scan_ins_stats(self):
        """(window scan milliseconds, allele launch milliseconds) of the last site_scan_ins."""
        a = C.c_double(); b = C.c_double()
        self._check(self._lib.cl_site_scan_ins_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def site_scan_stats(self):
        """(kernel milliseconds, algorithmic bytes) of the last site_scan / site_scan_counts, filtered or not."""
        ms = C.c_double(); b = C.c_uint64()
        self._check(self._lib.cl_site_scan_stats(self._h, C.byref(ms), C.byref(b)))
        return ms.value, b.value

    def depth_profile(self, n_bins=1001, window=0):
        """The depth distribution of the resident contig, reduced on the device (cl_contig_depth_profile): a
        DepthProfile of numpy uint64 arrays (copies).  window = 0: no window table."""
        p = _lib.cl_depth_profile()
        self._check(self._lib.cl_contig_depth_profile(self._h, int(n_bins), int(window), C.byref(p)))

        def arr(ptr, n):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n and ptr else np.zeros(0, np.uint64)
        nw = int(p.n_windows)
        ms = C.c_double()
        self._check(self._lib.cl_contig_depth_profile_ms(self._h, C.byref(ms)))
        return DepthProfile(n_bins=int(p.n_bins), window=int(p.window), n_windows=nw, extent=int(p.extent),
                            sum_raw=int(p.sum_raw), sum_qc=int(p.sum_qc), hist_raw=arr(p.hist_raw, int(p.n_bins)),
                            hist_qc=arr(p.hist_qc, int(p.n_bins)), win_raw=arr(p.win_raw, nw) if window else None,
                            win_qc=arr(p.win_qc, nw) if window else None, kernel_ms=float(ms.value))

    def gc_bias(self, ref, window=100, max_invalid=4):
        """Both depths of the resident contig by the GC content of `ref` (bytes, or a numpy uint8 array; None or empty:
        every position is skipped) in a window of `window` positions centred on each position (cl_contig_gc_bias): a
        GcBias of numpy uint64 arrays.  Positions with more than max_invalid invalid bases in their window are skipped.
        Every call packs and uploads the reference's two bit planes again."""
        if ref is None:
            r = np.zeros(0, np.uint8)
        elif isinstance(ref, (bytes, bytearray, memoryview)):
            r = np.frombuffer(bytes(ref), np.uint8)
        else:
            r = np.ascontiguousarray(ref, dtype=np.uint8).reshape(-1)
        if not (0 <= int(window) <= 0xFFFFFFFF and 0 <= int(max_invalid) <= 0xFFFFFFFF):
            raise EngineError(-1, "gc_bias: window or max_invalid outside [0, 2^32 - 1]")
        g = _lib.cl_gc_bias()
        self._check(self._lib.cl_contig_gc_bias(self._h, _ptr(r) if r.size else None, int(r.size), int(window), int(max_invalid), C.byref(g)))
        ms, up = C.c_double(), C.c_double()
        self._check(self._lib.cl_contig_gc_bias_ms(self._h, C.byref(ms), C.byref(up)))
        return GcBias._from_c(g, float(ms.value), float(up.value))

    def depth_runs(self, kind="raw", edges=None):
        """The per-position depth of the resident contig as runs of equal value, built on the device
        (cl_contig_depth_runs): a DepthRuns of numpy uint32 arrays (copies).  kind: "raw" or "qc" (or the ABI's 0 / 1);
        edges: None or empty for the depth itself, else ascending band edges -- the value is the number of edges <= depth."""
        k = _lib.CL_DEPTH_KINDS.get(kind, kind)
        e = np.ascontiguousarray(edges if edges is not None else [], np.uint32)
        r = _lib.cl_depth_runs()
        self._check(self._lib.cl_contig_depth_runs(self._h, int(k), e.ctypes.data_as(C.POINTER(C.c_uint32)) if e.size else None,
                                                   int(e.size), C.byref(r)))
        n = int(r.n_runs)

        def arr(ptr):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        ms = C.c_double()
        self._check(self._lib.cl_contig_depth_runs_ms(self._h, C.byref(ms)))
        return DepthRuns(kind=int(r.kind), edges=e.copy(), extent=int(r.extent), n_runs=n, start=arr(r.start), value=arr(r.value),
                         kernel_ms=float(ms.value))

    def target_stats(self, starts, ends, thresholds=(1, 10, 20, 30)):
        """Depth and callable-base summaries of the resident contig over the targets [starts[i], ends[i]), 0-based half
        open, in any order and overlapping at will (cl_contig_targets): a TargetStats of numpy arrays (copies), one entry
        per target in the order given.  thresholds: up to 8 ascending depths, the first at least 1.  The contig must have
        been collected (contig_collect or contig_finish) since its last run."""
        def u32(v, what):
            a = np.asarray(v)
            if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
                raise EngineError(-1, f"target_stats: {what} outside [0, 2^32 - 1]")
            return np.ascontiguousarray(a, np.uint32).reshape(-1)
        s, e, t = u32(starts, "a start"), u32(ends, "an end"), u32(thresholds, "a threshold")
        if s.size != e.size:
            raise EngineError(-1, "target_stats: starts and ends differ in length")
        u32p = C.POINTER(C.c_uint32)
        out = C.POINTER(_lib.cl_target_stats)()
        self._check(self._lib.cl_contig_targets(self._h, s.ctypes.data_as(u32p) if s.size else None, e.ctypes.data_as(u32p) if e.size else None,
                                                int(s.size), t.ctypes.data_as(u32p) if t.size else None, int(t.size), C.byref(out)))
        n = int(s.size)
        rec = (np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(n * TARGET_STATS.itemsize,)).view(TARGET_STATS).copy()
               if n else np.zeros(0, TARGET_STATS))
        ms = C.c_double()
        parts = (C.c_double * 3)()
        self._check(self._lib.cl_contig_targets_ms(self._h, C.byref(ms), parts))
        return TargetStats.from_records(rec, t.copy(), float(ms.value), tuple(float(x) for x in parts))

    def target_order(self, starts, ends):
        """Minimum, quartiles and maximum of the raw and the quality-filtered depth of the resident contig over the targets
        [starts[i], ends[i]), 0-based half open, in any order and overlapping at will (cl_contig_target_order): a
        TargetOrder of numpy arrays (copies), one entry per target in the order given.  A quartile is an element of the
        sorted depths ((j * len + 3) // 4 - 1, the lower middle value for the median of an even length), a whole number.
        The contig must have been run; it need not have been collected."""
        def u32(v, what):
            a = np.asarray(v)
            if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
                raise EngineError(-1, f"target_order: {what} outside [0, 2^32 - 1]")
            return np.ascontiguousarray(a, np.uint32).reshape(-1)
        s, e = u32(starts, "a start"), u32(ends, "an end")
        if s.size != e.size:
            raise EngineError(-1, "target_order: starts and ends differ in length")
        u32p = C.POINTER(C.c_uint32)
        out = C.POINTER(_lib.cl_target_order)()
        self._check(self._lib.cl_contig_target_order(self._h, s.ctypes.data_as(u32p) if s.size else None,
                                                     e.ctypes.data_as(u32p) if e.size else None, int(s.size), C.byref(out)))
        n = int(s.size)
        rec = (np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(n * TARGET_ORDER.itemsize,)).view(TARGET_ORDER).copy()
               if n else np.zeros(0, TARGET_ORDER))
        ms = C.c_double()
        rounds = C.c_uint32()
        self._check(self._lib.cl_contig_target_order_ms(self._h, C.byref(ms), C.byref(rounds)))
        return TargetOrder.from_records(rec, float(ms.value), int(rounds.value))


# cl_scan_candidate as a numpy record: pos is 1-based, ref and alt are ASCII codes
SCAN_CANDIDATE = np.dtype([("pos", np.uint32), ("ref", np.uint8), ("alt", np.uint8), ("pad", np.uint8, (2,)), ("a", np.uint32),
                           ("c", np.uint32), ("g", np.uint32), ("t", np.uint32), ("depth", np.uint32)])
# cl_scan_candidate_ex: a c g t depth over both strands, the alternative and reference base by strand
SCAN_CANDIDATE_EX = np.dtype(SCAN_CANDIDATE.descr + [("alt_fwd", np.uint32), ("alt_rev", np.uint32), ("ref_fwd", np.uint32),
                                                     ("ref_rev", np.uint32)])


# cl_minor_candidate: major and minor are ASCII codes; the strand counts are 0 in the unfiltered form
MINOR_CANDIDATE = np.dtype([("pos", np.uint32), ("ref", np.uint8), ("major", np.uint8), ("minor", np.uint8), ("pad", np.uint8),
                            ("a", np.uint32), ("c", np.uint32), ("g", np.uint32), ("t", np.uint32), ("depth", np.uint32),
                            ("major_fwd", np.uint32), ("major_rev", np.uint32), ("minor_fwd", np.uint32), ("minor_rev", np.uint32)])


# cl_del_candidate: the strand counts are 0 in the unfiltered form
DEL_CANDIDATE = np.dtype([("pos", np.uint32), ("ref", np.uint8), ("pad", np.uint8, (3,)), ("del", np.uint32), ("depth", np.uint32),
                          ("del_fwd", np.uint32), ("del_rev", np.uint32), ("depth_fwd", np.uint32), ("depth_rev", np.uint32)])


# cl_ins_candidate: pos is the anchor; the strand counts are 0 in the unfiltered form
INS_CANDIDATE = np.dtype([("pos", np.uint32), ("ref", np.uint8), ("pad", np.uint8, (3,)), ("ins", np.uint32), ("depth", np.uint32),
                          ("ins_fwd", np.uint32), ("ins_rev", np.uint32), ("depth_fwd", np.uint32), ("depth_rev", np.uint32)])

# cl_ins_obs: key = the first 32 inserted 4-bit codes, base j in key[j // 16] at bits 60 - 4 * (j % 16)
INS_OBS = np.dtype([("pos", np.uint32), ("len", np.uint32), ("key", np.uint64, (2,)), ("strand", np.uint32), ("pad", np.uint32)])


@dataclass
class ErrorProfile:
    """cl_ep_result (include/callable_loci.h): total[f, t], from5[d, f, t] and from3[d, f, t] count aligned bases with
    reference base f and read base t (A C G T, in the orientation the molecule was sequenced in) at distance d from the
    read's 5' and 3' end; ins5, ins3, del5, del3[d] count insertion and deletion events by the same distances."""
    start: int
    end: int
    n_cycles: int
    reads: int
    bases: int
    uncomparable: int
    ins: int
    ins_bases: int
    dels: int
    del_bases: int
    total: np.ndarray
    from5: np.ndarray
    from3: np.ndarray
    ins5: np.ndarray
    ins3: np.ndarray
    del5: np.ndarray
    del3: np.ndarray
    kernel_ms: float = 0.0

    @staticmethod
    def from_c(r, kernel_ms=0.0):
        c = int(r.n_cycles)

        def arr(ptr, n):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy().astype(np.uint64)
        return ErrorProfile(start=int(r.start), end=int(r.end), n_cycles=c, reads=int(r.n_reads), bases=int(r.n_bases), uncomparable=int(r.n_uncomparable),
                            ins=int(r.n_ins), ins_bases=int(r.ins_bases), dels=int(r.n_del), del_bases=int(r.del_bases),
                            total=np.array(list(r.total), np.uint64).reshape(4, 4), from5=arr(r.from5, 16 * c).reshape(c, 4, 4),
                            from3=arr(r.from3, 16 * c).reshape(c, 4, 4), ins5=arr(r.ins5, c), ins3=arr(r.ins3, c), del5=arr(r.del5, c), del3=arr(r.del3, c),
                            kernel_ms=kernel_ms)

    def to_c(self):
        """(cl_ep_result, the array its pointers are set into -- keep it alive as long as the record)."""
        c = int(self.n_cycles)
        tab = np.concatenate([np.ascontiguousarray(a, np.uint64).reshape(-1) for a in (self.from5, self.from3, self.ins5, self.ins3, self.del5, self.del3)])
        if tab.shape[0] != 36 * c or np.asarray(self.total).size != 16:
            raise ValueError("the tables do not have n_cycles cycles")
        r = _lib.cl_ep_result()
        r.start, r.end, r.n_cycles = int(self.start), int(self.end), c
        r.n_reads, r.n_bases, r.n_uncomparable = int(self.reads), int(self.bases), int(self.uncomparable)
        r.n_ins, r.ins_bases, r.n_del, r.del_bases = int(self.ins), int(self.ins_bases), int(self.dels), int(self.del_bases)
        for k, v in enumerate(np.asarray(self.total, np.uint64).reshape(-1)):
            r.total[k] = int(v)
        p = tab.ctypes.data_as(C.POINTER(C.c_uint64))
        at = lambda o: C.cast(C.addressof(p.contents) + 8 * o, C.POINTER(C.c_uint64))   # noqa: E731
        r.from5, r.from3, r.ins5, r.ins3, r.del5, r.del3 = at(0), at(16 * c), at(32 * c), at(33 * c), at(34 * c), at(35 * c)
        return r, tab

    def tables_equal(self, other):
        return (all(getattr(self, k) == getattr(other, k) for k in ("start", "end", "n_cycles", "reads", "bases", "uncomparable", "ins", "ins_bases", "dels", "del_bases"))
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("total", "from5", "from3", "ins5", "ins3", "del5", "del3")))


@dataclass
class LinkResult:
    """cl_link_result (include/callable_loci.h): first[i] = the CSR offset of anchor i's pairs (first[n] = n_pairs), pair
    first[i] + (j - i - 1) being (i, j); tables[pair, ca, cb] = the reads that take part for the anchor and observe class ca
    there and cb at the partner; site_counts[i, c] = the reads that observe class c at site i.  Classes: A C G T del other."""
    first: np.ndarray
    tables: np.ndarray
    site_counts: np.ndarray
    kernel_ms: float = 0.0


@dataclass
class StrResult:
    """cl_str_result (include/callable_loci.h): hist[i, strand, delta + 63] = the reads that span locus i with that delta
    (bin 127: every delta outside [-63, 63]; strand 0 forward, 1 reverse under a filter), partial[i] = the reads that take
    part without spanning it."""
    hist: np.ndarray
    partial: np.ndarray
    kernel_ms: float = 0.0


@dataclass
class ConsResult:
    """cl_cons_result (include/callable_loci.h): the five classes add up to end - start; cons[p - start] = the byte of
    position p, one of n - A C G T N."""
    start: int
    end: int
    low_depth: int
    deleted: int
    no_call: int
    ref: int
    alt: int
    cons: np.ndarray
    kernel_ms: float = 0.0


@dataclass
class InsResult:
    """cl_ins_result (include/callable_loci.h): the three classes add up to end - start; candidates = the positions of
    class inserted, ascending; observations = every counting insertion at a candidate."""
    start: int
    end: int
    low_depth: int
    kept: int
    inserted: int
    candidates: np.ndarray
    observations: np.ndarray
    kernel_ms: float = 0.0


@dataclass
class DelResult:
    """cl_del_result (include/callable_loci.h): the three classes add up to end - start; candidates = the positions of
    class deleted, ascending."""
    start: int
    end: int
    low_depth: int
    kept: int
    deleted: int
    candidates: np.ndarray
    kernel_ms: float = 0.0


@dataclass
class MinorResult:
    """cl_minor_result (include/callable_loci.h): the three classes add up to end - start; candidates = the positions of
    class minor, ascending."""
    start: int
    end: int
    low_depth: int
    single: int
    minor: int
    candidates: np.ndarray
    kernel_ms: float = 0.0


@dataclass
class ScanResult:
    """cl_scan_result (include/callable_loci.h): the five classes add up to end - start; candidates = the positions of
    class variant, ascending."""
    start: int
    end: int
    low_depth: int
    mixed: int
    uncomparable: int
    match: int
    variant: int
    candidates: np.ndarray


@dataclass
class DepthProfile:
    """cl_depth_profile (include/callable_loci.h): hist_*[b] = positions with min(depth, n_bins - 1) == b, the exact
    sums, and per window of `window` positions the sum of the depths (None without a window)."""
    n_bins: int
    window: int
    n_windows: int
    extent: int
    sum_raw: int
    sum_qc: int
    hist_raw: np.ndarray
    hist_qc: np.ndarray
    win_raw: Optional[np.ndarray]
    win_qc: Optional[np.ndarray]
    kernel_ms: float = 0.0          # cl_contig_depth_profile_ms: the kernel by device events while profiling is on

    def _c(self):
        p = _lib.cl_depth_profile()
        p.n_bins, p.window, p.n_windows, p.extent = self.n_bins, self.window, self.n_windows, self.extent
        p.sum_raw, p.sum_qc = self.sum_raw, self.sum_qc
        keep = [np.ascontiguousarray(a, np.uint64) if a is not None else None
                for a in (self.hist_raw, self.hist_qc, self.win_raw, self.win_qc)]
        u64p = C.POINTER(C.c_uint64)
        p.hist_raw, p.hist_qc, p.win_raw, p.win_qc = [k.ctypes.data_as(u64p) if k is not None and k.size else u64p() for k in keep]
        # (an empty histogram still needs a pointer: n_bins >= 2 always; only the window tables may be empty)
        return p, keep


@dataclass
class GcBias:
    """cl_gc_bias (include/callable_loci.h): per GC percentage b of the window around a position, positions[b] counted
    positions, the sums of their raw and qc depth and zero_raw[b] of them without a read; n_skipped positions had more
    than max_invalid invalid bases in their window.  Records add up (`+`, dut_gc_bias_add)."""
    window: int
    max_invalid: int
    extent: int
    n_skipped: int
    positions: np.ndarray
    sum_raw: np.ndarray
    sum_qc: np.ndarray
    zero_raw: np.ndarray
    kernel_ms: float = 0.0          # cl_contig_gc_bias_ms: the kernel by device events while profiling is on
    upload_ms: float = 0.0          # ... pack + upload of the reference's bit planes, by the host's clock

    @classmethod
    def _from_c(cls, g, kernel_ms=0.0, upload_ms=0.0):
        def arr(a):
            return np.ctypeslib.as_array(a).astype(np.uint64)
        return cls(window=int(g.window), max_invalid=int(g.max_invalid), extent=int(g.extent), n_skipped=int(g.n_skipped),
                   positions=arr(g.positions), sum_raw=arr(g.sum_raw), sum_qc=arr(g.sum_qc), zero_raw=arr(g.zero_raw),
                   kernel_ms=kernel_ms, upload_ms=upload_ms)

    @classmethod
    def empty(cls):
        """a zeroed record: the start of a sum (it takes the window and max_invalid of the first record added)"""
        return cls._from_c(_lib.cl_gc_bias())

    def _c(self):
        g = _lib.cl_gc_bias()
        g.window, g.max_invalid, g.extent, g.n_skipped = self.window, self.max_invalid, self.extent, self.n_skipped
        for f in ("positions", "sum_raw", "sum_qc", "zero_raw"):
            a = np.ascontiguousarray(getattr(self, f), np.uint64).reshape(-1)
            if a.size != _lib.CL_GC_BINS:
                raise EngineError(-1, f"GcBias.{f}: {_lib.CL_GC_BINS} bins")
            getattr(g, f)[:] = [int(x) for x in a]
        return g

    def add(self, other):
        """dut_gc_bias_add: the sum of both records (EngineError where window or max_invalid differ)"""
        t, p = self._c(), other._c()
        st = _lib.load().dut_gc_bias_add(C.byref(t), C.byref(p))
        if st != 0:
            raise EngineError(st, "dut_gc_bias_add: the records differ in window or max_invalid")
        return GcBias._from_c(t)

    __add__ = add

    def tobytes(self):
        return bytes(self._c())


def gc_bias_stats(g: GcBias):
    """dut_gc_bias_stats: the totals, the per-bin means, normalised means and zero fractions (numpy f64, NaN where not
    available) and the four dropouts (None where not available) of a GcBias, as a dict."""
    c = g._c()
    out = _lib.dut_gc_stats()
    st = _lib.load().dut_gc_bias_stats(C.byref(c), C.byref(out))
    if st != 0:
        raise EngineError(st, "dut_gc_bias_stats failed")

    def arr(a):
        v = np.ctypeslib.as_array(a).astype(np.float64)
        v[v < 0] = np.nan
        return v

    def num(x):
        return None if x < 0 else float(x)
    return {"positions": int(out.positions), "sum_raw": int(out.sum_raw), "sum_qc": int(out.sum_qc),
            "total_mean_raw": num(out.total_mean_raw), "total_mean_qc": num(out.total_mean_qc),
            "at_dropout_raw": num(out.at_dropout_raw), "gc_dropout_raw": num(out.gc_dropout_raw),
            "at_dropout_qc": num(out.at_dropout_qc), "gc_dropout_qc": num(out.gc_dropout_qc),
            "mean_raw": arr(out.mean_raw), "mean_qc": arr(out.mean_qc), "norm_raw": arr(out.norm_raw), "norm_qc": arr(out.norm_qc),
            "zero_frac": arr(out.zero_frac)}


def _write_gc(path, contigs, header, line, total):
    lib = _lib.load()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    contigs = list(contigs)
    f = libc.fopen(path.encode(), b"wb")
    if not f:
        raise OSError("cannot open " + path)
    st = getattr(lib, header)(f)
    acc = None
    for name, g in contigs:
        c = g._c()
        if st == 0:
            st = getattr(lib, line)(f, name.encode(), C.byref(c))
        acc = g if acc is None else acc.add(g)
    if st == 0 and total and acc is not None:
        c = acc._c()
        st = getattr(lib, line)(f, b"total", C.byref(c))
    if libc.fclose(f) != 0 and st == 0:
        st = -1
    if st != 0:
        raise EngineError(st, "cannot write " + path)


def write_gc_bias(path, contigs, total=True):
    """dut_gc_bias_write_header / dut_gc_bias_write: the bias table of include/dut_coverage.h.  contigs: (name, GcBias) in
    output order; total: the sum of the records follows as `total`."""
    _write_gc(path, contigs, "dut_gc_bias_write_header", "dut_gc_bias_write", total)


def write_gc_summary(path, contigs, total=True):
    """dut_gc_summary_write_header / dut_gc_summary_write: one summary line per (name, GcBias), then `total`."""
    _write_gc(path, contigs, "dut_gc_summary_write_header", "dut_gc_summary_write", total)


@dataclass
class DepthRuns:
    """cl_depth_runs (include/callable_loci.h): run i = [start[i], start[i + 1]) -- the last one ends at extent -- of
    value[i]; the value is the depth, or with edges the number of edges <= depth."""
    kind: int
    edges: np.ndarray
    extent: int
    n_runs: int
    start: np.ndarray
    value: np.ndarray
    kernel_ms: float = 0.0          # cl_contig_depth_runs_ms: both launches and the scan, while profiling is on

    def ends(self):
        return np.append(self.start[1:], np.uint32(self.extent)).astype(np.uint64) if self.n_runs else np.zeros(0, np.uint64)


# cl_target_stats as a numpy record
TARGET_STATS = np.dtype([("start", np.uint32), ("end", np.uint32), ("len", np.uint32), ("reserved", np.uint32),
                         ("sum_raw", np.uint64), ("sum_qc", np.uint64), ("state", np.uint32, (6,)),
                         ("ge_raw", np.uint32, (_lib.CL_TARGET_MAX_THRESHOLDS,)), ("ge_qc", np.uint32, (_lib.CL_TARGET_MAX_THRESHOLDS,))])
assert TARGET_STATS.itemsize == C.sizeof(_lib.cl_target_stats)


@dataclass
class TargetStats:
    """cl_target_stats per target (include/callable_loci.h), one array entry per target in the order given: start, end and
    len clipped to the extent, the exact sums of raw and qc depth, state[i, s] = positions of CalledState s, and
    ge_raw[i, k] / ge_qc[i, k] = positions with raw / qc depth >= thresholds[k]."""
    thresholds: np.ndarray
    start: np.ndarray
    end: np.ndarray
    len: np.ndarray
    sum_raw: np.ndarray
    sum_qc: np.ndarray
    state: np.ndarray
    ge_raw: np.ndarray
    ge_qc: np.ndarray
    kernel_ms: float = 0.0          # cl_contig_targets_ms: the three launches, while profiling is on
    launch_ms: tuple = (0.0, 0.0, 0.0)   # ... k_target_depth, k_target_scan, k_target_finish apart

    @classmethod
    def from_records(cls, rec, thresholds, kernel_ms=0.0, launch_ms=(0.0, 0.0, 0.0)):
        k = int(np.asarray(thresholds).size)
        return cls(thresholds=np.asarray(thresholds, np.uint32), start=rec["start"].copy(), end=rec["end"].copy(), len=rec["len"].copy(),
                   sum_raw=rec["sum_raw"].copy(), sum_qc=rec["sum_qc"].copy(), state=rec["state"].copy(),
                   ge_raw=rec["ge_raw"][:, :k].copy(), ge_qc=rec["ge_qc"][:, :k].copy(), kernel_ms=kernel_ms, launch_ms=launch_ms)

    def records(self):
        """the cl_target_stats records (a TARGET_STATS array)"""
        n, k = int(self.start.size), int(self.thresholds.size)
        rec = np.zeros(n, TARGET_STATS)
        for f in ("start", "end", "len", "sum_raw", "sum_qc", "state"):
            rec[f] = getattr(self, f)
        rec["ge_raw"][:, :k] = self.ge_raw
        rec["ge_qc"][:, :k] = self.ge_qc
        return rec


# cl_target_order as a numpy record
TARGET_ORDER = np.dtype([("start", np.uint32), ("end", np.uint32), ("len", np.uint32), ("raw", np.uint32, (5,)), ("qc", np.uint32, (5,))])
assert TARGET_ORDER.itemsize == C.sizeof(_lib.cl_target_order)


@dataclass
class TargetOrder:
    """cl_target_order per target (include/callable_loci.h), one array entry per target in the order given: start, end and
    len clipped to the extent, raw[i] and qc[i] = (min, q1, median, q3, max) of the raw and the quality-filtered depth over
    the target, all zeros for a target of length 0."""
    start: np.ndarray
    end: np.ndarray
    len: np.ndarray
    raw: np.ndarray
    qc: np.ndarray
    kernel_ms: float = 0.0          # cl_contig_target_order_ms: all launches, while profiling is on
    n_rounds: int = 0               # ... the bit rounds: the bit length of the largest raw depth of any target

    @classmethod
    def from_records(cls, rec, kernel_ms=0.0, n_rounds=0):
        return cls(start=rec["start"].copy(), end=rec["end"].copy(), len=rec["len"].copy(), raw=rec["raw"].copy().reshape(-1, 5),
                   qc=rec["qc"].copy().reshape(-1, 5), kernel_ms=kernel_ms, n_rounds=n_rounds)

    def records(self):
        """the cl_target_order records (a TARGET_ORDER array)"""
        rec = np.zeros(int(self.start.size), TARGET_ORDER)
        for f in ("start", "end", "len", "raw", "qc"):
            rec[f] = getattr(self, f)
        return rec


def parse_targets(text):
    """dut_targets_parse: BED text (str or bytes) -> a list of (contig, starts, ends, names) in the order the contigs
    first appear, the targets of a contig in file order (starts and ends: numpy uint32; names: column 4, else ".").
    Raises EngineError with the line number for a malformed line."""
    lib = _lib.load()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    err = C.create_string_buffer(512)
    h = lib.dut_targets_parse(raw, len(raw), err, 512)
    if not h:
        raise EngineError(-1, err.value.decode())
    try:
        out = []
        for c in range(lib.dut_targets_n_contigs(h)):
            n = C.c_size_t()
            name = lib.dut_targets_contig(h, c, C.byref(n)).decode()
            s, e, ln = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
            nm = C.POINTER(C.c_char_p)()
            lib.dut_targets_get(h, c, C.byref(s), C.byref(e), C.byref(nm), C.byref(ln))
            k = int(n.value)
            out.append((name, np.ctypeslib.as_array(s, shape=(k,)).copy(), np.ctypeslib.as_array(e, shape=(k,)).copy(),
                        [nm[i].decode() for i in range(k)]))
        return out
    finally:
        lib.dut_targets_free(h)


def thresholds_parse(spec):
    """dut_thresholds_parse: the depth thresholds of a `--target-thresholds` argument ("1,10,20,30") as a list."""
    t = (C.c_uint32 * _lib.CL_TARGET_MAX_THRESHOLDS)()
    n = C.c_uint32()
    err = C.create_string_buffer(256)
    st = _lib.load().dut_thresholds_parse(spec.encode() if spec is not None else None, t, C.byref(n), err, 256)
    if st != 0:
        raise EngineError(st, err.value.decode())
    return [int(t[i]) for i in range(n.value)]


def write_target_stats(path, contigs, thresholds, order=None):
    """dut_targets_write_header_ex / dut_targets_write_ex / dut_targets_write_total_ex: the per-target table of
    include/dut_coverage.h.  contigs: (contig, TargetStats, names) in output order; the file ends with the `total` line over
    all of them.  order: None, or one TargetOrder per entry of contigs (of the same targets): the table gets the ten
    columns raw_min ... qc_max behind the others."""
    lib = _lib.load()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    t = np.ascontiguousarray(thresholds, np.uint32).reshape(-1)
    u32p = C.POINTER(C.c_uint32)
    f = libc.fopen(path.encode(), b"wb")
    if not f:
        raise OSError("cannot open " + path)
    total = (C.c_uint64 * 32)()                    # dut_target_total
    contigs = list(contigs)
    if order is not None and len(order) != len(contigs):
        libc.fclose(f)
        raise EngineError(-1, "write_target_stats: one TargetOrder per contig")
    cols = 0 if order is None else 1
    st = lib.dut_targets_write_header_ex(f, t.ctypes.data_as(u32p) if t.size else None, int(t.size), cols)
    for i, (contig, stats, names) in enumerate(contigs):
        rec = np.ascontiguousarray(stats.records())
        n = int(rec.size)
        nm = (C.c_char_p * max(n, 1))(*[(x or ".").encode() for x in names])
        orec = np.ascontiguousarray(order[i].records()) if order is not None else None
        if orec is not None and int(orec.size) != n:
            st = st or -1
        if st == 0:
            st = lib.dut_targets_write_ex(f, contig.encode(), rec.ctypes.data_as(C.POINTER(_lib.cl_target_stats)),
                                          orec.ctypes.data_as(C.POINTER(_lib.cl_target_order)) if orec is not None else None,
                                          nm, n, int(t.size), C.cast(total, C.c_void_p))
    if st == 0:
        st = lib.dut_targets_write_total_ex(f, C.cast(total, C.c_void_p), int(t.size), cols)
    if libc.fclose(f) != 0 and st == 0:
        st = -1
    if st != 0:
        raise EngineError(st, "write_target_stats: cannot write " + path)


def quantize_parse(spec):
    """dut_quantize_parse: the band edges of a `--quantize` argument ("1:4:100", "0:1:4:100:") as a list; None or empty
    text: [] (exact depth).  Raises EngineError with the reason for a malformed one."""
    edges = (C.c_uint32 * _lib.CL_RUNS_MAX_EDGES)()
    n = C.c_uint32()
    err = C.create_string_buffer(256)
    st = _lib.load().dut_quantize_parse(spec.encode() if spec is not None else None, edges, C.byref(n), err, 256)
    if st != 0:
        raise EngineError(st, err.value.decode())
    return [int(edges[i]) for i in range(n.value)]


def write_depth_bed(path, contig, runs: DepthRuns, append=False):
    """dut_depth_bed_write: the runs of one contig as lines of a depth BED (contig, start, end, depth or LO:HI band)."""
    lib = _lib.load()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    u32p = C.POINTER(C.c_uint32)
    keep = [np.ascontiguousarray(a, np.uint32) for a in (runs.start, runs.value, runs.edges)]
    r = _lib.cl_depth_runs(int(runs.kind), int(keep[2].size), int(runs.extent), int(runs.n_runs),
                           keep[0].ctypes.data_as(u32p), keep[1].ctypes.data_as(u32p))
    f = libc.fopen(path.encode(), b"ab" if append else b"wb")
    if not f:
        raise OSError("cannot open " + path)
    st = lib.dut_depth_bed_write(f, contig.encode(), C.byref(r), keep[2].ctypes.data_as(u32p) if keep[2].size else None)
    if libc.fclose(f) != 0 and st == 0:
        st = -1
    if st != 0:
        raise EngineError(st, "dut_depth_bed_write: cannot write " + path)


def depth_stats(hist, total):
    """dut_depth_stats: positions, mean, quartiles (value, saturated) and the share of positions at or above
    1, 5, 10, 15, 20, 30, 50, 100 (None where the histogram's last exact bin lies below the threshold)."""
    h = np.ascontiguousarray(hist, np.uint64)
    out = _lib.dut_depth_summary()
    st = _lib.load().dut_depth_stats(h.ctypes.data_as(C.POINTER(C.c_uint64)), h.shape[0], int(total), C.byref(out))
    if st != 0:
        raise EngineError(st, "dut_depth_stats: a histogram needs at least two bins")
    return {"positions": int(out.positions), "mean": float(out.mean),
            "q1": (int(out.q1), bool(out.q1_saturated)), "median": (int(out.median), bool(out.median_saturated)),
            "q3": (int(out.q3), bool(out.q3_saturated)),
            "frac_at_least": {t: (None if out.frac_at_least[k] < 0 else float(out.frac_at_least[k]))
                              for k, t in enumerate(_lib.DEPTH_THRESHOLDS)}}


class DepthAccumulator:
    """dut_depth_acc: adds contigs' depth profiles (in output order) into a total and writes the distribution,
    window and summary files (formats: include/dut_coverage.h)."""

    def __init__(self, n_bins, window=0, windows_path=None):
        self._lib = _lib.load()
        self.n_bins = n_bins
        self._h = self._lib.dut_depth_acc_new(n_bins, window, windows_path.encode() if windows_path else None)
        if not self._h:
            raise EngineError(-1, "dut_depth_acc_new: bad bin count or window, or the window file cannot be created")

    def add(self, contig, profile: DepthProfile):
        p, keep = profile._c()
        st = self._lib.dut_depth_acc_add(self._h, contig.encode(), C.byref(p))
        del keep
        if st != 0:
            raise EngineError(st, "dut_depth_acc_add: the profile does not fit the accumulator")

    def total(self):
        hr, hq = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        sr, sq = C.c_uint64(), C.c_uint64()
        self._lib.dut_depth_acc_total(self._h, C.byref(hr), C.byref(hq), C.byref(sr), C.byref(sq))
        return (np.ctypeslib.as_array(hr, shape=(self.n_bins,)).copy(), np.ctypeslib.as_array(hq, shape=(self.n_bins,)).copy(),
                int(sr.value), int(sq.value))

    def finish(self, dist_path=None, summary_path=None):
        st = self._lib.dut_depth_acc_finish(self._h, dist_path.encode() if dist_path else None,
                                            summary_path.encode() if summary_path else None)
        if st != 0:
            raise EngineError(st, "dut_depth_acc_finish: cannot write the depth profile files")

    def close(self):
        if self._h:
            self._lib.dut_depth_acc_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostStage(Engine):
    """A context WITHOUT a device (cl_debug_host_create), for the CPU test suite: contig_begin / push_reads stage a
    contig exactly as a device context does, `pass_rows_segments` runs the upload's row builder over it and `pass_rows`
    the one-stack-per-window builder it is held against.  Everything that needs a
    device raises: there is no CPU pileup."""

    def __init__(self, options: CallableOptions):
        self._lib = _lib.load()
        self.options = options
        self._opt_c = options.to_c()
        h = C.c_void_p()
        st = self._lib.cl_debug_host_create(C.byref(self._opt_c), C.byref(h))
        if st != 0:
            raise EngineError(st, "cl_debug_host_create failed")
        self._h = h
        self.device_id = -1
        self._keep = []

    def pass_rows(self):
        """(n_groups per window, rows as uint32 array of 256-word groups window after window, summed_baseq)."""
        nwords = C.c_uint64(); nwin = C.c_uint32(); sq = C.c_uint64()
        self._check(self._lib.cl_debug_pass_rows(self._h, None, 0, None, 0, C.byref(nwords), C.byref(nwin), C.byref(sq)))
        ng = np.zeros(max(nwin.value, 1), np.uint32)
        rows = np.zeros(max(nwords.value, 1), np.uint32)
        self._check(self._lib.cl_debug_pass_rows(self._h, _ptr(ng), nwin.value, _ptr(rows), nwords.value, C.byref(nwords),
                                                 C.byref(nwin), C.byref(sq)))
        return ng[:nwin.value], rows[:nwords.value], int(sq.value)

    def pass_rows_segments(self):
        """The rows as the device holds them, a stack per segment of 256 positions: (heights (n_windows, 8) in units, the
        height word of every window's record -- 0: the equal-heights form --, units as uint32 array of 32-word units, window
        after window and segment after segment)."""
        nwords = C.c_uint64(); nwin = C.c_uint32()
        self._check(self._lib.cl_debug_pass_rows_segments(self._h, None, None, 0, None, 0, C.byref(nwords), C.byref(nwin)))
        h = np.zeros((max(nwin.value, 1), 8), np.uint32)
        words = np.zeros(max(nwin.value, 1), np.uint64)
        units = np.zeros(max(nwords.value, 1), np.uint32)
        self._check(self._lib.cl_debug_pass_rows_segments(self._h, _ptr(h), _ptr(words), nwin.value, _ptr(units), nwords.value,
                                                          C.byref(nwords), C.byref(nwin)))
        return h[:nwin.value], words[:nwin.value], units[:nwords.value]


@dataclass
class ContigResult:
    summary: "_lib.cl_contig_summary"
    intervals: np.ndarray       # (n,3) uint32: start, end (exclusive), state

    @property
    def state_counts(self):
        return [int(x) for x in self.summary.state_counts]

    def as_dict(self):
        s = self.summary
        return dict(state_counts=self.state_counts, n_covered_bases=int(s.n_covered_bases),
                    summed_coverage=int(s.summed_coverage), summed_baseq=int(s.summed_baseq),
                    summed_mapq=int(s.summed_mapq), quality_bases=int(s.quality_bases),
                    extent=int(s.extent), max_raw_depth=int(s.max_raw_depth),
                    n_intervals=int(s.n_intervals))


class CallableProfiler:
    """CallableProfiler (callable_profiler.rs): owns the BED file."""

    def __init__(self, bed_file: str, largest_contig_length: int = 0):
        self._lib = _lib.load()
        self._h = self._lib.dut_profiler_new(bed_file.encode())
        if not self._h:
            raise OSError(f"cannot create {bed_file}")
        self.largest_contig_length = largest_contig_length

    def enable_plots(self, largest_contig_length: Optional[int] = None):
        """From here on every BED line of a plotted state is a range of the current contig's coverage figure
        (callable_profiler.rs:48-59); `finish_plot` writes `<dir of the BED>/<contig>_coverage.svg`."""
        if largest_contig_length is not None:
            self.largest_contig_length = largest_contig_length
        self._lib.dut_profiler_enable_plots(self._h, self.largest_contig_length)

    def plot_bins(self, contig: str, contig_length: int):
        """(stride, callable, low_qual, ref_n): positions of the three plotted states per stride of the
        pending ranges (histogram_plotter.rs:74-101)."""
        n = C.c_size_t(); stride = C.c_uint32()
        st = self._lib.dut_profiler_plot_bins(self._h, contig.encode(), contig_length, C.byref(stride), None, None, None, 0, C.byref(n))
        if st != 0:
            raise EngineError(st, "dut_profiler_plot_bins failed")
        a = [np.zeros(n.value, np.uint32) for _ in range(3)]
        self._lib.dut_profiler_plot_bins(self._h, contig.encode(), contig_length, C.byref(stride), _ptr(a[0]), _ptr(a[1]), _ptr(a[2]),
                                         n.value, C.byref(n))
        return int(stride.value), a[0], a[1], a[2]

    def finish_plot(self, contig: str, contig_length: int) -> bool:
        st = self._lib.dut_profiler_finish_plot(self._h, contig.encode(), contig_length)
        if st < 0:
            raise EngineError(st, "dut_profiler_finish_plot failed")
        return st == 1

    def get_contig_counts(self, contig: str):
        out = (C.c_uint64 * 6)()
        self._lib.dut_profiler_contig_counts(self._h, contig.encode(), out)
        return [int(x) for x in out]

    def feed_contig(self, contig: str, result: ContigResult):
        iv = np.ascontiguousarray(result.intervals, np.uint32)
        cnt = (C.c_uint64 * 6)(*result.state_counts)
        st = self._lib.dut_profiler_feed_contig(self._h, contig.encode(), _ptr(iv), iv.shape[0], cnt)
        if st != 0:
            raise EngineError(st, "dut_profiler_feed_contig failed")

    def close(self):
        """Drop: flush the writer."""
        if self._h:
            self._lib.dut_profiler_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class ContigProfiler:
    """ContigProfiler (contig_profiler.rs): per-contig accumulators + derived statistics."""
    name: str
    length: int
    n_covered_bases: int = 0
    summed_coverage: int = 0
    summed_baseq: int = 0
    summed_mapq: int = 0
    quality_bases: int = 0
    n_reads: int = 0

    def _c(self):
        return _lib.dut_contig_stats(self.length, self.n_covered_bases, self.summed_coverage,
                                     self.summed_baseq, self.summed_mapq, self.quality_bases,
                                     self.n_reads, 0)

    def _load(self, c):
        self.n_covered_bases = int(c.n_covered_bases); self.summed_coverage = int(c.summed_coverage)
        self.summed_baseq = int(c.summed_baseq); self.summed_mapq = int(c.summed_mapq)
        self.quality_bases = int(c.quality_bases); self.n_reads = int(c.n_reads)

    def derived(self):
        d = _lib.dut_contig_derived()
        c = self._c()
        _lib.load().dut_contig_derive(C.byref(c), C.byref(d))
        return dict(coverage_percent=d.coverage_percent, average_depth=d.average_depth,
                    average_mapq=d.average_mapq, average_baseq=d.average_baseq,
                    q30_percentage=d.q30_percentage)

    def get_coverage_stats(self):
        d = self.derived()
        return dict(unique_reads=self.n_reads, coverage_percent=d["coverage_percent"],
                    average_depth=d["average_depth"], covered_bases=self.n_covered_bases,
                    total_bases=self.length)

    def get_quality_stats(self):
        d = self.derived()
        return dict(average_mapq=d["average_mapq"], average_baseq=d["average_baseq"],
                    q30_percentage=d["q30_percentage"])


def admit_reads(options: CallableOptions, tid: int, contig_len: int, rec: ContigRecords):
    """FUNMAP drop + maxcnt rule + region filter; returns (accepted mask, n distinct names)."""
    lib = _lib.load()
    acc = np.zeros(max(rec.n, 1), np.uint8)
    nn = C.c_uint32(); na = C.c_uint64()
    oc = options.to_c(); rc = _records_c(rec)
    st = lib.dut_admit_reads(C.byref(oc), tid, contig_len, C.byref(rc), _ptr(acc), C.byref(nn), C.byref(na))
    if st != 0:
        raise EngineError(st, "reads are not coordinate sorted" if st == -3 else "dut_admit_reads failed")
    return acc[:rec.n].astype(bool), nn.value


def process_single_contig(engine: Engine, counter: CallableProfiler, stats: ContigProfiler,
                          options: CallableOptions, tid: int, rec: ContigRecords,
                          ref: Optional[np.ndarray]):
    """process_single_contig (mod.rs:44-147): `bam`/`fasta`/`header` of the reference become the
    decoded records of the contig, its FASTA bytes and (stats.name, stats.length)."""
    lib = _lib.load()
    ref = np.ascontiguousarray(ref, np.uint8) if ref is not None else np.zeros(0, np.uint8)
    oc = options.to_c(); rc = _records_c(rec); cs = stats._c()
    st = lib.dut_process_single_contig(engine._h, counter._h, C.byref(cs), C.byref(oc), stats.name.encode(),
                                       tid, stats.length, _ptr(ref), ref.shape[0], C.byref(rc))
    if st != 0:
        msg = lib.cl_last_error(engine._h).decode() or "admission failed"
        if st == -3:
            msg = msg or "reads are not coordinate sorted"
        raise EngineError(st, msg)
    stats._load(cs)


def compare_contig_names(a: str, b: str) -> int:
    return _lib.load().dut_compare_contig_names(a.encode(), b.encode())


def genome_summary(stats: List[ContigProfiler], callable_counts: List[int]):
    """report.rs:26-126 over contigs sorted with compare_contig_names (report.rs:37-38)."""
    import functools
    order = sorted(range(len(stats)), key=functools.cmp_to_key(
        lambda i, j: compare_contig_names(stats[i].name, stats[j].name)))
    n = len(order)
    arr = (_lib.dut_contig_stats * max(n, 1))()
    call = (C.c_uint64 * max(n, 1))()
    for k, i in enumerate(order):
        arr[k] = stats[i]._c()
        call[k] = callable_counts[i]
    out = _lib.dut_genome_summary()
    _lib.load().dut_genome_summary_build(arr, call, n, C.byref(out))
    return dict(total_bases=int(out.total_bases), callable_bases=int(out.callable_bases),
                callable_percentage=out.callable_percentage, average_depth=out.average_depth,
                average_mapq=out.average_mapq, average_baseq=out.average_baseq,
                q30_percentage=out.q30_percentage, total_unique_reads=int(out.total_unique_reads),
                contigs_analyzed=int(out.contigs_analyzed),
                order=[stats[i].name for i in order])
