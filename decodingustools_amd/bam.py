"""BAM / FASTA input (include/dut_bam.h) and the file-level `coverage` entry point: what the reference
does with rust-htslib before and around the hot path (utils/bam_reader.rs:7-14, mod.rs:53-55,
api/coverage.rs:53-115)."""
import ctypes as C

import numpy as np

from . import _lib
from .callable_loci import CallableOptions, EngineError
from .records import ContigRecords


def _arr(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n).copy()


class BamReader:
    """IndexedReader stand-in: header + per-contig fetch of decoded records."""

    def __init__(self, path: str):
        self._lib = _lib.load()
        err = C.create_string_buffer(512)
        self._h = self._lib.dut_bam_open(path.encode(), err, 512)
        if not self._h:
            raise OSError(err.value.decode())
        n = self._lib.dut_bam_n_ref(self._h)
        self.target_names = [self._lib.dut_bam_ref_name(self._h, t).decode() for t in range(n)]
        self.target_lens = [int(self._lib.dut_bam_ref_len(self._h, t)) for t in range(n)]
        ln = C.c_size_t()
        p = self._lib.dut_bam_header_text(self._h, C.byref(ln))
        self.header_text = C.string_at(p, ln.value).decode(errors="replace") if ln.value else ""
        self.has_index = bool(self._lib.dut_bam_has_index(self._h))
        # mapped reads per reference from the .bai metadata (-1 = not recorded): the balancing weight
        self.target_mapped = [int(self._lib.dut_bam_ref_mapped(self._h, t)) for t in range(n)]

    def fetch_contig(self, tid: int, with_seq: bool = False) -> ContigRecords:
        r = _lib.dut_records()
        so, sq = C.c_void_p(), C.c_void_p()
        st = self._lib.dut_bam_read_contig(self._h, tid, C.byref(r), C.byref(so) if with_seq else None,
                                           C.byref(sq) if with_seq else None)
        if st != 0:
            raise EngineError(st, self._lib.dut_bam_error(self._h).decode())
        n = int(r.n)
        coff = _arr(r.cigar_off, n + 1, np.uint32); qoff = _arr(r.qual_off, n + 1, np.uint64)
        noff = _arr(r.qname_off, n + 1, np.uint32)
        rec = ContigRecords(
            pos=_arr(r.pos, n, np.int32), flag=_arr(r.flag, n, np.uint16), mapq=_arr(r.mapq, n, np.uint8),
            cigar_off=coff, cigar=_arr(r.cigar, int(coff[-1]), np.uint32), qual_off=qoff,
            qual=_arr(r.qual, int(qoff[-1]), np.uint8), qname_off=noff, qname=_arr(r.qname, int(noff[-1]), np.uint8))
        if with_seq:
            rec.seq_off = _arr(so.value, n + 1, np.uint64)
            rec.seq4 = _arr(sq.value, (int(rec.seq_off[-1]) + 1) // 2, np.uint8)
        return rec.validate()

    def fetch_contig_bits(self, tid: int, min_base_quality: int):
        """dut_bam_read_contig_bits: the records with the base-quality test taken at parse -> (ContigRecords without
        quality bytes, pass_bits uint64, pass_sum uint32)."""
        r = _lib.dut_records()
        st = self._lib.dut_bam_read_contig_bits(self._h, tid, min_base_quality, C.byref(r))
        if st != 0:
            raise EngineError(st, self._lib.dut_bam_error(self._h).decode())
        n = int(r.n)
        coff = _arr(r.cigar_off, n + 1, np.uint32); qoff = _arr(r.qual_off, n + 1, np.uint64)
        noff = _arr(r.qname_off, n + 1, np.uint32)
        rec = ContigRecords(
            pos=_arr(r.pos, n, np.int32), flag=_arr(r.flag, n, np.uint16), mapq=_arr(r.mapq, n, np.uint8),
            cigar_off=coff, cigar=_arr(r.cigar, int(coff[-1]), np.uint32), qual_off=qoff,
            qual=np.zeros(0, np.uint8), qname_off=noff, qname=_arr(r.qname, int(noff[-1]), np.uint8))
        bits = _arr(r.pass_bits, (int(qoff[-1]) + 63) // 64 + 1, np.uint64)
        return rec, bits, _arr(r.pass_sum, n, np.uint32)

    def close(self):
        if self._h:
            self._lib.dut_bam_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class FastaReader:
    def __init__(self, path: str):
        self._lib = _lib.load()
        err = C.create_string_buffer(512)
        self._h = self._lib.dut_fasta_open(path.encode(), err, 512)
        if not self._h:
            raise OSError(err.value.decode())

    def fetch(self, name: str) -> np.ndarray:
        p, n = C.c_void_p(), C.c_uint64()
        st = self._lib.dut_fasta_fetch(self._h, name.encode(), C.byref(p), C.byref(n))
        if st != 0:                                    # fetch_seq(..)? of the reference (mod.rs:79)
            raise OSError(self._lib.dut_fasta_error(self._h).decode())
        return _arr(p.value, int(n.value), np.uint8)

    def close(self):
        if self._h:
            self._lib.dut_fasta_close(self._h)
            self._h = None


def coverage_files(bam_file: str, reference_file: str, output_bed: str = "callable_regions.bed",
                   summary_json: str = None, options: CallableOptions = None, contigs=None, device_id: int = 0,
                   output_summary: str = None, devices=None, depth_dist: str = None, depth_windows: str = None,
                   depth_summary: str = None, depth_cap: int = 1000, window: int = 0, depth_bed: str = None,
                   depth_bed_kind: str = "raw", quantize: str = None, targets: str = None, target_out: str = None,
                   target_thresholds=None, target_quantiles: bool = False, gc_bias: str = None, gc_summary: str = None,
                   gc_window: int = None, gc_max_invalid: int = None):
    """CoverageAnalyzer::analyze on files (CoverageInput of api/coverage.rs:124-132); summary_json
    receives the CoverageOutput JSON of main.rs:68-69; output_summary, when given, the HTML report
    (api/coverage.rs:104; None: not written, the JSON then names "summary.html").  The per-contig coverage
    figures `<contig>_coverage.svg` go beside the BED file (callable_profiler.rs:80-84).
    devices: a list of HIP ordinals (one may repeat) -- the contigs are dealt to them inside the library
    (dut_coverage_files_multi: one host thread and one engine context per entry, no torch, no collective).
    depth_dist / depth_windows (with window >= 16) / depth_summary: the depth profile files of dut_coverage_files_ex
    (formats: include/dut_coverage.h); depth_cap: depths above it share the last histogram bin.
    depth_bed: the per-base depth of every contig as a BED of runs of equal depth (dut_coverage_files_ex2);
    depth_bed_kind "raw" or "qc"; quantize: band edges such as "1:4:100" (None or "": exact depth).
    targets: a BED of regions, target_out: the per-target table of dut_coverage_files_ex3 (include/dut_coverage.h has the
    format); target_thresholds: up to 8 ascending depths (default 1, 10, 20, 30); target_quantiles: the table also gets
    minimum, quartiles and maximum of both depths per target (dut_coverage_files_ex4, DUT_TARGETS_ORDER).
    gc_bias / gc_summary: the GC-bias table and summary of dut_coverage_files_ex5 (include/dut_coverage.h has the
    formats), with a window of gc_window positions (default 100) around each position and at most gc_max_invalid
    (default 4) invalid bases in it."""
    lib = _lib.load()
    options = options or CallableOptions()
    oc = options.to_c()
    arr = None
    n = 0
    if contigs is not None:
        n = len(contigs)
        arr = (C.c_char_p * max(n, 1))(*[c.encode() for c in contigs])
    err = C.create_string_buffer(1024)
    if depth_bed is None and (quantize is not None or depth_bed_kind != "raw"):
        raise EngineError(-1, "quantize and depth_bed_kind need depth_bed")
    if targets is None and (target_out is not None or target_thresholds is not None):
        raise EngineError(-1, "target_out and target_thresholds need targets")
    if targets is None and target_quantiles:
        raise EngineError(-1, "target_quantiles needs targets")
    if targets is not None and target_out is None:
        raise EngineError(-1, "targets needs target_out")
    if gc_bias is None and gc_summary is None and (gc_window is not None or gc_max_invalid is not None):
        raise EngineError(-1, "gc_window and gc_max_invalid need gc_bias or gc_summary")
    if gc_bias is not None or gc_summary is not None:
        gw, gk = int(100 if gc_window is None else gc_window), int(4 if gc_max_invalid is None else gc_max_invalid)
        if not 1 <= gw <= _lib.CL_GC_MAX_WINDOW:
            raise EngineError(-1, "gc_window outside [1, 1024]")
        if not 0 <= gk < gw:
            raise EngineError(-1, "gc_max_invalid is not below gc_window")
        enc = lambda p: p.encode() if p else None          # noqa: E731
        go = _lib.dut_gc_options(enc(gc_bias), enc(gc_summary), gw, gk)
        to = bo = None
        if targets is not None:
            thr = [int(t) for t in ((1, 10, 20, 30) if target_thresholds is None else target_thresholds)]
            if any(t < 0 or t > 0xFFFFFFFF for t in thr):
                raise EngineError(-1, "target_thresholds outside [0, 2^32 - 1]")
            ta = (C.c_uint32 * max(len(thr), 1))(*thr)
            to = _lib.dut_target_options(targets.encode(), target_out.encode(), ta, len(thr))
        if depth_bed:
            from .callable_loci import quantize_parse
            if depth_bed_kind not in _lib.CL_DEPTH_KINDS:
                raise EngineError(-1, f"depth_bed_kind {depth_bed_kind!r}: raw or qc")
            edges = quantize_parse(quantize)
            ea = (C.c_uint32 * max(len(edges), 1))(*edges)
            bo = _lib.dut_depth_bed_options(depth_bed.encode(), _lib.CL_DEPTH_KINDS[depth_bed_kind], ea, len(edges))
        dlist = [int(d) for d in devices] if devices is not None else [int(device_id)]
        dv = (C.c_int * len(dlist))(*dlist)
        do = _lib.dut_depth_options(int(depth_cap) + 1, int(window), enc(depth_dist), enc(depth_windows), enc(depth_summary))
        st = lib.dut_coverage_files_ex5(bam_file.encode(), reference_file.encode(), output_bed.encode(), enc(summary_json),
                                        enc(output_summary), C.byref(oc), arr, n, dv, len(dlist), 0, C.byref(do),
                                        C.byref(bo) if bo is not None else None, C.byref(to) if to is not None else None,
                                        _lib.DUT_TARGETS_ORDER if target_quantiles else 0, C.byref(go), err, 1024)
        if st != 0:
            raise EngineError(st, err.value.decode())
        return
    if targets is not None:
        thr = [int(t) for t in ((1, 10, 20, 30) if target_thresholds is None else target_thresholds)]
        if any(t < 0 or t > 0xFFFFFFFF for t in thr):
            raise EngineError(-1, "target_thresholds outside [0, 2^32 - 1]")
        ta = (C.c_uint32 * max(len(thr), 1))(*thr)
        to = _lib.dut_target_options(targets.encode(), target_out.encode(), ta, len(thr))
        bo = None
        if depth_bed is None and (quantize is not None or depth_bed_kind != "raw"):
            raise EngineError(-1, "quantize and depth_bed_kind need depth_bed")
        if depth_bed:
            from .callable_loci import quantize_parse
            if depth_bed_kind not in _lib.CL_DEPTH_KINDS:
                raise EngineError(-1, f"depth_bed_kind {depth_bed_kind!r}: raw or qc")
            edges = quantize_parse(quantize)
            ea = (C.c_uint32 * max(len(edges), 1))(*edges)
            bo = _lib.dut_depth_bed_options(depth_bed.encode(), _lib.CL_DEPTH_KINDS[depth_bed_kind], ea, len(edges))
        dlist = [int(d) for d in devices] if devices is not None else [int(device_id)]
        dv = (C.c_int * len(dlist))(*dlist)
        enc = lambda p: p.encode() if p else None          # noqa: E731
        do = _lib.dut_depth_options(int(depth_cap) + 1, int(window), enc(depth_dist), enc(depth_windows), enc(depth_summary))
        st = lib.dut_coverage_files_ex4(bam_file.encode(), reference_file.encode(), output_bed.encode(), enc(summary_json),
                                        enc(output_summary), C.byref(oc), arr, n, dv, len(dlist), 0, C.byref(do),
                                        C.byref(bo) if bo is not None else None, C.byref(to),
                                        _lib.DUT_TARGETS_ORDER if target_quantiles else 0, err, 1024)
        if st != 0:
            raise EngineError(st, err.value.decode())
        return
    if depth_bed:
        from .callable_loci import quantize_parse
        if depth_bed_kind not in _lib.CL_DEPTH_KINDS:
            raise EngineError(-1, f"depth_bed_kind {depth_bed_kind!r}: raw or qc")
        edges = quantize_parse(quantize)
        ea = (C.c_uint32 * max(len(edges), 1))(*edges)
        bo = _lib.dut_depth_bed_options(depth_bed.encode(), _lib.CL_DEPTH_KINDS[depth_bed_kind], ea, len(edges))
        dlist = [int(d) for d in devices] if devices is not None else [int(device_id)]
        dv = (C.c_int * len(dlist))(*dlist)
        enc = lambda p: p.encode() if p else None          # noqa: E731
        do = _lib.dut_depth_options(int(depth_cap) + 1, int(window), enc(depth_dist), enc(depth_windows), enc(depth_summary))
        st = lib.dut_coverage_files_ex2(bam_file.encode(), reference_file.encode(), output_bed.encode(), enc(summary_json),
                                        enc(output_summary), C.byref(oc), arr, n, dv, len(dlist), 0, C.byref(do), C.byref(bo), err, 1024)
    elif depth_dist or depth_windows or depth_summary:
        dlist = [int(d) for d in devices] if devices is not None else [int(device_id)]
        dv = (C.c_int * len(dlist))(*dlist)
        enc = lambda p: p.encode() if p else None          # noqa: E731
        do = _lib.dut_depth_options(int(depth_cap) + 1, int(window), enc(depth_dist), enc(depth_windows), enc(depth_summary))
        st = lib.dut_coverage_files_ex(bam_file.encode(), reference_file.encode(), output_bed.encode(), enc(summary_json),
                                       enc(output_summary), C.byref(oc), arr, n, dv, len(dlist), 0, C.byref(do), err, 1024)
    elif devices is not None:
        dv = (C.c_int * len(devices))(*[int(d) for d in devices])
        st = lib.dut_coverage_files_multi(bam_file.encode(), reference_file.encode(), output_bed.encode(),
                                          summary_json.encode() if summary_json else None, output_summary.encode() if output_summary else None,
                                          C.byref(oc), arr, n, dv, len(devices), 0, err, 1024)
    else:
        st = lib.dut_coverage_files(bam_file.encode(), reference_file.encode(), output_bed.encode(),
                                    summary_json.encode() if summary_json else None, output_summary.encode() if output_summary else None,
                                    C.byref(oc), arr, n, device_id, err, 1024)
    if st != 0:
        raise EngineError(st, err.value.decode())
