"""`find-variants`: where a sample differs from the reference at all, and which of those differences the haplogroup
tree does not know (include/dut_variants.h).  The counting and the call run on the device (Engine.site_scan); this module
holds the host side: the per-position classification in plain code, the annotation against a tree, the TSV."""
import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .callable_loci import (DEL_CANDIDATE, INS_CANDIDATE, INS_OBS, MINOR_CANDIDATE, SCAN_CANDIDATE, SCAN_CANDIDATE_EX, ConsResult, DelResult,
                            EngineError, ErrorProfile, InsResult, LinkResult, MinorResult, ScanResult, StrResult, _ptr)
from .haplogroup import FTDNA, YDNA, HaplogroupTree

LOW_DEPTH, MIXED, UNCOMPARABLE, MATCH, VARIANT, UNDETERMINED = range(6)
MINOR_LOW_DEPTH, MINOR_SINGLE, MINOR_MINOR = range(3)
MINOR_CLASS_NAMES = ("low_depth", "single", "minor")
DEL_LOW_DEPTH, DEL_KEPT, DEL_DELETED = range(3)
DEL_CLASS_NAMES = ("low_depth", "kept", "deleted")
INS_LOW_DEPTH, INS_KEPT, INS_INSERTED = range(3)
INS_CLASS_NAMES = ("low_depth", "kept", "inserted")
INS_CODES = "=ACMGRSVTWYHKDBN"
CONS_LOW_DEPTH, CONS_DELETED, CONS_NO_CALL, CONS_REF, CONS_ALT = range(5)
CONS_CLASS_NAMES = ("low_depth", "deleted", "no_call", "ref", "alt")
CONS_KINDS = ("snv", "del", "ins", "ins_skipped")
CONS_NOTES = ("", "anchor_deleted", "too_long", "no_allele")
CLASS_NAMES = ("low_depth", "mixed", "uncomparable", "match", "variant", "undetermined")
STR_LOW_DEPTH, STR_MIXED, STR_CALLED = range(3)
STR_STATUS_NAMES = ("low_depth", "mixed", "called")
LINK_LOW_DEPTH, LINK_CIS, LINK_TRANS, LINK_UNRESOLVED = range(4)
LINK_STATUS_NAMES = ("low_depth", "cis", "trans", "unresolved")


def _classify(fn, counts, width, ref_byte, min_depth) -> Tuple[int, str]:
    arr = np.ascontiguousarray(counts, np.uint32)
    if arr.shape != (width,):
        raise ValueError(f"expected {width} counters")
    if isinstance(ref_byte, (str, bytes)):
        ref_byte = ord(ref_byte)
    called = C.create_string_buffer(2)
    st = fn(arr.ctypes.data, int(ref_byte), int(min_depth), called)
    if st < 0:
        raise EngineError(st, "invalid counters")
    return st, called.value.decode()


def scan_classify(hist16, ref_byte, min_depth) -> Tuple[int, str]:
    """(class, called base or '') of one position from its 16-code histogram, by the f64 rule of caller.rs:132-149."""
    return _classify(_lib.load().dut_scan_classify, hist16, 16, ref_byte, min_depth)


def scan_classify_counts(counts5, ref_byte, min_depth) -> Tuple[int, str]:
    """The same from (a, c, g, t, depth) of Engine.site_scan_counts; UNDETERMINED when the other codes hold 0.7 together."""
    return _classify(_lib.load().dut_scan_classify_counts, counts5, 5, ref_byte, min_depth)


def _candidates(candidates) -> np.ndarray:
    cand = np.ascontiguousarray(candidates, SCAN_CANDIDATE)
    return cand.reshape(-1)


def annotate_variants(tree: HaplogroupTree, build_id: str, chromosome: str, candidates) -> List[Tuple[bool, str, str]]:
    """Per candidate (known, names, alleles): dut_variants_annotate; names and alleles are '' for a novel one."""
    lib = _lib.load()
    cand = _candidates(candidates)
    notes = C.POINTER(_lib.dut_variant_note)()
    st = lib.dut_variants_annotate(tree._h, build_id.encode(), chromosome.encode(), cand.ctypes.data, cand.shape[0], C.byref(notes))
    if st != 0:
        raise EngineError(st, "annotation failed")
    try:
        return [(bool(notes[i].known), (notes[i].names or b"").decode(), (notes[i].alleles or b"").decode())
                for i in range(cand.shape[0])]
    finally:
        lib.dut_variants_free_notes(notes, cand.shape[0])


def _call(fn, *args, size=512):
    """fn(*args, err, size) of the library; an EngineError with its message unless it answers 0."""
    err = C.create_string_buffer(size)
    st = fn(*args, err, size)
    if st != 0:
        raise EngineError(st, err.value.decode())


def _c_result(ctype, cand_ctype, dtype, result, what, **counts):
    """(the C result struct of `result` with its n_* counts, the candidates as a contiguous array that it points to)."""
    cand = np.ascontiguousarray(result.candidates, dtype).reshape(-1)
    if cand.shape[0] != getattr(result, what):
        raise ValueError(f"{what} count and candidates disagree")
    r = ctype()
    r.start, r.end = result.start, result.end
    for name, v in counts.items():
        setattr(r, name, v)
    r.candidates = C.cast(cand.ctypes.data, C.POINTER(cand_ctype))
    return r, cand


def _find_files(fn, bam_file, reference_file, contig, region, *rest):
    """A dut_find_*_files: the paths, the region as (has_region, start, end), then `rest`."""
    start, end = region if region is not None else (0, 0)
    _call(fn, bam_file.encode(), reference_file.encode(), contig.encode(), 1 if region is not None else 0, int(start), int(end), *rest, size=1024)


def _scan_result(ctype, cand_ctype, dtype, result):
    return _c_result(ctype, cand_ctype, dtype, result, "variant", n_low_depth=result.low_depth, n_mixed=result.mixed,
                     n_uncomparable=result.uncomparable, n_match=result.match, n_variant=result.variant)


def _write_variants(writer, annotate, r, cand, path, contig, args, tree, build_id):
    """The TSV of the C result r over cand by `writer`, annotated by `annotate` when there is a tree."""
    lib = _lib.load()
    notes = C.POINTER(_lib.dut_variant_note)()
    if tree is not None:
        if not build_id:
            raise ValueError("a tree needs its build id")
        st = annotate(tree._h, build_id.encode(), contig.encode(), cand.ctypes.data, cand.shape[0], C.byref(notes))
        if st != 0:
            raise EngineError(st, "annotation failed")
    try:
        _call(writer, path.encode(), contig.encode(), C.byref(r), *args, notes if tree is not None else None)
    finally:
        if tree is not None:
            lib.dut_variants_free_notes(notes, cand.shape[0])


def write_variants(path: str, contig: str, result: ScanResult, min_depth: int, min_quality: int,
                   tree: Optional[HaplogroupTree] = None, build_id: Optional[str] = None):
    """The TSV of find-variants for a ScanResult; with a tree (and its build id) the candidates are annotated."""
    lib = _lib.load()
    r, cand = _scan_result(_lib.cl_scan_result, _lib.cl_scan_candidate, SCAN_CANDIDATE, result)
    _write_variants(lib.dut_variants_write, lib.dut_variants_annotate, r, cand, path, contig, (int(min_depth), int(min_quality)), tree, build_id)


def _filter_options(o, min_base_quality, exclude_flags):
    """The filter fields every options struct has, checked and set."""
    if min_base_quality is not None and not 0 <= int(min_base_quality) <= 255:
        raise ValueError("min_base_quality: 0..255")
    if not 0 <= int(exclude_flags) <= 0xFFFF:
        raise ValueError("exclude_flags: 0..65535")
    o.has_min_base_quality = 0 if min_base_quality is None else 1
    o.min_base_quality = 0 if min_base_quality is None else int(min_base_quality)
    o.exclude_flags = int(exclude_flags)
    return o


def _options(min_base_quality, exclude_flags, min_alt_per_strand) -> "_lib.dut_variants_options":
    o = _filter_options(_lib.dut_variants_options(), min_base_quality, exclude_flags)
    if not 0 <= int(min_alt_per_strand) <= 0xFFFFFFFF:
        raise ValueError("min_alt_per_strand: 0..2^32-1")
    o.filtered = 1
    o.min_alt_per_strand = int(min_alt_per_strand)
    return o


def write_variants_ex(path: str, contig: str, result: ScanResult, min_depth: int, min_quality: int, min_base_quality=None,
                      exclude_flags: int = 0, min_alt_per_strand: int = 0, tree: Optional[HaplogroupTree] = None,
                      build_id: Optional[str] = None):
    """The extended TSV (dut_variants_write_ex) for the ScanResult of Engine.site_scan_ex: per-strand counts and the
    strand filter; min_base_quality=None prints '.'.  No device is needed."""
    lib = _lib.load()
    r, cand = _scan_result(_lib.cl_scan_result_ex, _lib.cl_scan_candidate_ex, SCAN_CANDIDATE_EX, result)
    opt = _options(min_base_quality, exclude_flags, min_alt_per_strand)
    _write_variants(lib.dut_variants_write_ex, lib.dut_variants_annotate_ex, r, cand, path, contig, (int(min_depth), int(min_quality), C.byref(opt)),
                    tree, build_id)


def find_variants(bam_file: str, reference_file: str, contig: str, output_file: str, region: Optional[Tuple[int, int]] = None,
                  tree_json: Optional[str] = None, provider: int = FTDNA, tree_type: int = YDNA, min_depth: int = 10,
                  min_quality: int = 20, device_id: int = 0, min_base_quality: Optional[int] = None, exclude_flags: int = 0,
                  min_alt_per_strand: int = 0):
    """dut_find_variants_files(_ex): BAM (+ index) and FASTA in, the TSV out; region = (start, end), 0-based half open.
    With min_base_quality, exclude_flags or min_alt_per_strand the scan is the filtered, strand-aware one and the TSV the
    extended one; with none of them nothing changes."""
    opt = None
    if min_base_quality is not None or exclude_flags or min_alt_per_strand:
        opt = C.byref(_options(min_base_quality, exclude_flags, min_alt_per_strand))
    _find_files(_lib.load().dut_find_variants_files_ex, bam_file, reference_file, contig, region, tree_json.encode() if tree_json else None, provider,
                tree_type, output_file.encode(), int(min_depth), int(min_quality), opt, device_id)


def _fraction_parse(fn, text: str) -> int:
    v = C.c_uint32()
    err = C.create_string_buffer(256)
    st = fn(text.encode(), C.byref(v), err, 256)
    if st != 0:
        raise ValueError(f"invalid fraction '{text}': {err.value.decode()}")
    return int(v.value)


def minor_fraction_parse(text: str) -> int:
    """dut_minor_fraction_parse: decimal text in (0, 0.5] with at most four decimals to parts per 10 000, exactly."""
    return _fraction_parse(_lib.load().dut_minor_fraction_parse, text)


def minor_classify_counts(a, c, g, t, depth, min_depth, min_minor_count, min_minor_per_10k) -> Tuple[int, str, str]:
    """(class, major, minor) of one position by the rule of cl_site_scan_minor in plain code (dut_minor_classify_counts)."""
    prm = _lib.cl_minor_params(int(min_depth), int(min_minor_count), int(min_minor_per_10k))
    major, minor = C.create_string_buffer(2), C.create_string_buffer(2)
    st = _lib.load().dut_minor_classify_counts(int(a), int(c), int(g), int(t), int(depth), C.byref(prm), major, minor)
    if st < 0:
        raise EngineError(st, "invalid counters or parameters")
    return st, major.value.decode(), minor.value.decode()


def _rule_options(stem, min_depth, min_quality, count, per_10k, min_base_quality, exclude_flags, per_strand):
    """dut_minor_options (stem "minor"), dut_del_options ("del") or dut_ins_options ("ins"): the same members under the
    rule's names."""
    o = _filter_options(getattr(_lib, f"dut_{stem}_options")(), min_base_quality, exclude_flags)
    if not 0 <= int(min_quality) <= 255:
        raise ValueError("min_quality: 0..255")
    own = {f"min_{stem}_count": count, f"min_{stem}_per_10k": per_10k, f"min_{stem}_per_strand": per_strand}
    for name, v in (("min_depth", min_depth), *own.items()):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{name}: 0..2^32-1")
    o.min_depth, o.min_quality = int(min_depth), int(min_quality)
    for name, v in own.items():
        setattr(o, name, int(v))
    return o


def write_minor(path: str, contig: str, result: MinorResult, min_depth: int, min_quality: int, min_minor_count: int,
                min_minor_per_10k: int, min_base_quality=None, exclude_flags: int = 0, min_minor_per_strand: int = 0):
    """The TSV of find-minor-alleles (dut_minor_write) for the MinorResult of Engine.site_scan_minor.  No device is needed."""
    r, _cand = _c_result(_lib.cl_minor_result, _lib.cl_minor_candidate, MINOR_CANDIDATE, result, "minor", n_low_depth=result.low_depth,
                         n_single=result.single, n_minor=result.minor)
    opt = _rule_options("minor", min_depth, min_quality, min_minor_count, min_minor_per_10k, min_base_quality, exclude_flags, min_minor_per_strand)
    _call(_lib.load().dut_minor_write, path.encode(), contig.encode(), C.byref(r), C.byref(opt))


def find_minor_alleles(bam_file: str, reference_file: str, contig: str, output_file: str, region: Optional[Tuple[int, int]] = None,
                       min_depth: int = 10, min_quality: int = 20, min_minor_fraction="0.05", min_minor_count: int = 3,
                       min_base_quality: Optional[int] = None, exclude_flags: int = 0, min_minor_per_strand: int = 0, device_id: int = 0):
    """dut_find_minor_files: BAM (+ index) and FASTA in, the TSV of second alleles out; region = (start, end), 0-based half
    open.  min_minor_fraction: decimal text (or a number whose text is one) in (0, 0.5], at most four decimals."""
    per_10k = minor_fraction_parse(str(min_minor_fraction))
    opt = _rule_options("minor", min_depth, min_quality, min_minor_count, per_10k, min_base_quality, exclude_flags, min_minor_per_strand)
    _find_files(_lib.load().dut_find_minor_files, bam_file, reference_file, contig, region, C.byref(opt), output_file.encode(), device_id)


def del_fraction_parse(text: str) -> int:
    """dut_del_fraction_parse: decimal text in (0, 1] with at most four decimals to parts per 10 000, exactly."""
    return _fraction_parse(_lib.load().dut_del_fraction_parse, text)


def del_classify_counts(n_del, depth, min_depth, min_del_count, min_del_per_10k) -> int:
    """The class of one position by the rule of cl_site_scan_dels in plain code (dut_del_classify_counts)."""
    prm = _lib.cl_del_params(int(min_depth), int(min_del_count), int(min_del_per_10k))
    st = _lib.load().dut_del_classify_counts(int(n_del), int(depth), C.byref(prm))
    if st < 0:
        raise EngineError(st, "invalid parameters")
    return st


def del_events(candidates) -> List[dict]:
    """dut_del_events: the candidates (DEL_CANDIDATE, ascending position) merged into events, one per maximal run of
    consecutive positions: start, end (1-based, inclusive), length, and of the position q where del is smallest (the first
    among equals) del, span, del_fwd, del_rev; max_del over the run."""
    cand = np.ascontiguousarray(candidates, DEL_CANDIDATE).reshape(-1)
    ev = C.POINTER(_lib.dut_del_event)()
    n = C.c_size_t()
    lib = _lib.load()
    st = lib.dut_del_events(cand.ctypes.data if cand.shape[0] else None, cand.shape[0], C.byref(ev), C.byref(n))
    if st != 0:
        raise EngineError(st, "candidate positions must ascend")
    try:
        return [dict(start=int(e.start), end=int(e.end), length=int(e.length), q=int(e.q), span=int(e.span), max_del=int(e.max_del),
                     del_fwd=int(e.del_fwd), del_rev=int(e.del_rev), **{"del": int(getattr(e, "del"))}) for e in ev[:n.value]]
    finally:
        lib.dut_del_events_free(ev)


def write_deletions(path: str, contig: str, result: DelResult, min_depth: int, min_quality: int, min_del_count: int,
                    min_del_per_10k: int, min_base_quality=None, exclude_flags: int = 0, min_del_per_strand: int = 0):
    """The TSV of find-deletions (dut_del_write) for the DelResult of Engine.site_scan_dels.  No device is needed."""
    r, _cand = _c_result(_lib.cl_del_result, _lib.cl_del_candidate, DEL_CANDIDATE, result, "deleted", n_low_depth=result.low_depth,
                         n_kept=result.kept, n_deleted=result.deleted)
    opt = _rule_options("del", min_depth, min_quality, min_del_count, min_del_per_10k, min_base_quality, exclude_flags, min_del_per_strand)
    _call(_lib.load().dut_del_write, path.encode(), contig.encode(), C.byref(r), C.byref(opt))


def find_deletions(bam_file: str, reference_file: str, contig: str, output_file: str, region: Optional[Tuple[int, int]] = None,
                   min_depth: int = 10, min_quality: int = 20, min_del_fraction="0.7", min_del_count: int = 3,
                   min_base_quality: Optional[int] = None, exclude_flags: int = 0, min_del_per_strand: int = 0, device_id: int = 0):
    """dut_find_deletions_files: BAM (+ index) and FASTA in, the TSV of deletion events out; region = (start, end), 0-based
    half open.  min_del_fraction: decimal text (or a number whose text is one) in (0, 1], at most four decimals."""
    per_10k = del_fraction_parse(str(min_del_fraction))
    opt = _rule_options("del", min_depth, min_quality, min_del_count, per_10k, min_base_quality, exclude_flags, min_del_per_strand)
    _find_files(_lib.load().dut_find_deletions_files, bam_file, reference_file, contig, region, C.byref(opt), output_file.encode(), device_id)


def ins_classify_counts(n_ins, depth, min_depth, min_ins_count, min_ins_per_10k) -> int:
    """The class of one position by the rule of cl_site_scan_ins in plain code (dut_ins_classify_counts)."""
    prm = _lib.cl_ins_params(int(min_depth), int(min_ins_count), int(min_ins_per_10k))
    st = _lib.load().dut_ins_classify_counts(int(n_ins), int(depth), C.byref(prm))
    if st < 0:
        raise EngineError(st, "invalid parameters")
    return st


def ins_key_text(length, key) -> str:
    """The inserted bases a key holds: the first min(length, 32), decoded with =ACMGRSVTWYHKDBN."""
    return "".join(INS_CODES[(int(key[j // 16]) >> (60 - 4 * (j % 16))) & 15] for j in range(min(int(length), 32)))


def ins_alleles(observations) -> List[dict]:
    """dut_ins_alleles: the observations (INS_OBS, any order) grouped into alleles of equal (len, key): ascending position,
    within a position the top allele first (most observations, then the smaller len, then the smaller key), the others by
    (len, key).  Per allele pos, len, key (two ints), seq (the first 32 bases), count, fwd, rev.  Insertions longer than 32
    bases that agree in length and in their first 32 bases are one allele."""
    obs = np.ascontiguousarray(observations, INS_OBS).reshape(-1)
    al = C.POINTER(_lib.dut_ins_allele)()
    n = C.c_size_t()
    lib = _lib.load()
    st = lib.dut_ins_alleles(obs.ctypes.data if obs.shape[0] else None, obs.shape[0], C.byref(al), C.byref(n))
    if st != 0:
        raise EngineError(st, "dut_ins_alleles failed")
    try:
        return [dict(pos=int(a.pos), len=int(a.len), key=(int(a.key[0]), int(a.key[1])), seq=ins_key_text(a.len, a.key), count=int(a.count),
                     fwd=int(a.fwd), rev=int(a.rev)) for a in al[:n.value]]
    finally:
        lib.dut_ins_alleles_free(al)


def write_insertions(path: str, contig: str, result: InsResult, min_depth: int, min_quality: int, min_ins_count: int,
                     min_ins_per_10k: int, min_base_quality=None, exclude_flags: int = 0, min_ins_per_strand: int = 0):
    """The TSV of find-insertions (dut_ins_write) for the InsResult of Engine.site_scan_ins.  No device is needed."""
    r, _cand = _c_result(_lib.cl_ins_result, _lib.cl_ins_candidate, INS_CANDIDATE, result, "inserted", n_low_depth=result.low_depth,
                         n_kept=result.kept, n_inserted=result.inserted)
    obs = np.ascontiguousarray(result.observations, INS_OBS).reshape(-1)
    r.n_obs = obs.shape[0]
    r.obs = C.cast(obs.ctypes.data, C.POINTER(_lib.cl_ins_obs))
    opt = _rule_options("ins", min_depth, min_quality, min_ins_count, min_ins_per_10k, min_base_quality, exclude_flags, min_ins_per_strand)
    _call(_lib.load().dut_ins_write, path.encode(), contig.encode(), C.byref(r), C.byref(opt))


def find_insertions(bam_file: str, reference_file: str, contig: str, output_file: str, region: Optional[Tuple[int, int]] = None,
                    min_depth: int = 10, min_quality: int = 20, min_ins_fraction="0.7", min_ins_count: int = 3,
                    min_base_quality: Optional[int] = None, exclude_flags: int = 0, min_ins_per_strand: int = 0, device_id: int = 0):
    """dut_find_insertions_files: BAM (+ index) and FASTA in, the TSV of insertions out; region = (start, end), 0-based half
    open.  min_ins_fraction: decimal text (or a number whose text is one) in (0, 1], at most four decimals."""
    per_10k = del_fraction_parse(str(min_ins_fraction))
    opt = _rule_options("ins", min_depth, min_quality, min_ins_count, per_10k, min_base_quality, exclude_flags, min_ins_per_strand)
    _find_files(_lib.load().dut_find_insertions_files, bam_file, reference_file, contig, region, C.byref(opt), output_file.encode(), device_id)


def cons_classify_counts(a, c, g, t, depth, n_del, min_depth, min_del_count, min_del_per_10k, ref_byte) -> Tuple[int, str]:
    """(class, byte) of one position by the rule of cl_site_scan_consensus in plain code (dut_cons_classify_counts)."""
    prm = _lib.cl_cons_params(int(min_depth), int(min_del_count), int(min_del_per_10k))
    if isinstance(ref_byte, (str, bytes)):
        ref_byte = ord(ref_byte)
    byte = C.create_string_buffer(2)
    st = _lib.load().dut_cons_classify_counts(int(a), int(c), int(g), int(t), int(depth), int(n_del), C.byref(prm), int(ref_byte), byte)
    if st < 0:
        raise EngineError(st, "invalid counters or parameters")
    return st, byte.value.decode()


class ConsAssembly:
    """dut_cons_assembly: seq (str), changes (dicts of pos, end, kind, ref, cons, count, depth, note) and the numbers of
    deletion runs, spliced and skipped insertions.  Holds the C structure for the writers until it is collected."""

    def __init__(self, c):
        self._c = c
        self.seq = C.string_at(c.seq, int(c.seq_len)).decode() if c.seq_len else ""
        self.changes = [dict(pos=int(x.pos), end=int(x.end), kind=CONS_KINDS[x.kind], ref=x.ref.decode(), cons=x.cons.decode(), count=int(x.count),
                             depth=int(x.depth), note=CONS_NOTES[x.note]) for x in c.changes[:c.n_changes]]
        self.deletions, self.insertions, self.insertions_skipped = int(c.n_deletions), int(c.n_insertions), int(c.n_insertions_skipped)

    def __del__(self):
        c, self._c = self._c, None
        if c is not None:
            _lib.load().dut_cons_assembly_free(C.byref(c))


def cons_assemble(cons, ref, start: int = 0, ins: Optional[InsResult] = None, min_depth: int = 10, min_ins_count: int = 3,
                  min_ins_per_10k: int = 7000, fill: str = "N") -> ConsAssembly:
    """dut_cons_assemble: the sequence and the change list of [start, start + len(cons)) from the bytes of
    Engine.site_scan_consensus.  ref: the whole reference the scans were given (its bytes from `start` on are used); ins: the
    InsResult of Engine.site_scan_ins over the same range and gates, with the parameters it was asked with; fill: "N" or
    "ref".  No device is needed."""
    if fill not in ("N", "ref"):
        raise ValueError("fill: N or ref")
    lib = _lib.load()
    cons = np.ascontiguousarray(cons, np.uint8).reshape(-1)
    ref = np.ascontiguousarray(ref, np.uint8).reshape(-1)
    start, end = int(start), int(start) + cons.shape[0]
    part = np.ascontiguousarray(ref[start:end])
    r = al = None
    n_al = C.c_size_t()
    prm = _lib.cl_ins_params(int(min_depth), int(min_ins_count), int(min_ins_per_10k))
    alp = C.POINTER(_lib.dut_ins_allele)()
    if ins is not None:
        r, _cand = _c_result(_lib.cl_ins_result, _lib.cl_ins_candidate, INS_CANDIDATE, ins, "inserted", n_low_depth=ins.low_depth, n_kept=ins.kept,
                             n_inserted=ins.inserted)
        obs = np.ascontiguousarray(ins.observations, INS_OBS).reshape(-1)
        st = lib.dut_ins_alleles(obs.ctypes.data if obs.shape[0] else None, obs.shape[0], C.byref(alp), C.byref(n_al))
        if st != 0:
            raise EngineError(st, "dut_ins_alleles failed")
    out = _lib.dut_cons_assembly()
    try:
        st = lib.dut_cons_assemble(cons.ctypes.data if cons.shape[0] else None, start, end, part.ctypes.data if part.shape[0] else None, part.shape[0],
                                   C.byref(r) if r is not None else None, C.cast(alp, C.c_void_p), n_al.value, C.byref(prm), 1 if fill == "ref" else 0,
                                   C.byref(out))
    finally:
        lib.dut_ins_alleles_free(alp)
    if st != 0:
        raise EngineError(st, "dut_cons_assemble refused its arguments")
    return ConsAssembly(out)


def _cons_options(min_depth, min_quality, min_del_count, min_del_per_10k, min_ins_count, min_ins_per_10k, min_base_quality, exclude_flags, fill, line_width):
    if fill not in ("N", "ref"):
        raise ValueError("fill: N or ref")
    o = _filter_options(_lib.dut_cons_options(), min_base_quality, exclude_flags)
    if not 0 <= int(min_quality) <= 255:
        raise ValueError("min_quality: 0..255")
    for name, v in (("min_depth", min_depth), ("min_del_count", min_del_count), ("min_del_per_10k", min_del_per_10k), ("min_ins_count", min_ins_count),
                    ("min_ins_per_10k", min_ins_per_10k), ("line_width", line_width)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{name}: 0..2^32-1")
        setattr(o, name, int(v))
    o.min_quality = int(min_quality)
    o.fill_ref = 1 if fill == "ref" else 0
    return o


def write_consensus(path: str, contig: str, assembly: ConsAssembly, start: int, end: int, whole_contig: bool = False, line_width: int = 60):
    """The FASTA of `consensus` (dut_cons_write_fasta): ">contig" for the whole contig, else ">contig:START-END" (1-based,
    inclusive).  No device is needed."""
    seq = assembly.seq.encode()
    _call(_lib.load().dut_cons_write_fasta, path.encode(), contig.encode(), 1 if whole_contig else 0, int(start), int(end), seq, len(seq), int(line_width))


def write_consensus_changes(path: str, contig: str, result: ConsResult, assembly: ConsAssembly, min_depth: int = 10, min_quality: int = 20,
                            min_del_count: int = 3, min_del_per_10k: int = 7000, min_ins_count: int = 3, min_ins_per_10k: int = 7000,
                            min_base_quality=None, exclude_flags: int = 0, fill: str = "N"):
    """The change list of `consensus` (dut_cons_write_changes) for a ConsResult and its assembly.  No device is needed."""
    r = _lib.cl_cons_result()
    r.start, r.end = result.start, result.end
    r.n_low_depth, r.n_deleted, r.n_no_call, r.n_ref, r.n_alt = result.low_depth, result.deleted, result.no_call, result.ref, result.alt
    opt = _cons_options(min_depth, min_quality, min_del_count, min_del_per_10k, min_ins_count, min_ins_per_10k, min_base_quality, exclude_flags, fill, 60)
    _call(_lib.load().dut_cons_write_changes, path.encode(), contig.encode(), C.byref(r), C.byref(assembly._c), C.byref(opt))


def consensus(bam_file: str, reference_file: str, contig: str, output_file: str, region: Optional[Tuple[int, int]] = None, min_depth: int = 10,
              min_quality: int = 20, min_del_fraction="0.7", min_del_count: int = 3, min_ins_fraction="0.7", min_ins_count: int = 3,
              min_base_quality: Optional[int] = None, exclude_flags: int = 0, fill: str = "N", line_width: int = 60,
              changes_file: Optional[str] = None, device_id: int = 0):
    """dut_find_consensus_files: BAM (+ index) and FASTA in, the sample's sequence over the contig or the region as FASTA
    out, and with changes_file the list of its differences from the reference; region = (start, end), 0-based half open.
    The fractions: decimal text (or a number whose text is one) in (0, 1], at most four decimals."""
    opt = _cons_options(min_depth, min_quality, min_del_count, del_fraction_parse(str(min_del_fraction)), min_ins_count,
                        del_fraction_parse(str(min_ins_fraction)), min_base_quality, exclude_flags, fill, line_width)
    _find_files(_lib.load().dut_find_consensus_files, bam_file, reference_file, contig, region, C.byref(opt), output_file.encode(),
                changes_file.encode() if changes_file else None, device_id)


def str_measure(rec, contig_len: int, loci, flank: int, min_quality: int, exclude_flags: Optional[int] = None) -> StrResult:
    """dut_str_measure: what Engine.site_str_lengths returns, from the records on the host (no device needed).
    exclude_flags=None: one strand, no flag takes part; a mask (0 included): two strands, forward first."""
    loci = np.ascontiguousarray(loci, np.uint32).reshape(-1, 2)
    strands = 1 if exclude_flags is None else 2
    hist = np.zeros((loci.shape[0], strands, _lib.CL_STR_BINS), np.uint32)
    partial = np.zeros(loci.shape[0], np.uint32)
    pos, mapq = np.ascontiguousarray(rec.pos, np.int32), np.ascontiguousarray(rec.mapq, np.uint8)
    flag = np.ascontiguousarray(rec.flag, np.uint16)
    cigar_off, cigar = np.ascontiguousarray(rec.cigar_off, np.uint32), np.ascontiguousarray(rec.cigar, np.uint32)
    st = _lib.load().dut_str_measure(_ptr(pos), _ptr(flag), _ptr(mapq), _ptr(cigar_off), _ptr(cigar), int(rec.n), int(contig_len), int(min_quality),
                                     int(exclude_flags or 0), int(flank), _ptr(loci) if loci.shape[0] else None, loci.shape[0],
                                     _ptr(hist) if loci.shape[0] else None, _ptr(partial) if loci.shape[0] else None, strands)
    if st != 0:
        raise EngineError(st, "dut_str_measure refused its arguments")
    return StrResult(hist=hist, partial=partial)


def str_call(hist_fwd, hist_rev=None, min_depth: int = 10, min_allele_per_10k: int = 7000) -> dict:
    """dut_str_call: the allele of one locus from its histogram(s) of 128 bins -- status (STR_LOW_DEPTH, STR_MIXED,
    STR_CALLED), n, other, the top allele's delta, count, fwd, rev and the second's delta2, count2."""
    hf = np.ascontiguousarray(hist_fwd, np.uint32).reshape(-1)
    hr = None if hist_rev is None else np.ascontiguousarray(hist_rev, np.uint32).reshape(-1)
    if hf.shape[0] != _lib.CL_STR_BINS or (hr is not None and hr.shape[0] != _lib.CL_STR_BINS):
        raise ValueError("a histogram has 128 bins")
    prm = _lib.dut_str_params(int(min_depth), int(min_allele_per_10k))
    c = _lib.dut_str_allele_call()
    st = _lib.load().dut_str_call(_ptr(hf), _ptr(hr), C.byref(prm), C.byref(c))
    if st != 0:
        raise EngineError(st, "invalid parameters")
    return dict(status=int(c.status), n=int(c.n), other=int(c.other), delta=int(c.delta), count=int(c.count), fwd=int(c.fwd), rev=int(c.rev),
                delta2=int(c.delta2), count2=int(c.count2))


def str_units(span: int, delta: int, period: int) -> str:
    """dut_str_units: span + delta bases in units of `period`, "9.3" for nine units and three bases."""
    buf = C.create_string_buffer(_lib.DUT_STR_UNITS_LEN)
    if not (0 <= int(span) <= 0xFFFFFFFF and -2 ** 31 <= int(delta) < 2 ** 31 and 0 <= int(period) <= 0xFFFFFFFF):
        raise ValueError("span, delta or period out of range")
    st = _lib.load().dut_str_units(int(span), int(delta), int(period), buf)
    if st != 0:
        raise EngineError(st, "period outside 1..255 or a length below zero")
    return buf.value.decode()


def str_loci_parse(path: str, contig: str) -> Tuple[List[dict], int]:
    """dut_str_loci_parse: (the loci of `contig` in file order as dicts of start, end, period, name; the lines of other
    contigs).  An EngineError names a malformed line by its number."""
    lib = _lib.load()
    lp = C.POINTER(_lib.dut_str_locus)()
    n, skipped = C.c_size_t(), C.c_size_t()
    _call(lib.dut_str_loci_parse, path.encode(), contig.encode(), C.byref(lp), C.byref(n), C.byref(skipped))
    try:
        return [dict(start=int(l.start), end=int(l.end), period=int(l.period), name=l.name.decode()) for l in lp[:n.value]], int(skipped.value)
    finally:
        lib.dut_str_loci_free(lp)


def _str_options(min_depth, min_quality, exclude_flags, flank, min_allele_fraction):
    if not 0 <= int(min_quality) <= 255:
        raise ValueError("min_quality: 0..255")
    if not 0 <= int(exclude_flags) <= 0xFFFF:
        raise ValueError("exclude_flags: 0..65535")
    for name, v in (("min_depth", min_depth), ("flank", flank)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{name}: 0..2^32-1")
    return _lib.dut_str_options(int(min_depth), int(min_quality), int(exclude_flags), int(flank), del_fraction_parse(str(min_allele_fraction)))


def write_strs(path: str, contig: str, loci, result: StrResult, loci_skipped: int = 0, flank: int = 5, min_depth: int = 10, min_quality: int = 20,
               min_allele_fraction="0.7", exclude_flags: int = 0):
    """The TSV of find-strs (dut_str_write) for loci (dicts of start, end, period, name, as str_loci_parse returns them) and
    the StrResult of Engine.site_str_lengths or str_measure over them.  No device is needed."""
    arr = (_lib.dut_str_locus * max(len(loci), 1))()
    for i, l in enumerate(loci):
        arr[i].start, arr[i].end, arr[i].period, arr[i].name = int(l["start"]), int(l["end"]), int(l["period"]), l["name"].encode()
    hist = np.ascontiguousarray(result.hist, np.uint32)
    partial = np.ascontiguousarray(result.partial, np.uint32)
    if hist.ndim != 3 or hist.shape[0] != len(loci) or hist.shape[2] != _lib.CL_STR_BINS or partial.shape != (len(loci),):
        raise ValueError("the result does not belong to these loci")
    opt = _str_options(min_depth, min_quality, exclude_flags, flank, min_allele_fraction)
    _call(_lib.load().dut_str_write, path.encode(), contig.encode(), arr, len(loci), int(loci_skipped), _ptr(hist) if len(loci) else None,
          _ptr(partial) if len(loci) else None, int(hist.shape[1]), C.byref(opt))


def find_strs(bam_file: str, reference_file: str, contig: str, loci_file: str, output_file: str, flank: int = 5, min_depth: int = 10,
              min_quality: int = 20, min_allele_fraction="0.7", exclude_flags: int = 0, device_id: int = 0):
    """dut_find_strs_files: BAM (+ index), FASTA and a loci file (contig start end period name, tab separated, 0-based half
    open) in, the TSV of repeat alleles out.  min_allele_fraction: decimal text in (0, 1], at most four decimals."""
    opt = _str_options(min_depth, min_quality, exclude_flags, flank, min_allele_fraction)
    _call(_lib.load().dut_find_strs_files, bam_file.encode(), reference_file.encode(), contig.encode(), loci_file.encode(), C.byref(opt),
          output_file.encode(), device_id, size=1024)


def _ep_options(n_cycles, min_quality, exclude_flags, min_base_quality, filtered=True):
    if not 0 <= int(min_quality) <= 255:
        raise ValueError("min_quality: 0..255")
    if not 0 <= int(exclude_flags) <= 0xFFFF:
        raise ValueError("exclude_flags: 0..65535")
    if min_base_quality is not None and not 0 <= int(min_base_quality) <= 255:
        raise ValueError("min_base_quality: 0..255")
    if not 0 <= int(n_cycles) <= 0xFFFFFFFF:
        raise ValueError("n_cycles: 0..2^32-1 (the library refuses what lies outside 1..256)")
    return _lib.dut_ep_options(int(min_quality), 1 if filtered else 0, int(exclude_flags), 0 if min_base_quality is None else 1,
                               int(min_base_quality or 0), int(n_cycles))


def error_profile_measure(rec, contig_len: int, ref, n_cycles: int, min_quality: int, start: int = 0, end: Optional[int] = None,
                          exclude_flags: Optional[int] = None, min_base_quality: Optional[int] = None) -> ErrorProfile:
    """dut_error_profile_measure: what Engine.site_error_profile returns, from the records on the host (no device needed).
    exclude_flags=None: the unfiltered form, every read forward; a mask (0 included): the filtered form, with
    min_base_quality (None: every base passes) taken over the records' quality values."""
    ref = np.ascontiguousarray(ref, np.uint8)
    end = ref.shape[0] if end is None else end
    keep = [np.ascontiguousarray(rec.pos, np.int32), np.ascontiguousarray(rec.flag, np.uint16), np.ascontiguousarray(rec.mapq, np.uint8),
            np.ascontiguousarray(rec.cigar_off, np.uint32), np.ascontiguousarray(rec.cigar, np.uint32),
            np.ascontiguousarray(rec.seq_off if rec.seq_off is not None else np.zeros(rec.n + 1, np.uint64), np.uint64),
            np.ascontiguousarray(rec.seq4 if rec.seq4 is not None else np.zeros(0, np.uint8), np.uint8),
            np.ascontiguousarray(rec.qual_off, np.uint64), np.ascontiguousarray(rec.qual, np.uint8)]
    reads = _lib.dut_ep_reads(rec.n, *[a.ctypes.data if a.shape[0] else None for a in keep])
    opt = _ep_options(n_cycles, min_quality, exclude_flags or 0, min_base_quality if exclude_flags is not None else None, exclude_flags is not None)
    tables = np.zeros(36 * max(int(n_cycles), 1), np.uint64)
    r = _lib.cl_ep_result()
    st = _lib.load().dut_error_profile_measure(C.byref(reads), int(contig_len), _ptr(ref) if ref.shape[0] else None, ref.shape[0], int(start), int(end),
                                               C.byref(opt), _ptr(tables), C.byref(r))
    if st != 0:
        raise EngineError(st, "dut_error_profile_measure refused its arguments")
    return ErrorProfile.from_c(r)


def write_error_profile(path: str, contig: str, result: ErrorProfile, min_quality: int = 20, min_base_quality: Optional[int] = None,
                        exclude_flags: int = 0):
    """The TSV of error-profile (dut_error_profile_write) for an ErrorProfile of Engine.site_error_profile or
    error_profile_measure.  No device is needed."""
    r, keep = result.to_c()
    opt = _ep_options(result.n_cycles, min_quality, exclude_flags, min_base_quality)
    _call(_lib.load().dut_error_profile_write, path.encode(), contig.encode(), C.byref(r), C.byref(opt))
    del keep


def error_profile(bam_file: str, reference_file: str, contig: str, output_file: str, region: Optional[Tuple[int, int]] = None, cycles: int = 50,
                  min_quality: int = 20, min_base_quality: Optional[int] = None, exclude_flags: int = 0, device_id: int = 0):
    """dut_error_profile_files: BAM (+ index) and FASTA in, the TSV of substitutions and indels by read cycle out.
    region: (start, end), 0-based half open, or None for the whole contig."""
    opt = _ep_options(cycles, min_quality, exclude_flags, min_base_quality)
    _find_files(_lib.load().dut_error_profile_files, bam_file, reference_file, contig, region, C.byref(opt), output_file.encode(), device_id)


def link_discordance_parse(text: str) -> int:
    """dut_link_discordance_parse: decimal text in [0, 0.4999] with at most four decimals to parts per 10 000, exactly."""
    return _fraction_parse(_lib.load().dut_link_discordance_parse, text)


def _link_options(min_depth=10, min_quality=20, exclude_flags=0, min_base_quality=None, max_dist=1000, max_partners=4, min_link_count=3,
                  max_discordance="0.05", filtered=True):
    if not 0 <= int(min_quality) <= 255:
        raise ValueError("min_quality: 0..255")
    if not 0 <= int(exclude_flags) <= 0xFFFF:
        raise ValueError("exclude_flags: 0..65535")
    if min_base_quality is not None and not 0 <= int(min_base_quality) <= 255:
        raise ValueError("min_base_quality: 0..255")
    for name, v in (("min_depth", min_depth), ("max_dist", max_dist), ("max_partners", max_partners), ("min_link_count", min_link_count)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{name}: 0..2^32-1")
    return _lib.dut_link_options(int(min_depth), int(min_quality), 1 if filtered else 0, int(exclude_flags), 0 if min_base_quality is None else 1,
                                 int(min_base_quality or 0), int(max_dist), int(max_partners), int(min_link_count), link_discordance_parse(str(max_discordance)))


def link_pair_offsets(sites, max_dist: int, max_partners: int) -> np.ndarray:
    """dut_link_pair_offsets: first (n + 1) of the pair set of strictly ascending sites; first[n] is the number of pairs."""
    sites = np.ascontiguousarray(sites, np.uint32).reshape(-1)
    first = np.zeros(sites.shape[0] + 1, np.uint32)
    n_pairs = C.c_uint64()
    st = _lib.load().dut_link_pair_offsets(_ptr(sites) if sites.shape[0] else None, sites.shape[0], int(max_dist), int(max_partners), _ptr(first), C.byref(n_pairs))
    if st != 0:
        raise EngineError(st, "dut_link_pair_offsets refused its arguments")
    return first


def link_measure(rec, contig_len: int, sites, max_dist: int, max_partners: int, min_quality: int, exclude_flags: Optional[int] = None,
                 min_base_quality: Optional[int] = None) -> LinkResult:
    """dut_link_measure: what Engine.site_link_counts returns, from the records on the host (no device needed).
    exclude_flags=None: the unfiltered form; a mask (0 included): the filtered form, with min_base_quality (None: every
    base passes) taken over the records' quality values."""
    sites = np.ascontiguousarray(sites, np.uint32).reshape(-1)
    n = sites.shape[0]
    first = link_pair_offsets(sites, max_dist, max_partners)
    tables = np.zeros((int(first[n]), _lib.CL_LINK_CLASSES, _lib.CL_LINK_CLASSES), np.uint32)
    site_counts = np.zeros((n, _lib.CL_LINK_CLASSES), np.uint32)
    keep = [np.ascontiguousarray(rec.pos, np.int32), np.ascontiguousarray(rec.flag, np.uint16), np.ascontiguousarray(rec.mapq, np.uint8),
            np.ascontiguousarray(rec.cigar_off, np.uint32), np.ascontiguousarray(rec.cigar, np.uint32),
            np.ascontiguousarray(rec.seq_off if rec.seq_off is not None else np.zeros(rec.n + 1, np.uint64), np.uint64),
            np.ascontiguousarray(rec.seq4 if rec.seq4 is not None else np.zeros(0, np.uint8), np.uint8),
            np.ascontiguousarray(rec.qual_off, np.uint64), np.ascontiguousarray(rec.qual, np.uint8)]
    reads = _lib.dut_ep_reads(rec.n, *[a.ctypes.data if a.shape[0] else None for a in keep])
    opt = _link_options(1, min_quality, exclude_flags or 0, min_base_quality if exclude_flags is not None else None, max_dist, max_partners,
                        filtered=exclude_flags is not None)
    st = _lib.load().dut_link_measure(C.byref(reads), int(contig_len), C.byref(opt), _ptr(sites) if n else None, n, _ptr(first),
                                      _ptr(tables) if tables.shape[0] else None, _ptr(site_counts) if n else None)
    if st != 0:
        raise EngineError(st, "dut_link_measure refused its arguments")
    return LinkResult(first=first, tables=tables, site_counts=site_counts)


def link_summarise(site_counts_a, site_counts_b, table, min_depth: int = 10, min_link_count: int = 3, max_discord_per_10k: int = 500) -> dict:
    """dut_link_summarise: one pair from its two sites' counts and its table -- status (LINK_LOW_DEPTH, LINK_CIS, LINK_TRANS,
    LINK_UNRESOLVED), the major and minor class of each site (0..4: A C G T del), depth_a, depth_b, both, MM, Mm, mM, mm, other."""
    a = np.ascontiguousarray(site_counts_a, np.uint32).reshape(-1)
    b = np.ascontiguousarray(site_counts_b, np.uint32).reshape(-1)
    t = np.ascontiguousarray(table, np.uint32).reshape(-1)
    if a.shape[0] != 6 or b.shape[0] != 6 or t.shape[0] != 36:
        raise ValueError("a site has 6 counts and a pair 36 cells")
    for name, v in (("min_depth", min_depth), ("min_link_count", min_link_count), ("max_discord_per_10k", max_discord_per_10k)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{name}: 0..2^32-1")
    prm = _lib.dut_link_params(int(min_depth), int(min_link_count), int(max_discord_per_10k))
    u = _lib.dut_link_summary()
    st = _lib.load().dut_link_summarise(_ptr(a), _ptr(b), _ptr(t), C.byref(prm), C.byref(u))
    if st != 0:
        raise EngineError(st, "invalid parameters")
    return dict(status=int(u.status), major_a=int(u.major_a), minor_a=int(u.minor_a), major_b=int(u.major_b), minor_b=int(u.minor_b),
                depth_a=int(u.depth_a), depth_b=int(u.depth_b), both=int(u.both), MM=int(u.MM), Mm=int(u.Mm), mM=int(u.mM), mm=int(u.mm), other=int(u.other))


def link_sites_parse(path: str, contig: str) -> Tuple[np.ndarray, int]:
    """dut_link_sites_parse: (the 0-based positions of `contig` in the file, sorted, duplicates merged; the lines of other
    contigs).  An EngineError names a malformed line by its number."""
    lib = _lib.load()
    sp = C.POINTER(C.c_uint32)()
    n, skipped = C.c_size_t(), C.c_size_t()
    _call(lib.dut_link_sites_parse, path.encode(), contig.encode(), C.byref(sp), C.byref(n), C.byref(skipped))
    try:
        return np.array(sp[:n.value], np.uint32), int(skipped.value)
    finally:
        lib.dut_link_sites_free(sp)


def write_links(path: str, contig: str, sites, result: LinkResult, sites_skipped: int = 0, max_dist: int = 1000, max_partners: int = 4, min_depth: int = 10,
                min_quality: int = 20, min_link_count: int = 3, max_discordance="0.05", min_base_quality: Optional[int] = None, exclude_flags: int = 0):
    """The TSV of phase-sites (dut_link_write) for 0-based sites and the LinkResult of Engine.site_link_counts or link_measure
    over them under the same max_dist and max_partners.  No device is needed."""
    sites = np.ascontiguousarray(sites, np.uint32).reshape(-1)
    n = sites.shape[0]
    first = np.ascontiguousarray(result.first, np.uint32).reshape(-1)
    tables = np.ascontiguousarray(result.tables, np.uint32)
    site_counts = np.ascontiguousarray(result.site_counts, np.uint32)
    if first.shape[0] != n + 1 or site_counts.shape != (n, 6) or tables.shape != (int(first[n]), 6, 6):
        raise ValueError("the result does not belong to these sites")
    opt = _link_options(min_depth, min_quality, exclude_flags, min_base_quality, max_dist, max_partners, min_link_count, max_discordance)
    _call(_lib.load().dut_link_write, path.encode(), contig.encode(), _ptr(sites) if n else None, n, int(sites_skipped), _ptr(first),
          _ptr(tables) if tables.shape[0] else None, _ptr(site_counts) if n else None, C.byref(opt))


def phase_sites(bam_file: str, reference_file: str, contig: str, sites_file: str, output_file: str, max_dist: int = 1000, max_partners: int = 4,
                min_depth: int = 10, min_quality: int = 20, min_link_count: int = 3, max_discordance="0.05", min_base_quality: Optional[int] = None,
                exclude_flags: int = 0, device_id: int = 0):
    """dut_find_links_files: BAM (+ index), FASTA and a sites file (contig and 1-based position, tab separated; the TSVs of
    find-variants, find-minor-alleles and find-deletions as they are) in, the TSV of linked site pairs out.
    max_discordance: decimal text in [0, 0.4999], at most four decimals."""
    opt = _link_options(min_depth, min_quality, exclude_flags, min_base_quality, max_dist, max_partners, min_link_count, max_discordance)
    _call(_lib.load().dut_find_links_files, bam_file.encode(), reference_file.encode(), contig.encode(), sites_file.encode(), C.byref(opt),
          output_file.encode(), device_id, size=1024)
