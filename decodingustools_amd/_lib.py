"""ctypes binding of libcallable_hip.so (include/callable_loci.h, dut_coverage.h, dut_bam.h, dut_report.h,
dut_haplogroup.h, dut_fingerprint.h, dut_variants.h).

There is no fallback: if the shared library is missing or does not load, importing the engine
raises.  Build it with `python -m decodingustools_amd.build` (or __graft_entry__.build()).
"""
import ctypes as C
import os

from . import build as _build

_LIB = None


class cl_options(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("max_depth", C.c_uint32),
                ("min_mapping_quality", C.c_uint8), ("min_base_quality", C.c_uint8),
                ("min_depth_for_low_mapq", C.c_uint32), ("max_low_mapq", C.c_uint8),
                ("max_low_mapq_fraction", C.c_double)]


class cl_read_tile(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("pos", C.c_void_p), ("mapq", C.c_void_p),
                ("cigar_off", C.c_void_p), ("cigar", C.c_void_p),
                ("qual_off", C.c_void_p), ("qual", C.c_void_p)]


class cl_read_tile_bits(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("pos", C.c_void_p), ("mapq", C.c_void_p),
                ("cigar_off", C.c_void_p), ("cigar", C.c_void_p),
                ("qual_off", C.c_void_p), ("pass_bits", C.c_void_p), ("pass_sum", C.c_void_p)]


class cl_contig_summary(C.Structure):
    _fields_ = [("state_counts", C.c_uint64 * 6), ("n_covered_bases", C.c_uint64),
                ("summed_coverage", C.c_uint64), ("summed_baseq", C.c_uint64),
                ("summed_mapq", C.c_uint64), ("quality_bases", C.c_uint64),
                ("extent", C.c_uint64), ("max_raw_depth", C.c_uint64),
                ("n_intervals", C.c_uint64)]


class cl_interval(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("state", C.c_uint32)]


class cl_layout_info(C.Structure):
    _fields_ = [("form", C.c_int32), ("counter_planes", C.c_uint32), ("n_reads", C.c_uint64), ("n_records", C.c_uint64),
                ("n_windows", C.c_uint64), ("n_qual", C.c_uint64), ("n_cigar", C.c_uint64), ("row_groups", C.c_uint64),
                ("max_groups", C.c_uint64), ("run_table_entries", C.c_uint64), ("device_bytes", C.c_uint64),
                ("upload_h2d_bytes", C.c_uint64), ("tail_wpc", C.c_uint32), ("tail_chunks", C.c_uint32)]


class cl_site_tile(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("pos", C.c_void_p), ("mapq", C.c_void_p),
                ("cigar_off", C.c_void_p), ("cigar", C.c_void_p),
                ("seq_off", C.c_void_p), ("seq4", C.c_void_p)]


class dut_records(C.Structure):
    _fields_ = [("n", C.c_uint64), ("pos", C.c_void_p), ("flag", C.c_void_p), ("mapq", C.c_void_p),
                ("cigar_off", C.c_void_p), ("cigar", C.c_void_p), ("qual_off", C.c_void_p),
                ("qual", C.c_void_p), ("qname_off", C.c_void_p), ("qname", C.c_void_p),
                ("pass_bits", C.c_void_p), ("pass_sum", C.c_void_p)]


class dut_contig_stats(C.Structure):
    _fields_ = [("length", C.c_uint64), ("n_covered_bases", C.c_uint64),
                ("summed_coverage", C.c_uint64), ("summed_baseq", C.c_uint64),
                ("summed_mapq", C.c_uint64), ("quality_bases", C.c_uint64),
                ("n_reads", C.c_uint32), ("reserved", C.c_uint32)]


class dut_contig_derived(C.Structure):
    _fields_ = [("coverage_percent", C.c_double), ("average_depth", C.c_double),
                ("average_mapq", C.c_double), ("average_baseq", C.c_double),
                ("q30_percentage", C.c_double)]


class dut_genome_summary(C.Structure):
    _fields_ = [("total_bases", C.c_uint64), ("callable_bases", C.c_uint64),
                ("callable_percentage", C.c_double), ("average_depth", C.c_double),
                ("average_mapq", C.c_double), ("average_baseq", C.c_double),
                ("q30_percentage", C.c_double), ("total_unique_reads", C.c_uint64),
                ("contigs_analyzed", C.c_uint64)]


class dut_export_meta(C.Structure):
    _fields_ = [("aligner", C.c_char_p), ("reference_build", C.c_char_p),
                ("sequencing_platform", C.c_char_p), ("read_length", C.c_uint64),
                ("bed_file", C.c_char_p), ("summary_html", C.c_char_p),
                ("coverage_plots", C.POINTER(C.c_char_p)), ("n_coverage_plots", C.c_size_t)]


class dut_snp_call(C.Structure):
    _fields_ = [("position", C.c_uint32), ("depth", C.c_uint32), ("freq", C.c_double), ("base", C.c_char)]


class dut_haplogroup_result(C.Structure):
    _fields_ = [("name", C.c_char_p), ("score", C.c_double), ("matching_snps", C.c_uint32),
                ("mismatching_snps", C.c_uint32), ("ancestral_matches", C.c_uint32), ("no_calls", C.c_uint32),
                ("total_snps", C.c_uint32), ("cumulative_snps", C.c_uint32), ("depth", C.c_uint32)]


class dut_fp_options(C.Structure):
    _fields_ = [("ksize", C.c_uint32), ("scaled", C.c_uint64), ("max_frequency", C.c_uint32),
                ("has_max_frequency", C.c_int32)]


class dut_fpc_record(C.Structure):
    _fields_ = [("n_a", C.c_uint64), ("n_b", C.c_uint64), ("n_common", C.c_uint64), ("sum_a", C.c_uint64),
                ("sum_b", C.c_uint64), ("sum_min", C.c_uint64)]


class dut_fpc_sketch(C.Structure):
    _fields_ = [("ksize", C.c_uint32), ("scaled", C.c_uint64), ("n", C.c_uint64), ("hashes", C.c_void_p),
                ("counts", C.c_void_p), ("region", C.c_char * 32), ("max_frequency", C.c_uint32),
                ("has_max_frequency", C.c_int32), ("owner", C.c_void_p)]


class dut_fpc_file_options(C.Structure):
    _fields_ = [("query", C.c_char_p), ("min_jaccard", C.c_double), ("has_min_jaccard", C.c_int32)]


class dut_fp_result(C.Structure):
    _fields_ = [("processed", C.c_uint64), ("n_distinct", C.c_uint64), ("n_entries", C.c_uint64),
                ("hashes", C.c_void_p), ("counts", C.c_void_p), ("hexdigest", C.c_char * 65)]


CL_K_NAMES = ("prep", "bounds", "pileup", "rle")
CL_K_COUNT = 4

class cl_depth_profile(C.Structure):
    _fields_ = [("n_bins", C.c_uint32), ("window", C.c_uint32), ("n_windows", C.c_uint64), ("extent", C.c_uint64),
                ("sum_raw", C.c_uint64), ("sum_qc", C.c_uint64),
                ("hist_raw", C.POINTER(C.c_uint64)), ("hist_qc", C.POINTER(C.c_uint64)),
                ("win_raw", C.POINTER(C.c_uint64)), ("win_qc", C.POINTER(C.c_uint64))]


DEPTH_THRESHOLDS = (1, 5, 10, 15, 20, 30, 50, 100)


class dut_depth_summary(C.Structure):
    _fields_ = [("positions", C.c_uint64), ("mean", C.c_double), ("q1", C.c_uint32), ("median", C.c_uint32), ("q3", C.c_uint32),
                ("q1_saturated", C.c_uint8), ("median_saturated", C.c_uint8), ("q3_saturated", C.c_uint8), ("reserved", C.c_uint8),
                ("frac_at_least", C.c_double * len(DEPTH_THRESHOLDS))]


class dut_depth_options(C.Structure):
    _fields_ = [("n_bins", C.c_uint32), ("window", C.c_uint32), ("dist_path", C.c_char_p), ("windows_path", C.c_char_p),
                ("summary_path", C.c_char_p)]


CL_RUNS_MAX_EDGES = 64
CL_DEPTH_KINDS = {"raw": 0, "qc": 1}


class cl_depth_runs(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("n_edges", C.c_uint32), ("extent", C.c_uint64), ("n_runs", C.c_uint64),
                ("start", C.POINTER(C.c_uint32)), ("value", C.POINTER(C.c_uint32))]


class dut_depth_bed_options(C.Structure):
    _fields_ = [("path", C.c_char_p), ("kind", C.c_uint32), ("edges", C.POINTER(C.c_uint32)), ("n_edges", C.c_uint32)]


CL_TARGET_MAX_THRESHOLDS = 8
CL_TARGETS_MAX = 1 << 24


class cl_target_stats(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("len", C.c_uint32), ("reserved", C.c_uint32),
                ("sum_raw", C.c_uint64), ("sum_qc", C.c_uint64), ("state", C.c_uint32 * 6),
                ("ge_raw", C.c_uint32 * CL_TARGET_MAX_THRESHOLDS), ("ge_qc", C.c_uint32 * CL_TARGET_MAX_THRESHOLDS)]


CL_TARGET_ORDER_MAX_PIECES = 1 << 26
DUT_TARGETS_ORDER = 1


class cl_target_order(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("len", C.c_uint32), ("raw", C.c_uint32 * 5), ("qc", C.c_uint32 * 5)]


class dut_target_options(C.Structure):
    _fields_ = [("bed_path", C.c_char_p), ("out_path", C.c_char_p), ("thresholds", C.POINTER(C.c_uint32)), ("n_thresholds", C.c_uint32)]


CL_GC_BINS = 101
CL_GC_MAX_WINDOW = 1024


class cl_gc_bias(C.Structure):
    _fields_ = [("window", C.c_uint32), ("max_invalid", C.c_uint32), ("extent", C.c_uint32), ("pad_", C.c_uint32),
                ("n_skipped", C.c_uint64), ("positions", C.c_uint64 * CL_GC_BINS), ("sum_raw", C.c_uint64 * CL_GC_BINS),
                ("sum_qc", C.c_uint64 * CL_GC_BINS), ("zero_raw", C.c_uint64 * CL_GC_BINS)]


class dut_gc_stats(C.Structure):
    _fields_ = [("positions", C.c_uint64), ("sum_raw", C.c_uint64), ("sum_qc", C.c_uint64),
                ("total_mean_raw", C.c_double), ("total_mean_qc", C.c_double),
                ("at_dropout_raw", C.c_double), ("gc_dropout_raw", C.c_double), ("at_dropout_qc", C.c_double), ("gc_dropout_qc", C.c_double),
                ("mean_raw", C.c_double * CL_GC_BINS), ("mean_qc", C.c_double * CL_GC_BINS), ("norm_raw", C.c_double * CL_GC_BINS),
                ("norm_qc", C.c_double * CL_GC_BINS), ("zero_frac", C.c_double * CL_GC_BINS)]


class dut_gc_options(C.Structure):
    _fields_ = [("bias_path", C.c_char_p), ("summary_path", C.c_char_p), ("window", C.c_uint32), ("max_invalid", C.c_uint32)]


class cl_scan_candidate(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("ref", C.c_uint8), ("alt", C.c_uint8), ("pad", C.c_uint8 * 2),
                ("a", C.c_uint32), ("c", C.c_uint32), ("g", C.c_uint32), ("t", C.c_uint32), ("depth", C.c_uint32)]


class cl_scan_result(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("n_low_depth", C.c_uint64), ("n_mixed", C.c_uint64),
                ("n_uncomparable", C.c_uint64), ("n_match", C.c_uint64), ("n_variant", C.c_uint64),
                ("candidates", C.POINTER(cl_scan_candidate))]


class cl_site_quals(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("flag", C.c_void_p), ("qual_off", C.c_void_p), ("qual", C.c_void_p),
                ("seq_off", C.c_void_p)]


class cl_scan_filter(C.Structure):
    _fields_ = [("exclude_flags", C.c_uint16), ("use_base_quality", C.c_uint8), ("pad", C.c_uint8)]


class cl_scan_candidate_ex(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("ref", C.c_uint8), ("alt", C.c_uint8), ("pad", C.c_uint8 * 2),
                ("a", C.c_uint32), ("c", C.c_uint32), ("g", C.c_uint32), ("t", C.c_uint32), ("depth", C.c_uint32),
                ("alt_fwd", C.c_uint32), ("alt_rev", C.c_uint32), ("ref_fwd", C.c_uint32), ("ref_rev", C.c_uint32)]


class cl_scan_result_ex(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("n_low_depth", C.c_uint64), ("n_mixed", C.c_uint64),
                ("n_uncomparable", C.c_uint64), ("n_match", C.c_uint64), ("n_variant", C.c_uint64),
                ("candidates", C.POINTER(cl_scan_candidate_ex))]


class cl_minor_params(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_minor_count", C.c_uint32), ("min_minor_per_10k", C.c_uint32)]


class cl_minor_candidate(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("ref", C.c_uint8), ("major", C.c_uint8), ("minor", C.c_uint8), ("pad", C.c_uint8),
                ("a", C.c_uint32), ("c", C.c_uint32), ("g", C.c_uint32), ("t", C.c_uint32), ("depth", C.c_uint32),
                ("major_fwd", C.c_uint32), ("major_rev", C.c_uint32), ("minor_fwd", C.c_uint32), ("minor_rev", C.c_uint32)]


class cl_minor_result(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("n_low_depth", C.c_uint64), ("n_single", C.c_uint64),
                ("n_minor", C.c_uint64), ("candidates", C.POINTER(cl_minor_candidate))]


class dut_minor_options(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_quality", C.c_uint8), ("has_min_base_quality", C.c_int),
                ("min_base_quality", C.c_uint8), ("exclude_flags", C.c_uint16), ("min_minor_per_10k", C.c_uint32),
                ("min_minor_count", C.c_uint32), ("min_minor_per_strand", C.c_uint32)]


class cl_del_params(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_del_count", C.c_uint32), ("min_del_per_10k", C.c_uint32)]


class cl_del_candidate(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("ref", C.c_uint8), ("pad", C.c_uint8 * 3), ("del", C.c_uint32), ("depth", C.c_uint32),
                ("del_fwd", C.c_uint32), ("del_rev", C.c_uint32), ("depth_fwd", C.c_uint32), ("depth_rev", C.c_uint32)]


class cl_del_result(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("n_low_depth", C.c_uint64), ("n_kept", C.c_uint64),
                ("n_deleted", C.c_uint64), ("candidates", C.POINTER(cl_del_candidate))]


class cl_ins_params(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_ins_count", C.c_uint32), ("min_ins_per_10k", C.c_uint32)]


class cl_ins_candidate(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("ref", C.c_uint8), ("pad", C.c_uint8 * 3), ("ins", C.c_uint32), ("depth", C.c_uint32),
                ("ins_fwd", C.c_uint32), ("ins_rev", C.c_uint32), ("depth_fwd", C.c_uint32), ("depth_rev", C.c_uint32)]


class cl_ins_obs(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("len", C.c_uint32), ("key", C.c_uint64 * 2), ("strand", C.c_uint32), ("pad", C.c_uint32)]


class cl_ins_result(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("n_low_depth", C.c_uint64), ("n_kept", C.c_uint64),
                ("n_inserted", C.c_uint64), ("candidates", C.POINTER(cl_ins_candidate)), ("n_obs", C.c_uint64),
                ("obs", C.POINTER(cl_ins_obs))]


class dut_ins_allele(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("len", C.c_uint32), ("key", C.c_uint64 * 2), ("count", C.c_uint32), ("fwd", C.c_uint32),
                ("rev", C.c_uint32), ("pad", C.c_uint32)]


class dut_ins_options(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_quality", C.c_uint8), ("has_min_base_quality", C.c_int),
                ("min_base_quality", C.c_uint8), ("exclude_flags", C.c_uint16), ("min_ins_per_10k", C.c_uint32),
                ("min_ins_count", C.c_uint32), ("min_ins_per_strand", C.c_uint32)]


class dut_del_event(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("length", C.c_uint32), ("q", C.c_uint32), ("del", C.c_uint32),
                ("del_fwd", C.c_uint32), ("del_rev", C.c_uint32), ("max_del", C.c_uint32), ("span", C.c_uint64)]


class dut_del_options(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_quality", C.c_uint8), ("has_min_base_quality", C.c_int),
                ("min_base_quality", C.c_uint8), ("exclude_flags", C.c_uint16), ("min_del_per_10k", C.c_uint32),
                ("min_del_count", C.c_uint32), ("min_del_per_strand", C.c_uint32)]


class cl_cons_params(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_del_count", C.c_uint32), ("min_del_per_10k", C.c_uint32)]


class cl_cons_result(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("n_low_depth", C.c_uint64), ("n_deleted", C.c_uint64), ("n_no_call", C.c_uint64),
                ("n_ref", C.c_uint64), ("n_alt", C.c_uint64), ("cons", C.POINTER(C.c_uint8))]


class dut_cons_change(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("end", C.c_uint32), ("kind", C.c_uint32), ("note", C.c_uint32), ("count", C.c_uint32), ("depth", C.c_uint32),
                ("ref", C.c_char * 68), ("cons", C.c_char * 36)]


class dut_cons_assembly(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("seq_len", C.c_uint64), ("changes", C.POINTER(dut_cons_change)), ("n_changes", C.c_size_t),
                ("n_deletions", C.c_uint64), ("n_insertions", C.c_uint64), ("n_insertions_skipped", C.c_uint64)]


class dut_cons_options(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_quality", C.c_uint8), ("has_min_base_quality", C.c_int), ("min_base_quality", C.c_uint8),
                ("exclude_flags", C.c_uint16), ("min_del_per_10k", C.c_uint32), ("min_del_count", C.c_uint32), ("min_ins_per_10k", C.c_uint32),
                ("min_ins_count", C.c_uint32), ("fill_ref", C.c_int), ("line_width", C.c_uint32)]


class cl_str_locus(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32)]


class cl_str_result(C.Structure):
    _fields_ = [("n_loci", C.c_size_t), ("hist", C.POINTER(C.c_uint32)), ("partial", C.POINTER(C.c_uint32)), ("strands", C.c_uint32)]


class dut_str_params(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_allele_per_10k", C.c_uint32)]


class dut_str_allele_call(C.Structure):
    _fields_ = [("status", C.c_int), ("delta", C.c_int32), ("delta2", C.c_int32), ("count", C.c_uint32), ("fwd", C.c_uint32), ("rev", C.c_uint32),
                ("count2", C.c_uint32), ("n", C.c_uint64), ("other", C.c_uint64)]


class dut_str_locus(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("period", C.c_uint32), ("name", C.c_char * 64)]


class dut_str_options(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_quality", C.c_uint8), ("exclude_flags", C.c_uint16), ("flank", C.c_uint32),
                ("min_allele_per_10k", C.c_uint32)]


class cl_ep_result(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("n_cycles", C.c_uint32), ("pad", C.c_uint32),
                ("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_uncomparable", C.c_uint64), ("n_ins", C.c_uint64), ("ins_bases", C.c_uint64),
                ("n_del", C.c_uint64), ("del_bases", C.c_uint64), ("total", C.c_uint64 * 16),
                ("from5", C.POINTER(C.c_uint64)), ("from3", C.POINTER(C.c_uint64)), ("ins5", C.POINTER(C.c_uint64)), ("ins3", C.POINTER(C.c_uint64)),
                ("del5", C.POINTER(C.c_uint64)), ("del3", C.POINTER(C.c_uint64))]


class dut_ep_reads(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("pos", C.c_void_p), ("flag", C.c_void_p), ("mapq", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p),
                ("seq_off", C.c_void_p), ("seq4", C.c_void_p), ("qual_off", C.c_void_p), ("qual", C.c_void_p)]


class dut_ep_options(C.Structure):
    _fields_ = [("min_quality", C.c_uint8), ("filtered", C.c_int), ("exclude_flags", C.c_uint16), ("has_min_base_quality", C.c_int),
                ("min_base_quality", C.c_uint8), ("n_cycles", C.c_uint32)]


class cl_link_result(C.Structure):
    _fields_ = [("n_sites", C.c_size_t), ("n_pairs", C.c_size_t), ("first", C.POINTER(C.c_uint32)), ("tables", C.POINTER(C.c_uint32)),
                ("site_counts", C.POINTER(C.c_uint32))]


class dut_link_options(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_quality", C.c_uint8), ("filtered", C.c_int), ("exclude_flags", C.c_uint16),
                ("has_min_base_quality", C.c_int), ("min_base_quality", C.c_uint8), ("max_dist", C.c_uint32), ("max_partners", C.c_uint32),
                ("min_link_count", C.c_uint32), ("max_discord_per_10k", C.c_uint32)]


class dut_link_params(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_link_count", C.c_uint32), ("max_discord_per_10k", C.c_uint32)]


class dut_link_summary(C.Structure):
    _fields_ = [("status", C.c_int), ("major_a", C.c_uint8), ("minor_a", C.c_uint8), ("major_b", C.c_uint8), ("minor_b", C.c_uint8),
                ("depth_a", C.c_uint64), ("depth_b", C.c_uint64), ("both", C.c_uint64), ("MM", C.c_uint64), ("Mm", C.c_uint64), ("mM", C.c_uint64),
                ("mm", C.c_uint64), ("other", C.c_uint64)]


class dut_variants_options(C.Structure):
    _fields_ = [("filtered", C.c_int), ("has_min_base_quality", C.c_int), ("min_base_quality", C.c_uint8),
                ("exclude_flags", C.c_uint16), ("min_alt_per_strand", C.c_uint32)]


class dut_variant_note(C.Structure):
    _fields_ = [("known", C.c_int), ("names", C.c_char_p), ("alleles", C.c_char_p)]


class dut_tree_locus(C.Structure):
    _fields_ = [("position", C.c_uint32), ("name", C.c_char_p), ("ancestral", C.c_char_p), ("derived", C.c_char_p)]


CL_SCAN_MAX_DENSE = 1 << 20
CL_STR_BINS, CL_STR_MAX_FLANK, CL_STR_MAX_LOCI, CL_STR_MAX_SPAN = 128, 64, 65536, 1024
DUT_STR_UNITS_LEN = 24
CL_EP_MAX_CYCLES = 256
CL_LINK_CLASSES, CL_LINK_MAX_PARTNERS, CL_LINK_MAX_SITES, CL_LINK_MAX_PAIRS = 6, 15, 1 << 20, 1 << 20

# every symbol the headers declare: (name, restype, argtypes)
SYMBOLS = [
    ("cl_site_scan", C.c_int, [C.c_void_p, C.c_uint8, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                               C.POINTER(cl_scan_result)]),
    ("cl_site_scan_counts", C.c_int, [C.c_void_p, C.c_uint8, C.c_uint32, C.c_uint32, C.c_void_p]),
    ("cl_site_scan_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("cl_site_attach_quals", C.c_int, [C.c_void_p, C.POINTER(cl_site_quals), C.c_uint8]),
    ("cl_site_scan_ex", C.c_int, [C.c_void_p, C.c_uint8, C.c_uint32, C.POINTER(cl_scan_filter), C.c_void_p, C.c_uint64, C.c_uint32,
                                  C.c_uint32, C.POINTER(cl_scan_result_ex)]),
    ("cl_site_scan_counts_ex", C.c_int, [C.c_void_p, C.c_uint8, C.POINTER(cl_scan_filter), C.c_uint32, C.c_uint32, C.c_void_p]),
    ("cl_site_scan_minor", C.c_int, [C.c_void_p, C.c_uint8, C.POINTER(cl_scan_filter), C.POINTER(cl_minor_params), C.c_void_p, C.c_uint64,
                                     C.c_uint32, C.c_uint32, C.POINTER(cl_minor_result)]),
    ("cl_site_scan_dels", C.c_int, [C.c_void_p, C.c_uint8, C.POINTER(cl_scan_filter), C.POINTER(cl_del_params), C.c_void_p, C.c_uint64,
                                    C.c_uint32, C.c_uint32, C.POINTER(cl_del_result)]),
    ("cl_site_scan_ins", C.c_int, [C.c_void_p, C.c_uint8, C.POINTER(cl_scan_filter), C.POINTER(cl_ins_params), C.c_void_p, C.c_uint64,
                                   C.c_uint32, C.c_uint32, C.POINTER(cl_ins_result)]),
    ("cl_site_scan_ins_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("cl_site_scan_consensus", C.c_int, [C.c_void_p, C.c_uint8, C.POINTER(cl_scan_filter), C.POINTER(cl_cons_params), C.c_void_p, C.c_uint64,
                                         C.c_uint32, C.c_uint32, C.POINTER(cl_cons_result)]),
    ("cl_site_str_lengths", C.c_int, [C.c_void_p, C.c_uint8, C.POINTER(cl_scan_filter), C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(cl_str_result)]),
    ("cl_site_error_profile", C.c_int, [C.c_void_p, C.c_uint8, C.POINTER(cl_scan_filter), C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.POINTER(cl_ep_result)]),
    ("cl_site_error_profile_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("cl_site_link_counts", C.c_int, [C.c_void_p, C.c_uint8, C.POINTER(cl_scan_filter), C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                      C.POINTER(cl_link_result)]),
    ("cl_debug_site_pass_bits", C.c_int, [C.POINTER(cl_site_quals), C.c_uint8, C.c_void_p, C.c_uint64]),
    # include/dut_variants.h
    ("dut_variants_annotate_ex", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.POINTER(dut_variant_note))]),
    ("dut_variants_write_ex", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(cl_scan_result_ex), C.c_uint32, C.c_uint8,
                                        C.POINTER(dut_variants_options), C.POINTER(dut_variant_note), C.c_char_p, C.c_size_t]),
    ("dut_find_variants_files_ex", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p,
                                             C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_uint8, C.POINTER(dut_variants_options),
                                             C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_minor_fraction_parse", C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    ("dut_minor_classify_counts", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(cl_minor_params),
                                            C.c_char_p, C.c_char_p]),
    ("dut_minor_write", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(cl_minor_result), C.POINTER(dut_minor_options), C.c_char_p, C.c_size_t]),
    ("dut_find_minor_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(dut_minor_options),
                                       C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_del_fraction_parse", C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    ("dut_del_classify_counts", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(cl_del_params)]),
    ("dut_del_events", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(dut_del_event)), C.POINTER(C.c_size_t)]),
    ("dut_del_events_free", None, [C.POINTER(dut_del_event)]),
    ("dut_del_write", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(cl_del_result), C.POINTER(dut_del_options), C.c_char_p, C.c_size_t]),
    ("dut_find_deletions_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(dut_del_options),
                                           C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_ins_classify_counts", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(cl_ins_params)]),
    ("dut_ins_alleles", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(dut_ins_allele)), C.POINTER(C.c_size_t)]),
    ("dut_ins_alleles_free", None, [C.POINTER(dut_ins_allele)]),
    ("dut_ins_write", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(cl_ins_result), C.POINTER(dut_ins_options), C.c_char_p, C.c_size_t]),
    ("dut_find_insertions_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(dut_ins_options),
                                            C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_cons_classify_counts", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(cl_cons_params),
                                           C.c_uint8, C.c_char_p]),
    ("dut_cons_assemble", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(cl_ins_result), C.c_void_p, C.c_size_t,
                                    C.POINTER(cl_ins_params), C.c_int, C.POINTER(dut_cons_assembly)]),
    ("dut_cons_assembly_free", None, [C.POINTER(dut_cons_assembly)]),
    ("dut_cons_write_fasta", C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint32, C.c_char_p,
                                       C.c_size_t]),
    ("dut_cons_write_changes", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(cl_cons_result), C.POINTER(dut_cons_assembly), C.POINTER(dut_cons_options),
                                         C.c_char_p, C.c_size_t]),
    ("dut_find_consensus_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(dut_cons_options),
                                           C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_str_measure", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint8, C.c_uint16, C.c_uint32,
                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("dut_str_call", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(dut_str_params), C.POINTER(dut_str_allele_call)]),
    ("dut_str_units", C.c_int, [C.c_uint32, C.c_int32, C.c_uint32, C.c_char_p]),
    ("dut_str_loci_parse", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(dut_str_locus)), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                     C.c_char_p, C.c_size_t]),
    ("dut_str_loci_free", None, [C.POINTER(dut_str_locus)]),
    ("dut_str_write", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(dut_str_locus), C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32,
                                C.POINTER(dut_str_options), C.c_char_p, C.c_size_t]),
    ("dut_find_strs_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(dut_str_options), C.c_char_p, C.c_int, C.c_char_p,
                                      C.c_size_t]),
    ("dut_error_profile_measure", C.c_int, [C.POINTER(dut_ep_reads), C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(dut_ep_options),
                                            C.c_void_p, C.POINTER(cl_ep_result)]),
    ("dut_error_profile_write", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(cl_ep_result), C.POINTER(dut_ep_options), C.c_char_p, C.c_size_t]),
    ("dut_error_profile_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(dut_ep_options), C.c_char_p,
                                          C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_link_pair_offsets", C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    ("dut_link_measure", C.c_int, [C.POINTER(dut_ep_reads), C.c_uint32, C.POINTER(dut_link_options), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    ("dut_link_summarise", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(dut_link_params), C.POINTER(dut_link_summary)]),
    ("dut_link_discordance_parse", C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    ("dut_link_sites_parse", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                       C.c_char_p, C.c_size_t]),
    ("dut_link_sites_free", None, [C.POINTER(C.c_uint32)]),
    ("dut_link_write", C.c_int, [C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(dut_link_options), C.c_char_p, C.c_size_t]),
    ("dut_find_links_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(dut_link_options), C.c_char_p, C.c_int, C.c_char_p,
                                       C.c_size_t]),
    ("dut_scan_classify", C.c_int, [C.c_void_p, C.c_uint8, C.c_uint32, C.c_char_p]),
    ("dut_scan_classify_counts", C.c_int, [C.c_void_p, C.c_uint8, C.c_uint32, C.c_char_p]),
    ("dut_variants_annotate", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t,
                                        C.POINTER(C.POINTER(dut_variant_note))]),
    ("dut_variants_free_notes", None, [C.POINTER(dut_variant_note), C.c_size_t]),
    ("dut_variants_write", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(cl_scan_result), C.c_uint32, C.c_uint8,
                                     C.POINTER(dut_variant_note), C.c_char_p, C.c_size_t]),
    ("dut_find_variants_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p,
                                          C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_uint8, C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_tree_collect_loci", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(dut_tree_locus)),
                                        C.POINTER(C.c_size_t)]),
    ("cl_contig_depth_profile", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(cl_depth_profile)]),
    ("cl_contig_depth_profile_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("dut_depth_stats", C.c_int, [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.POINTER(dut_depth_summary)]),
    ("dut_depth_acc_new", C.c_void_p, [C.c_uint32, C.c_uint32, C.c_char_p]),
    ("dut_depth_acc_free", None, [C.c_void_p]),
    ("dut_depth_acc_add", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(cl_depth_profile)]),
    ("dut_depth_acc_total", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint64)),
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("dut_depth_acc_finish", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    ("dut_coverage_files_ex", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                        C.POINTER(cl_options), C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(C.c_int), C.c_size_t,
                                        C.c_uint, C.POINTER(dut_depth_options), C.c_char_p, C.c_size_t]),
    ("cl_contig_depth_runs", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(cl_depth_runs)]),
    ("cl_contig_depth_runs_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("dut_quantize_parse", C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    ("dut_depth_bed_write", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(cl_depth_runs), C.POINTER(C.c_uint32)]),
    ("dut_coverage_files_ex2", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                         C.POINTER(cl_options), C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(C.c_int), C.c_size_t,
                                         C.c_uint, C.POINTER(dut_depth_options), C.POINTER(dut_depth_bed_options), C.c_char_p,
                                         C.c_size_t]),
    ("cl_contig_targets", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32),
                                    C.c_uint32, C.POINTER(C.POINTER(cl_target_stats))]),
    ("cl_contig_targets_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("dut_targets_parse", C.c_void_p, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    ("dut_targets_read", C.c_void_p, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("dut_targets_free", None, [C.c_void_p]),
    ("dut_targets_n_contigs", C.c_size_t, [C.c_void_p]),
    ("dut_targets_contig", C.c_char_p, [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("dut_targets_get", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint32)),
                                  C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_uint32))]),
    ("dut_thresholds_parse", C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    ("dut_targets_write_header", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]),
    ("dut_targets_write", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(cl_target_stats), C.POINTER(C.c_char_p), C.c_size_t,
                                    C.c_uint32, C.c_void_p]),
    ("dut_targets_write_total", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("dut_coverage_files_ex3", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                         C.POINTER(cl_options), C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(C.c_int), C.c_size_t,
                                         C.c_uint, C.POINTER(dut_depth_options), C.POINTER(dut_depth_bed_options),
                                         C.POINTER(dut_target_options), C.c_char_p, C.c_size_t]),
    ("cl_contig_target_order", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t,
                                         C.POINTER(C.POINTER(cl_target_order))]),
    ("cl_contig_target_order_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    ("dut_targets_write_header_ex", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_int]),
    ("dut_targets_write_ex", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(cl_target_stats), C.POINTER(cl_target_order),
                                       C.POINTER(C.c_char_p), C.c_size_t, C.c_uint32, C.c_void_p]),
    ("dut_targets_write_total_ex", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]),
    ("dut_coverage_files_ex4", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                         C.POINTER(cl_options), C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(C.c_int), C.c_size_t,
                                         C.c_uint, C.POINTER(dut_depth_options), C.POINTER(dut_depth_bed_options),
                                         C.POINTER(dut_target_options), C.c_uint, C.c_char_p, C.c_size_t]),
    ("dut_coverage_files_ex5", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                         C.POINTER(cl_options), C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(C.c_int), C.c_size_t,
                                         C.c_uint, C.POINTER(dut_depth_options), C.POINTER(dut_depth_bed_options),
                                         C.POINTER(dut_target_options), C.c_uint, C.POINTER(dut_gc_options), C.c_char_p, C.c_size_t]),
    ("cl_contig_gc_bias", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(cl_gc_bias)]),
    ("cl_contig_gc_bias_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("cl_debug_gc_bits", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    ("dut_gc_bias_add", C.c_int, [C.POINTER(cl_gc_bias), C.POINTER(cl_gc_bias)]),
    ("dut_gc_bias_stats", C.c_int, [C.POINTER(cl_gc_bias), C.POINTER(dut_gc_stats)]),
    ("dut_gc_bias_write_header", C.c_int, [C.c_void_p]),
    ("dut_gc_bias_write", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(cl_gc_bias)]),
    ("dut_gc_summary_write_header", C.c_int, [C.c_void_p]),
    ("dut_gc_summary_write", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(cl_gc_bias)]),
    ("cl_abi_version", C.c_int, []),
    ("cl_device_count", C.c_int, []),
    ("cl_create", C.c_int, [C.POINTER(cl_options), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("cl_destroy", None, [C.c_void_p]),
    ("cl_last_error", C.c_char_p, [C.c_void_p]),
    ("cl_contig_begin", C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_uint64]),
    ("cl_contig_reserve", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]),
    ("cl_contig_prefetch_qual", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    ("cl_push_reads", C.c_int, [C.c_void_p, C.POINTER(cl_read_tile)]),
    ("cl_push_reads_bits", C.c_int, [C.c_void_p, C.POINTER(cl_read_tile_bits)]),
    ("cl_contig_finish", C.c_int, [C.c_void_p, C.POINTER(cl_contig_summary),
                                   C.POINTER(C.POINTER(cl_interval)), C.POINTER(C.c_size_t)]),
    ("cl_contig_abort", C.c_int, [C.c_void_p]),
    ("cl_contig_upload", C.c_int, [C.c_void_p]),
    ("cl_contig_run", C.c_int, [C.c_void_p]),
    ("cl_contig_collect", C.c_int, [C.c_void_p, C.POINTER(cl_contig_summary),
                                    C.POINTER(C.POINTER(cl_interval)), C.POINTER(C.c_size_t)]),
    ("cl_sync", C.c_int, [C.c_void_p]),
    ("cl_device_summary", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("cl_set_profiling", C.c_int, [C.c_void_p, C.c_int]),
    ("cl_get_kernel_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("cl_reset_kernel_ms", C.c_int, [C.c_void_p]),
    ("cl_contig_bytes", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("cl_contig_layout", C.c_int, [C.c_void_p, C.POINTER(cl_layout_info)]),
    ("cl_debug_ref_n_bits", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]),
    ("cl_debug_qual_pack", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint8, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]),
    ("cl_debug_host_create", C.c_int, [C.POINTER(cl_options), C.POINTER(C.c_void_p)]),
    ("cl_debug_pass_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("cl_debug_pass_rows_segments", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    ("cl_debug_depths", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("cl_debug_read_records", C.c_int, [C.c_int32, C.c_void_p, C.c_uint32, C.c_uint8, C.c_uint8, C.c_uint64, C.c_uint64,
                                        C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("cl_site_pileup", C.c_int, [C.c_void_p, C.c_uint8, C.c_uint32, C.c_uint64, C.POINTER(cl_site_tile),
                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    ("cl_site_upload", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(cl_site_tile)]),
    ("cl_site_run", C.c_int, [C.c_void_p, C.c_uint8, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("cl_site_pileup_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("dut_profiler_new", C.c_void_p, [C.c_char_p]),
    ("dut_profiler_free", None, [C.c_void_p]),
    ("dut_profiler_enable_plots", None, [C.c_void_p, C.c_uint32]),
    ("dut_profiler_plot_bins", C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("dut_profiler_finish_plot", C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32]),
    ("dut_profiler_contig_counts", None, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]),
    ("dut_profiler_feed_contig", C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_uint64)]),
    ("dut_admit_reads", C.c_int, [C.POINTER(cl_options), C.c_int32, C.c_uint32, C.POINTER(dut_records),
                                  C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("dut_process_single_contig", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(dut_contig_stats),
                                            C.POINTER(cl_options), C.c_char_p, C.c_int32, C.c_uint32,
                                            C.c_void_p, C.c_uint64, C.POINTER(dut_records)]),
    ("dut_process_single_contig_runs", C.c_int, [C.c_void_p, C.POINTER(dut_contig_stats), C.POINTER(cl_options), C.c_int32,
                                                 C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(dut_records),
                                                 C.POINTER(C.c_uint64), C.POINTER(C.POINTER(cl_interval)),
                                                 C.POINTER(C.c_size_t)]),
    ("dut_contig_derive", None, [C.POINTER(dut_contig_stats), C.POINTER(dut_contig_derived)]),
    ("dut_compare_contig_names", C.c_int, [C.c_char_p, C.c_char_p]),
    ("dut_genome_summary_build", None, [C.POINTER(dut_contig_stats), C.POINTER(C.c_uint64), C.c_size_t,
                                        C.POINTER(dut_genome_summary)]),
    ("dut_state_name", C.c_char_p, [C.c_uint32]),
    ("dut_bam_open", C.c_void_p, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("dut_bam_close", None, [C.c_void_p]),
    ("dut_bam_error", C.c_char_p, [C.c_void_p]),
    ("dut_bam_n_ref", C.c_int, [C.c_void_p]),
    ("dut_bam_ref_name", C.c_char_p, [C.c_void_p, C.c_int]),
    ("dut_bam_ref_len", C.c_uint32, [C.c_void_p, C.c_int]),
    ("dut_bam_header_text", C.c_void_p, [C.c_void_p, C.POINTER(C.c_size_t)]),
    ("dut_bam_has_index", C.c_int, [C.c_void_p]),
    ("dut_bam_ref_mapped", C.c_int64, [C.c_void_p, C.c_int]),
    ("dut_bam_read_contig", C.c_int, [C.c_void_p, C.c_int, C.POINTER(dut_records), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p)]),
    ("dut_bam_read_contig_bits", C.c_int, [C.c_void_p, C.c_int, C.c_uint8, C.POINTER(dut_records)]),
    ("dut_fasta_open", C.c_void_p, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("dut_fasta_close", None, [C.c_void_p]),
    ("dut_fasta_fetch", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    ("dut_fasta_error", C.c_char_p, [C.c_void_p]),
    ("dut_coverage_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                     C.POINTER(cl_options), C.POINTER(C.c_char_p), C.c_size_t, C.c_int,
                                     C.c_char_p, C.c_size_t]),
    ("dut_coverage_files_multi", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                           C.POINTER(cl_options), C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(C.c_int), C.c_size_t,
                                           C.c_uint, C.c_char_p, C.c_size_t]),
    ("dut_bam_sample", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("dut_bam_next_seqs", C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_void_p)]),
    # include/dut_fingerprint.h
    ("dut_fp_create", C.c_int, [C.POINTER(dut_fp_options), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("dut_fp_push_seq4", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("dut_fp_push_bytes", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("dut_fp_finish", C.c_int, [C.c_void_p, C.POINTER(dut_fp_result)]),
    ("dut_fp_destroy", None, [C.c_void_p]),
    ("dut_fp_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("dut_fp_last_error", C.c_char_p, [C.c_void_p]),
    ("dut_fp_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(dut_fp_options), C.c_char_p, C.c_int,
                               C.c_char_p, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    ("dut_fp_input_kind", C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("dut_fp_kmer_hashes_host", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("dut_fp_kmer_hashes_host_seq4", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("dut_fp_max_hash", C.c_uint64, [C.c_uint64]),
    ("dut_fp_sha256", None, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("dut_fpc_create", C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("dut_fpc_destroy", None, [C.c_void_p]),
    ("dut_fpc_last_error", C.c_char_p, [C.c_void_p]),
    ("dut_fpc_add", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]),
    ("dut_fpc_compare", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("dut_fpc_compare_all", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    ("dut_fpc_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("dut_fpc_tile", C.c_uint32, []),
    ("dut_fpc_compare_host", C.c_int, [C.POINTER(dut_fpc_sketch), C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                       C.c_char_p, C.c_size_t]),
    ("dut_fp_file_read", C.c_int, [C.c_char_p, C.POINTER(dut_fpc_sketch), C.c_char_p, C.c_size_t]),
    ("dut_fp_file_free", None, [C.POINTER(dut_fpc_sketch)]),
    ("dut_fpc_write", C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_uint64, C.c_double, C.c_int]),
    ("dut_fpc_write_matrix", C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_void_p, C.c_uint64, C.c_void_p]),
    ("dut_fingerprint_compare_files", C.c_int, [C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(dut_fpc_file_options), C.c_char_p,
                                                C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_fastq_open", C.c_void_p, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("dut_fastq_next", C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_void_p)]),
    ("dut_fastq_close", None, [C.c_void_p]),
    # include/dut_report.h
    ("dut_detect_aligner", C.c_char_p, [C.c_char_p, C.c_size_t]),
    ("dut_reference_build", C.c_char_p, [C.c_char_p, C.c_size_t]),
    ("dut_detect_platform_from_qname", C.c_int, [C.c_char_p, C.c_size_t]),
    ("dut_parse_read_name", C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("dut_infer_specific_platform", C.c_char_p, [C.c_int, C.c_char_p]),
    ("dut_bam_stats_new", C.c_void_p, [C.c_size_t]),
    ("dut_bam_stats_free", None, [C.c_void_p]),
    ("dut_bam_stats_set_header", None, [C.c_void_p, C.c_char_p, C.c_size_t]),
    ("dut_bam_stats_add", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint16, C.c_uint32, C.c_char_p, C.c_size_t,
                                    C.c_int32]),
    ("dut_bam_stats_collect", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    ("dut_bam_stats_aligner", C.c_char_p, [C.c_void_p]),
    ("dut_bam_stats_reference_build", C.c_char_p, [C.c_void_p]),
    ("dut_bam_stats_infer_platform", C.c_char_p, [C.c_void_p]),
    ("dut_bam_stats_primary_platform", C.c_int, [C.c_void_p]),
    ("dut_bam_stats_read_count", C.c_uint64, [C.c_void_p]),
    ("dut_bam_stats_average_read_length", C.c_uint64, [C.c_void_p]),
    ("dut_bam_stats_modal_read_length", C.c_uint64, [C.c_void_p]),
    ("dut_bam_stats_get", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]),
    ("dut_format_f64", C.c_size_t, [C.c_double, C.c_char_p]),
    ("dut_coverage_output_json", C.c_int, [C.POINTER(dut_contig_stats), C.POINTER(C.c_char_p),
                                           C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(dut_export_meta),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("dut_free", None, [C.c_void_p]),
    ("dut_write_html_report", C.c_int, [C.POINTER(dut_contig_stats), C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_size_t,
                                        C.POINTER(dut_export_meta), C.c_uint64, C.c_char_p]),
    # include/dut_haplogroup.h
    ("dut_tree_parse", C.c_void_p, [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_tree_load", C.c_void_p, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_tree_free", None, [C.c_void_p]),
    ("dut_tree_total_nodes", C.c_size_t, [C.c_void_p]),
    ("dut_tree_built_nodes", C.c_size_t, [C.c_void_p]),
    ("dut_tree_root_name", C.c_char_p, [C.c_void_p]),
    ("dut_tree_collect_sites", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("dut_call_sites", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("dut_tree_score", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
    ("dut_write_haplogroup_report", C.c_int, [C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_size_t, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]),
    ("dut_validate_reference", C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p), C.c_size_t, C.c_int,
                                         C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    ("dut_find_branch_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint8,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
]


def lib_path():
    # DUT_CALLABLE_LIB: tooling override to time a differently built variant of the same library
    return os.environ.get("DUT_CALLABLE_LIB") or _build.LIB


def load():
    """Load the shared library; raises if it is absent (no CPU fallback exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # PyTorch ships its own HIP runtime; whichever of two runtimes initialises second in a process finds
    # no device.  With torch imported first this library resolves against torch's runtime and both work,
    # in either order of use -- so import it here when it is installed (DUT_NO_TORCH_PRELOAD=1 skips this).
    import sys
    if "torch" not in sys.modules and os.environ.get("DUT_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -m decodingustools_amd.build` "
            "(needs hipcc). The engine has no CPU fallback.")
    lib = C.CDLL(path)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.cl_abi_version() != 1:
        raise RuntimeError("libcallable_hip.so ABI version mismatch")
    _LIB = lib
    return lib
