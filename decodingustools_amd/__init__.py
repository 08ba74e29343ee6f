"""decodingustools_amd -- MI355X-native callable-loci (`coverage`) hot path of DecodingUsTools.

Only what the path needs: csrc/ (HIP kernels + C ABI + C++ host mirror), a ctypes binding and
the host-side mirror of the reference's callable_loci module API.
"""
from .records import ContigRecords  # noqa: F401
from .callable_loci import (CallableOptions, CalledState, CallableProfiler, ContigProfiler,  # noqa: F401
                            ContigResult, ConsResult, DelResult, ErrorProfile, InsResult, LinkResult, StrResult, DepthAccumulator, DepthProfile, DepthRuns, Engine, EngineError, ScanResult,
                            admit_reads, compare_contig_names, depth_stats, genome_summary, process_single_contig,
                            quantize_parse, write_depth_bed, TargetStats, TargetOrder, parse_targets, thresholds_parse, write_target_stats,
                            GcBias, gc_bias_stats, write_gc_bias, write_gc_summary)
from .fingerprint import (Fingerprint, FingerprintError, FingerprintResult, fingerprint_file,  # noqa: F401
                          CompareResult, SketchFile, SketchSet, compare_files, compare_host, read_fingerprint_file)
from .variants import (annotate_variants, error_profile, error_profile_measure, write_error_profile, cons_assemble, cons_classify_counts, consensus, del_classify_counts, del_events, del_fraction_parse, find_deletions,  # noqa: F401
                       find_insertions, find_strs, find_variants, ins_alleles, ins_classify_counts, scan_classify, scan_classify_counts, str_call, str_loci_parse, str_measure, str_units,
                       write_consensus, write_consensus_changes, write_deletions, write_insertions, write_strs, write_variants,
                       link_measure, link_pair_offsets, link_sites_parse, link_summarise, phase_sites, write_links)

__all__ = ["ContigRecords", "CallableOptions", "CalledState", "CallableProfiler", "ContigProfiler",
           "ContigResult", "DepthAccumulator", "DepthProfile", "DepthRuns", "Engine", "EngineError", "admit_reads",
           "compare_contig_names", "depth_stats", "genome_summary", "process_single_contig", "Fingerprint", "FingerprintError", "FingerprintResult",
           "fingerprint_file", "ScanResult", "annotate_variants", "find_variants", "scan_classify", "scan_classify_counts",
           "write_variants", "quantize_parse", "write_depth_bed", "TargetStats", "TargetOrder", "parse_targets", "thresholds_parse", "write_target_stats", "DelResult", "find_deletions", "del_events", "write_deletions",
           "del_fraction_parse", "del_classify_counts", "InsResult", "find_insertions", "ins_alleles", "write_insertions",
           "ins_classify_counts", "ConsResult", "consensus", "cons_assemble", "cons_classify_counts", "write_consensus",
           "write_consensus_changes", "StrResult", "find_strs", "str_measure", "str_call", "str_units", "str_loci_parse", "write_strs",
           "ErrorProfile", "error_profile", "error_profile_measure", "write_error_profile",
           "CompareResult", "SketchFile", "SketchSet", "compare_files", "compare_host", "read_fingerprint_file",
           "LinkResult", "phase_sites", "link_measure", "link_pair_offsets", "link_summarise", "link_sites_parse", "write_links",
           "GcBias", "gc_bias_stats", "write_gc_bias", "write_gc_summary"]
