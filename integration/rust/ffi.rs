//! src/callable_loci/ffi.rs -- one declaration per symbol of include/callable_loci.h that the
//! coverage path uses.  Not compiled in this repository (no Rust toolchain in the image).
use std::os::raw::{c_char, c_int, c_uint, c_void};

#[repr(C)]
pub struct ClOptions {            // CallableOptions, options.rs:2-9
    pub min_depth: u32, pub max_depth: u32,
    pub min_mapping_quality: u8, pub min_base_quality: u8,
    pub min_depth_for_low_mapq: u32, pub max_low_mapq: u8,
    pub max_low_mapq_fraction: f64,
}
#[repr(C)]
pub struct ClReadTile {
    pub n_reads: u64,
    pub pos: *const i32, pub mapq: *const u8,
    pub cigar_off: *const u32, pub cigar: *const u32,
    pub qual_off: *const u64, pub qual: *const u8,
}
#[repr(C)]
pub struct ClReadTileBits {       // cl_read_tile_bits: the packed pass-bitmask variant
    pub n_reads: u64,
    pub pos: *const i32, pub mapq: *const u8,
    pub cigar_off: *const u32, pub cigar: *const u32,
    pub qual_off: *const u64,     // bit offsets into pass_bits
    pub pass_bits: *const u64,    // bit g = quality value g >= min_base_quality (mod.rs:33)
    pub pass_sum: *const u32,     // per read: sum of the passing values over its M/=/X bases (contig_profiler.rs:65-70)
}
#[repr(C)] #[derive(Default)]
pub struct ClContigSummary {
    pub state_counts: [u64; 6],   // indexed by CalledState as usize (types.rs:36-43)
    pub n_covered_bases: u64, pub summed_coverage: u64, pub summed_baseq: u64,
    pub summed_mapq: u64, pub quality_bases: u64,
    pub extent: u64, pub max_raw_depth: u64, pub n_intervals: u64,
}
#[repr(C)] pub struct ClInterval { pub start: u32, pub end: u32, pub state: u32 }
pub enum ClCtx {}

extern "C" {
    pub fn cl_create(opt: *const ClOptions, device_id: c_int, stream: *mut c_void, out: *mut *mut ClCtx) -> c_int;
    pub fn cl_destroy(ctx: *mut ClCtx);
    pub fn cl_last_error(ctx: *const ClCtx) -> *const c_char;
    pub fn cl_contig_begin(ctx: *mut ClCtx, tid: i32, contig_len: u32, ref_bases: *const u8, ref_len: u64) -> c_int;
    pub fn cl_contig_reserve(ctx: *mut ClCtx, n_reads: u64, n_cigar_ops: u64, n_qual_bytes: u64) -> c_int; // optional hint
    pub fn cl_contig_prefetch_qual(ctx: *mut ClCtx, qual: *const u8, n_bytes: u64) -> c_int;             // optional overlap
    pub fn cl_push_reads(ctx: *mut ClCtx, tile: *const ClReadTile) -> c_int;
    pub fn cl_push_reads_bits(ctx: *mut ClCtx, tile: *const ClReadTileBits) -> c_int;                     // optional: the test taken by the caller
    pub fn cl_contig_finish(ctx: *mut ClCtx, out: *mut ClContigSummary,
                            iv: *mut *const ClInterval, n_iv: *mut usize) -> c_int;
    pub fn cl_contig_abort(ctx: *mut ClCtx) -> c_int;      // error path: cancels an unclaimed prefetch, drops staged reads
    pub fn cl_contig_layout(ctx: *mut ClCtx, out: *mut ClLayoutInfo) -> c_int;   // what is resident: form, rows, HBM held
    // include/dut_bam.h: files in, files out, over one or several devices of a node (no collective: one process)
    pub fn dut_coverage_files_multi(bam: *const c_char, fasta: *const c_char, bed: *const c_char,
                                    summary_json: *const c_char, summary_html: *const c_char, opt: *const ClOptions,
                                    contigs: *const *const c_char, n_contigs: usize, devices: *const c_int, n_devices: usize,
                                    flags: c_uint, err: *mut c_char, err_len: usize) -> c_int;
    // the depth distribution of the resident contig (after cl_contig_finish / cl_contig_run), reduced on the device
    pub fn cl_contig_depth_profile(ctx: *mut ClCtx, n_bins: u32, window: u32, out: *mut ClDepthProfile) -> c_int;
    pub fn cl_contig_depth_profile_ms(ctx: *mut ClCtx, kernel_ms: *mut f64) -> c_int;   // measurement: its kernel by events
    // include/dut_coverage.h: statistics of a histogram, the accumulator and its writers (host only)
    pub fn dut_depth_stats(hist: *const u64, n_bins: u32, sum: u64, out: *mut DutDepthSummary) -> c_int;
    pub fn dut_depth_acc_new(n_bins: u32, window: u32, windows_path: *const c_char) -> *mut DutDepthAcc;
    pub fn dut_depth_acc_add(acc: *mut DutDepthAcc, contig: *const c_char, p: *const ClDepthProfile) -> c_int;
    pub fn dut_depth_acc_total(acc: *const DutDepthAcc, hist_raw: *mut *const u64, hist_qc: *mut *const u64,
                               sum_raw: *mut u64, sum_qc: *mut u64) -> c_int;
    pub fn dut_depth_acc_finish(acc: *mut DutDepthAcc, dist_path: *const c_char, summary_path: *const c_char) -> c_int;
    pub fn dut_depth_acc_free(acc: *mut DutDepthAcc);
    // include/dut_bam.h: dut_coverage_files_multi + the depth profile files (depth NULL: exactly that call)
    pub fn dut_coverage_files_ex(bam: *const c_char, fasta: *const c_char, bed: *const c_char,
                                 summary_json: *const c_char, summary_html: *const c_char, opt: *const ClOptions,
                                 contigs: *const *const c_char, n_contigs: usize, devices: *const c_int, n_devices: usize,
                                 flags: c_uint, depth: *const DutDepthOptions, err: *mut c_char, err_len: usize) -> c_int;
    // per-base depth as runs of equal value (README "Per-base depth"); kind 0 raw, 1 qc; edges null with n_edges 0: exact depth
    pub fn cl_contig_depth_runs(ctx: *mut ClCtx, kind: u32, edges: *const u32, n_edges: u32, out: *mut ClDepthRuns) -> c_int;
    pub fn cl_contig_depth_runs_ms(ctx: *mut ClCtx, kernel_ms: *mut f64) -> c_int;
    pub fn dut_quantize_parse(spec: *const c_char, edges: *mut u32, n_edges: *mut u32, err: *mut c_char, err_len: usize) -> c_int; // edges: room for 64
    pub fn dut_coverage_files_ex2(bam: *const c_char, fasta: *const c_char, bed: *const c_char,
                                  summary_json: *const c_char, summary_html: *const c_char, opt: *const ClOptions,
                                  contigs: *const *const c_char, n_contigs: usize, devices: *const c_int, n_devices: usize,
                                  flags: c_uint, depth: *const DutDepthOptions, depth_bed: *const DutDepthBedOptions,
                                  err: *mut c_char, err_len: usize) -> c_int;
    // the dense form of the site pileup: base counts and SNV calls at every position of a range of the tile
    // cl_site_upload left resident (README "Variant scan"); candidates are context-owned until the next scan / upload
    pub fn cl_site_scan(ctx: *mut ClCtx, min_quality: u8, min_depth: u32, ref_bases: *const u8, ref_len: u64,
                        start: u32, end: u32, out: *mut ClScanResult) -> c_int;
    pub fn cl_site_scan_counts(ctx: *mut ClCtx, min_quality: u8, start: u32, end: u32, counts: *mut u32) -> c_int; // (end - start) * 5, at most 1 << 20 positions
    pub fn cl_site_scan_stats(ctx: *mut ClCtx, kernel_ms: *mut f64, bytes: *mut u64) -> c_int;
    // include/dut_variants.h: classification on the host (f64 rule), annotation against a tree, the TSV, `find-variants` on files
    pub fn dut_scan_classify(hist16: *const u32, ref_byte: u8, min_depth: u32, called: *mut c_char) -> c_int;
    pub fn dut_scan_classify_counts(counts5: *const u32, ref_byte: u8, min_depth: u32, called: *mut c_char) -> c_int;
    pub fn dut_variants_annotate(tree: *const DutTree, build_id: *const c_char, chromosome: *const c_char,
                                 candidates: *const ClScanCandidate, n: usize, notes: *mut *mut DutVariantNote) -> c_int;
    pub fn dut_variants_free_notes(notes: *mut DutVariantNote, n: usize);
    pub fn dut_variants_write(path: *const c_char, contig: *const c_char, res: *const ClScanResult, min_depth: u32,
                              min_quality: u8, notes: *const DutVariantNote, err: *mut c_char, err_len: usize) -> c_int;
    pub fn dut_find_variants_files(bam: *const c_char, fasta: *const c_char, contig: *const c_char, has_region: c_int,
                                   start: u32, end: u32, tree_json: *const c_char, provider: c_int, tree_type: c_int,
                                   output: *const c_char, min_depth: u32, min_quality: u8, device_id: c_int,
                                   err: *mut c_char, err_len: usize) -> c_int;
    // short tandem repeats (README "Short tandem repeats"): per locus [start, end) the histogram of the spanning reads' deltas
    // and the partial reads, over the tile cl_site_upload left resident; filter null: one strand.  Context-owned arrays,
    // valid until the next cl_site_str_lengths / upload.  flank 1..64, at most 65536 loci of at most 1024 positions
    pub fn cl_site_str_lengths(ctx: *mut ClCtx, min_quality: u8, filter: *const ClScanFilter, flank: u32, loci: *const ClStrLocus,
                               n_loci: usize, out: *mut ClStrResult) -> c_int;
    // include/dut_variants.h: the same from host arrays, the call of one locus, the unit notation, `find-strs` on files
    pub fn dut_str_measure(pos: *const i32, flag: *const u16, mapq: *const u8, cigar_off: *const u32, cigar: *const u32, n_reads: u64,
                           contig_len: u32, min_quality: u8, exclude_flags: u16, flank: u32, loci: *const ClStrLocus, n_loci: usize,
                           hist: *mut u32, partial: *mut u32, strands: u32) -> c_int;
    pub fn dut_str_call(hist_fwd: *const u32, hist_rev: *const u32, params: *const DutStrParams, call: *mut DutStrAlleleCall) -> c_int;
    pub fn dut_str_units(span: u32, delta: i32, period: u32, buf: *mut c_char) -> c_int;                   // buf: 24 bytes
    pub fn dut_find_strs_files(bam: *const c_char, fasta: *const c_char, contig: *const c_char, loci_path: *const c_char,
                               opt: *const DutStrOptions, output: *const c_char, device_id: c_int, err: *mut c_char, err_len: usize) -> c_int;
    // error profile (README "Error profile"): substitutions by reference base and read base, the same by distance from either
    // end of the read, and insertion and deletion events by the same distances, over [start, end) of the tile cl_site_upload
    // left resident; filter null: unfiltered, every read forward.  n_cycles 1..256.  Context-owned arrays, valid until the
    // next cl_site_error_profile / upload.  cl_site_error_profile_stats: the two launches of the last call apart
    pub fn cl_site_error_profile(ctx: *mut ClCtx, min_quality: u8, filter: *const ClScanFilter, n_cycles: u32, ref_bases: *const u8,
                                 ref_len: u64, start: u32, end: u32, out: *mut ClEpResult) -> c_int;
    pub fn cl_site_error_profile_stats(ctx: *mut ClCtx, table_ms: *mut f64, sum_ms: *mut f64) -> c_int;
    // include/dut_variants.h: the same from host arrays (tables: 36 * n_cycles words of the caller's), the TSV, `error-profile` on files
    pub fn dut_error_profile_measure(reads: *const DutEpReads, contig_len: u32, ref_bases: *const u8, ref_len: u64, start: u32, end: u32,
                                     opt: *const DutEpOptions, tables: *mut u64, out: *mut ClEpResult) -> c_int;
    pub fn dut_error_profile_write(path: *const c_char, contig: *const c_char, res: *const ClEpResult, opt: *const DutEpOptions,
                                   err: *mut c_char, err_len: usize) -> c_int;
    pub fn dut_error_profile_files(bam: *const c_char, fasta: *const c_char, contig: *const c_char, has_region: c_int, start: u32, end: u32,
                                   opt: *const DutEpOptions, output: *const c_char, device_id: c_int, err: *mut c_char, err_len: usize) -> c_int;
    // linked sites (README "Linked sites"): for strictly ascending 0-based sites the pair set (every site with the next
    // max_partners <= 15 sites within max_dist), per pair the 6 x 6 table of the classes A C G T del other one read observes at
    // both sites, per site its six counts, over the tile cl_site_upload left resident; filter null: unfiltered.  Context-owned
    // arrays, valid until the next cl_site_link_counts / upload.  At most 2^20 sites and 2^20 pairs
    pub fn cl_site_link_counts(ctx: *mut ClCtx, min_quality: u8, filter: *const ClScanFilter, sites: *const u32, n_sites: usize, max_dist: u32,
                               max_partners: u32, out: *mut ClLinkResult) -> c_int;
    // include/dut_variants.h: the pair set alone (first may be null), the same counts from host arrays (first: n_sites + 1, tables:
    // 36 per pair, site_counts: 6 per site, the caller's), one pair's summary, the sites file, the TSV, `phase-sites` on files
    pub fn dut_link_pair_offsets(sites: *const u32, n_sites: usize, max_dist: u32, max_partners: u32, first: *mut u32, n_pairs: *mut u64) -> c_int;
    pub fn dut_link_measure(reads: *const DutEpReads, contig_len: u32, opt: *const DutLinkOptions, sites: *const u32, n_sites: usize,
                            first: *mut u32, tables: *mut u32, site_counts: *mut u32) -> c_int;
    pub fn dut_link_summarise(site_counts_a: *const u32, site_counts_b: *const u32, table: *const u32, params: *const DutLinkParams,
                              out: *mut DutLinkSummary) -> c_int;
    pub fn dut_link_discordance_parse(text: *const c_char, per_10k: *mut u32, err: *mut c_char, err_len: usize) -> c_int;
    pub fn dut_link_sites_parse(path: *const c_char, contig: *const c_char, sites: *mut *mut u32, n_sites: *mut usize, n_skipped: *mut usize,
                                err: *mut c_char, err_len: usize) -> c_int;
    pub fn dut_link_sites_free(sites: *mut u32);
    pub fn dut_link_write(path: *const c_char, contig: *const c_char, sites: *const u32, n_sites: usize, n_skipped: usize, first: *const u32,
                          tables: *const u32, site_counts: *const u32, opt: *const DutLinkOptions, err: *mut c_char, err_len: usize) -> c_int;
    pub fn dut_find_links_files(bam: *const c_char, fasta: *const c_char, contig: *const c_char, sites_path: *const c_char,
                                opt: *const DutLinkOptions, output: *const c_char, device_id: c_int, err: *mut c_char, err_len: usize) -> c_int;
    // include/dut_fingerprint.h: the `fingerprint` sketch on the device (1 <= ksize <= 64)
    pub fn dut_fp_create(opt: *const DutFpOptions, device_id: c_int, stream: *mut c_void, out: *mut *mut DutFpCtx) -> c_int;
    pub fn dut_fp_push_seq4(ctx: *mut DutFpCtx, seq4: *const u8, base_off: *const u64, n_seq: u64) -> c_int;
    pub fn dut_fp_push_bytes(ctx: *mut DutFpCtx, bytes: *const u8, base_off: *const u64, n_seq: u64) -> c_int;
    pub fn dut_fp_finish(ctx: *mut DutFpCtx, out: *mut DutFpResult) -> c_int;
    pub fn dut_fp_destroy(ctx: *mut DutFpCtx);
    pub fn dut_fp_last_error(ctx: *const DutFpCtx) -> *const c_char;
    pub fn dut_fp_files(input: *const c_char, reference: *const c_char, output: *const c_char, opt: *const DutFpOptions,
                        region: *const c_char, device_id: c_int, digest_out: *mut c_char, processed_out: *mut u64,
                        err: *mut c_char, err_len: usize) -> c_int;
}

pub enum DutFpCtx {}
pub enum DutTree {}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ClScanCandidate {      // cl_scan_candidate: pos 1-based, ref / alt ASCII 'A' 'C' 'G' 'T'
    pub pos: u32, pub ref_base: u8, pub alt: u8, pub pad: [u8; 2],
    pub a: u32, pub c: u32, pub g: u32, pub t: u32, pub depth: u32,
}

#[repr(C)]
pub struct ClScanResult {         // cl_scan_result: the five classes add up to end - start
    pub start: u32, pub end: u32,
    pub n_low_depth: u64, pub n_mixed: u64, pub n_uncomparable: u64, pub n_match: u64, pub n_variant: u64,
    pub candidates: *const ClScanCandidate,                 // n_variant, ascending position
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ClScanFilter {         // cl_scan_filter: use_base_quality must be 0 for cl_site_str_lengths
    pub exclude_flags: u16, pub use_base_quality: u8, pub pad: u8,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ClStrLocus { pub start: u32, pub end: u32 }      // cl_str_locus: 0-based, half open

#[repr(C)]
pub struct ClStrResult {          // cl_str_result: hist[(i * strands + strand) * 128 + delta + 63], bin 127 = every other delta
    pub n_loci: usize, pub hist: *const u32, pub partial: *const u32, pub strands: u32,
}

#[repr(C)]
pub struct ClEpResult {           // cl_ep_result: total[4 * from + to] in A C G T; from5 / from3: n_cycles * 16; ins5 .. del3: n_cycles
    pub start: u32, pub end: u32, pub n_cycles: u32, pub pad: u32,
    pub n_reads: u64, pub n_bases: u64, pub n_uncomparable: u64, pub n_ins: u64, pub ins_bases: u64, pub n_del: u64, pub del_bases: u64,
    pub total: [u64; 16],
    pub from5: *const u64, pub from3: *const u64,
    pub ins5: *const u64, pub ins3: *const u64, pub del5: *const u64, pub del3: *const u64,
}

#[repr(C)]
pub struct ClLinkResult {         // cl_link_result: first: n_sites + 1; tables: n_pairs * 36; site_counts: n_sites * 6 (A C G T del other)
    pub n_sites: usize, pub n_pairs: usize,
    pub first: *const u32, pub tables: *const u32, pub site_counts: *const u32,
}

#[repr(C)]
pub struct DutLinkOptions {       // dut_link_options
    pub min_depth: u32, pub min_quality: u8, pub filtered: c_int, pub exclude_flags: u16, pub has_min_base_quality: c_int,
    pub min_base_quality: u8, pub max_dist: u32, pub max_partners: u32, pub min_link_count: u32, pub max_discord_per_10k: u32,
}

#[repr(C)]
pub struct DutLinkParams { pub min_depth: u32, pub min_link_count: u32, pub max_discord_per_10k: u32 }

#[repr(C)]
pub struct DutLinkSummary {       // dut_link_summary: status 0 low_depth, 1 cis, 2 trans, 3 unresolved; alleles 0..4: A C G T del
    pub status: c_int, pub major_a: u8, pub minor_a: u8, pub major_b: u8, pub minor_b: u8,
    pub depth_a: u64, pub depth_b: u64, pub both: u64, pub major_major: u64, pub major_minor: u64, pub minor_major: u64, pub minor_minor: u64, pub other: u64,   // MM Mm mM mm
}

#[repr(C)]
pub struct DutEpReads {           // dut_ep_reads: flag may be null unfiltered, qual_off / qual without a base-quality threshold
    pub n_reads: u64, pub pos: *const i32, pub flag: *const u16, pub mapq: *const u8, pub cigar_off: *const u32, pub cigar: *const u32,
    pub seq_off: *const u64, pub seq4: *const u8, pub qual_off: *const u64, pub qual: *const u8,
}

#[repr(C)]
pub struct DutEpOptions {         // dut_ep_options: filtered 0 = no flag read, every read forward, every base passes
    pub min_quality: u8, pub filtered: c_int, pub exclude_flags: u16, pub has_min_base_quality: c_int, pub min_base_quality: u8,
    pub n_cycles: u32,
}

#[repr(C)]
pub struct DutStrParams { pub min_depth: u32, pub min_allele_per_10k: u32 }

#[repr(C)]
pub struct DutStrAlleleCall {     // dut_str_allele_call: status 0 low_depth, 1 mixed, 2 called
    pub status: c_int, pub delta: i32, pub delta2: i32,
    pub count: u32, pub fwd: u32, pub rev: u32, pub count2: u32,
    pub n: u64, pub other: u64,
}

#[repr(C)]
pub struct DutStrOptions {        // dut_str_options
    pub min_depth: u32, pub min_quality: u8, pub exclude_flags: u16, pub flank: u32, pub min_allele_per_10k: u32,
}

#[repr(C)]
pub struct DutVariantNote {       // dut_variant_note: names / alleles null when known == 0
    pub known: c_int, pub names: *mut c_char, pub alleles: *mut c_char,
}
pub enum DutDepthAcc {}

#[repr(C)]
pub struct ClDepthProfile {       // cl_depth_profile: the arrays are context-owned, valid until the next profile / contig
    pub n_bins: u32, pub window: u32,
    pub n_windows: u64, pub extent: u64, pub sum_raw: u64, pub sum_qc: u64,
    pub hist_raw: *const u64, pub hist_qc: *const u64,     // n_bins each; the last bin saturates
    pub win_raw: *const u64, pub win_qc: *const u64,       // n_windows each, or null (window == 0)
}

#[repr(C)]
pub struct DutDepthSummary {      // dut_depth_summary; frac_at_least: depth >= 1, 5, 10, 15, 20, 30, 50, 100; -1.0 = not available
    pub positions: u64, pub mean: f64,
    pub q1: u32, pub median: u32, pub q3: u32,
    pub q1_saturated: u8, pub median_saturated: u8, pub q3_saturated: u8, pub reserved: u8,
    pub frac_at_least: [f64; 8],
}

#[repr(C)]
pub struct DutDepthOptions {      // dut_depth_options: n_bins 2..=4096, window >= 16 with windows_path; paths may be null
    pub n_bins: u32, pub window: u32,
    pub dist_path: *const c_char, pub windows_path: *const c_char, pub summary_path: *const c_char,
}

#[repr(C)]
pub struct ClDepthRuns {          // cl_depth_runs: run i = [start[i], start[i + 1]), the last one ends at extent; context-owned arrays
    pub kind: u32, pub n_edges: u32,
    pub extent: u64, pub n_runs: u64,
    pub start: *const u32, pub value: *const u32,          // n_runs each
}

#[repr(C)]
pub struct DutDepthBedOptions {   // dut_depth_bed_options: kind 0 raw / 1 qc; at most 64 strictly ascending edges, the first above 0
    pub path: *const c_char, pub kind: u32, pub edges: *const u32, pub n_edges: u32,
}

#[repr(C)]
pub struct DutFpOptions {         // dut_fp_options, include/dut_fingerprint.h
    pub ksize: u32, pub scaled: u64, pub max_frequency: u32, pub has_max_frequency: i32,
}

#[repr(C)]
pub struct DutFpResult {          // dut_fp_result: hashes / counts stay valid until dut_fp_destroy
    pub processed: u64, pub n_distinct: u64, pub n_entries: u64,
    pub hashes: *const u64, pub counts: *const u32, pub hexdigest: [c_char; 65],
}

#[repr(C)] #[derive(Default)]
pub struct ClLayoutInfo {         // cl_layout_info, include/callable_loci.h
    pub form: i32, pub counter_planes: u32,
    pub n_reads: u64, pub n_records: u64, pub n_windows: u64, pub n_qual: u64, pub n_cigar: u64,
    pub row_groups: u64, pub max_groups: u64, pub run_table_entries: u64,
    pub device_bytes: u64, pub upload_h2d_bytes: u64,
}
