/*
 * dut_coverage.h -- host-side mirror of the reference's callable_loci module API, in C.
 *
 * These are the pieces of the `coverage` path that stay on the host, above the device engine of
 * callable_loci.h, with the reference's names, argument meaning and error behaviour:
 *
 *   dut_profiler_*            CallableProfiler            profilers/callable_profiler.rs:11-160
 *   dut_contig_stats          ContigProfiler (data part)  profilers/contig_profiler.rs:7-20
 *   dut_admit_reads           what htslib's pileup keeps: BAM_FUNMAP drop + bam_plp_set_maxcnt
 *                             rule (mod.rs:55-60), region filter of
 *                             bam.fetch((tid,0,len)) (mod.rs:53), distinct read names
 *                             (contig_profiler.rs:59-62)
 *   dut_process_single_contig callable_loci::process_single_contig   mod.rs:44-147
 *   dut_contig_derive         get_coverage_stats / get_quality_stats  contig_profiler.rs:93-157
 *   dut_compare_contig_names  report.rs:339-393
 *   dut_genome_summary_build  report.rs:26-126
 *
 * Records are handed over decoded, structure-of-arrays, one contig at a time -- what a BAM
 * reader (rust-htslib in the reference, utils/bam_reader.rs:7-14) yields for the contig.
 */
#ifndef DUT_COVERAGE_H
#define DUT_COVERAGE_H

#include "callable_loci.h"

#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* All fetched records of one contig, file order.  Same fields as SURVEY.md Appendix B. */
typedef struct dut_records {
    uint64_t        n;
    const int32_t  *pos;
    const uint16_t *flag;
    const uint8_t  *mapq;
    const uint32_t *cigar_off;   /* n+1 */
    const uint32_t *cigar;
    const uint64_t *qual_off;    /* n+1 */
    const uint8_t  *qual;
    const uint32_t *qname_off;   /* n+1 */
    const uint8_t  *qname;
    /* the packed variant (dut_bam_read_contig_bits; both NULL otherwise): the base-quality test already taken -- bit
     * qual_off[i] + k of pass_bits <-> quality value k of read i --, and per read the sum of the passing values over
     * its matched bases (cl_read_tile_bits, callable_loci.h).  `qual` may then be NULL. */
    const uint64_t *pass_bits;
    const uint32_t *pass_sum;
} dut_records;

/* ContigProfiler fields the report reads (contig_profiler.rs:7-20, report.rs:40-86) */
typedef struct dut_contig_stats {
    uint64_t length;
    uint64_t n_covered_bases;
    uint64_t summed_coverage;
    uint64_t summed_baseq;
    uint64_t summed_mapq;
    uint64_t quality_bases;
    uint32_t n_reads;
    uint32_t reserved;
} dut_contig_stats;

typedef struct dut_contig_derived {
    double coverage_percent;
    double average_depth;
    double average_mapq;
    double average_baseq;
    double q30_percentage;
} dut_contig_derived;

typedef struct dut_genome_summary {
    uint64_t total_bases;
    uint64_t callable_bases;
    double   callable_percentage;
    double   average_depth;
    double   average_mapq;
    double   average_baseq;
    double   q30_percentage;
    uint64_t total_unique_reads;
    uint64_t contigs_analyzed;
} dut_genome_summary;

typedef struct dut_profiler dut_profiler;

/* CallableProfiler::new -- creates/truncates the BED file.  NULL on I/O error. */
dut_profiler *dut_profiler_new(const char *bed_path);
/* Drop: flushes; like the reference it does not write a pending state. */
void dut_profiler_free(dut_profiler *p);
/* The per-contig coverage figure (callable_profiler.rs:48-59,64-84; utils/histogram_plotter.rs:74-101,412-440):
 * after enable_plots every BED line of state CALLABLE / POOR_MAPPING_QUALITY / REF_N is also a range of the
 * current figure -- the duplicated last line of the previous contig included, as in the reference.
 * largest_contig_length: the longest selected contig other than "chrM" (api/coverage.rs:210-215).
 * plot_bins: positions of the three states per stride (ceil(largest / 2000); "chrM": ceil(16569 / 200)),
 * n = contig_length / stride + 1 entries each (arrays may be NULL; filled only if cap >= n).
 * finish_plot: what finish_contig does after the last line -- writes `<dir of the BED>/<contig>_coverage.svg`
 * (this project's own drawing of those arrays) and clears the ranges.  Returns 1 if a file was written,
 * 0 if there was nothing to draw, negative on error. */
void dut_profiler_enable_plots(dut_profiler *p, uint32_t largest_contig_length);
int dut_profiler_plot_bins(const dut_profiler *p, const char *contig, uint32_t contig_length, uint32_t *stride,
                           uint32_t *callable, uint32_t *low_qual, uint32_t *ref_n, size_t cap, size_t *n_bins);
int dut_profiler_finish_plot(dut_profiler *p, const char *contig, uint32_t contig_length);
/* get_contig_counts (callable_profiler.rs:158-160): zeros for an unknown contig */
void dut_profiler_contig_counts(const dut_profiler *p, const char *contig, uint64_t out[6]);
/* Feeds one contig's runs (what process_position would have produced position by position,
 * callable_profiler.rs:122-155) and then finish_contig's write_state (:64-66, state is NOT
 * cleared, so the next contig re-emits this contig's last line). */
int dut_profiler_feed_contig(dut_profiler *p, const char *contig, const cl_interval *iv, size_t n_iv,
                             const uint64_t state_counts[6]);

/* Read admission.  accepted[i] (n bytes) = 1 for the reads htslib's pileup would hold AND that
 * span at least one reference position; *n_unique_names = distinct read names among them.
 * maxcnt follows mod.rs:56-60: max_depth if > 0 else 500.
 * Returns CL_OK, CL_ERR_UNSORTED for out-of-order input (htslib aborts the pileup). */
int dut_admit_reads(const cl_options *opt, int32_t tid, uint32_t contig_len, const dut_records *rec,
                    uint8_t *accepted, uint32_t *n_unique_names, uint64_t *n_accepted);

/* process_single_contig (mod.rs:44-147) on the device engine: admission, SoA tiles to
 * cl_push_reads, cl_contig_finish, BED runs to the profiler, ContigProfiler numbers to *stats
 * (stats->length is set to contig_len).  ref/ref_len as cl_contig_begin.
 * Errors: negative cl_status; message via cl_last_error(ctx) ("Error processing contig: ..." is
 * prefixed by the caller as in api/coverage.rs:251). */
int dut_process_single_contig(cl_ctx *ctx, dut_profiler *prof, dut_contig_stats *stats,
                              const cl_options *opt, const char *contig_name, int32_t tid,
                              uint32_t contig_len, const uint8_t *ref, uint64_t ref_len,
                              const dut_records *rec);

/* The same without a BED writer: the contig's runs (context-owned, valid until the next contig of ctx)
 * and state counts are handed back -- what a rank of a multi-GPU run sends to the rank that writes
 * the BED (decodingustools_amd/coverage.py). */
int dut_process_single_contig_runs(cl_ctx *ctx, dut_contig_stats *stats, const cl_options *opt, int32_t tid,
                                   uint32_t contig_len, const uint8_t *ref, uint64_t ref_len,
                                   const dut_records *rec, uint64_t state_counts[6],
                                   const cl_interval **intervals, size_t *n_intervals);

void dut_contig_derive(const dut_contig_stats *s, dut_contig_derived *out);
int  dut_compare_contig_names(const char *a, const char *b);
/* stats/callable for contigs already in dut_compare_contig_names order (report.rs:37-38) */
void dut_genome_summary_build(const dut_contig_stats *stats, const uint64_t *callable, size_t n_contigs,
                              dut_genome_summary *out);

/* ---- depth profile: statistics and text files of cl_contig_depth_profile's histograms ---------------------
 * (host code only; histograms of contigs, devices or ranks add up bin by bin) */
#define DUT_DEPTH_N_THRESHOLDS 8
/* the depths of frac_at_least[]: 1, 5, 10, 15, 20, 30, 50, 100 */
extern const uint32_t dut_depth_thresholds[DUT_DEPTH_N_THRESHOLDS];
typedef struct dut_depth_summary {
    uint64_t positions;            /* sum of the histogram                                                        */
    double   mean;                 /* sum / positions in f64; 0 without positions                                 */
    uint32_t q1, median, q3;       /* smallest depth d whose cumulative count reaches ceil(q * positions)         */
    uint8_t  q1_saturated, median_saturated, q3_saturated;   /* it is the last bin: "that depth or more"          */
    uint8_t  reserved;
    /* share of the positions with depth >= dut_depth_thresholds[k]; -1.0 = not available: the threshold lies
     * beyond the last exact bin (> n_bins - 1), the histogram cannot tell; 0 without positions */
    double   frac_at_least[DUT_DEPTH_N_THRESHOLDS];
} dut_depth_summary;
/* hist: n_bins >= 2 counts, the last bin saturating; sum: the exact sum of the depths.  CL_OK or CL_ERR_INVALID. */
int dut_depth_stats(const uint64_t *hist, uint32_t n_bins, uint64_t sum, dut_depth_summary *out);

/* The accumulator behind `--depth-dist`, `--depth-windows` and `--depth-summary`: contigs are added in the order their
 * lines shall have (the BED's), their histograms and sums also go into a `total`.
 *   windows file (written as the contigs are added; windows_path NULL: none), header
 *       #contig\tstart\tend\tmean_raw\tmean_qc
 *     one line per window [start, end) of every contig, the means sum / (end - start) in f64 as %.2f
 *   distribution file, header
 *       #contig\tkind\tdepth\tpositions\tfraction_at_or_above
 *     per contig, then for `total`: kind `raw`, then `qc`, one line per non-empty bin in ascending depth; the last bin's
 *     depth is written `<n_bins-1>+`; the fraction (positions at that depth or above / positions) as %.6f
 *   summary file, header
 *       #contig\tkind\tpositions\tsum\tmean\tq1\tmedian\tq3\tfrac_ge_1\tfrac_ge_5\tfrac_ge_10\tfrac_ge_15\tfrac_ge_20\tfrac_ge_30\tfrac_ge_50\tfrac_ge_100
 *     per contig, then for `total`: a `raw` and a `qc` line of dut_depth_stats: positions and sum as integers, the
 *     mean as %.4f, a quartile as an integer with `+` behind it when saturated, a fraction as %.6f or `NA`
 * dut_depth_acc_new: NULL when n_bins is outside [2, 4096], window is 1..15, or the windows file cannot be created. */
typedef struct dut_depth_acc dut_depth_acc;
dut_depth_acc *dut_depth_acc_new(uint32_t n_bins, uint32_t window, const char *windows_path);
void dut_depth_acc_free(dut_depth_acc *a);
/* p: n_bins and window as the accumulator's.  Copies what it keeps. */
int dut_depth_acc_add(dut_depth_acc *a, const char *contig, const cl_depth_profile *p);
/* the total so far: context-owned, n_bins entries each */
int dut_depth_acc_total(const dut_depth_acc *a, const uint64_t **hist_raw, const uint64_t **hist_qc, uint64_t *sum_raw, uint64_t *sum_qc);
/* closes the windows file and writes the other two (either path may be NULL) */
int dut_depth_acc_finish(dut_depth_acc *a, const char *dist_path, const char *summary_path);

/* ---- per-base depth: the text of cl_contig_depth_runs' runs (host code only) -------------------------------
 * dut_quantize_parse: the band edges of `--quantize SPEC`, colon separated whole numbers that ascend strictly, at most
 * CL_RUNS_MAX_EDGES of them: "1:4:100" = the bands 0, 1-3, 4-99 and 100 or more.  As mosdepth writes them, a leading
 * "0:" and a trailing ":" are accepted and say nothing more: "0:1:4:100:" is "1:4:100".  NULL or empty text: no edge,
 * *n_edges = 0 (exact depth).  edges: room for CL_RUNS_MAX_EDGES values.  CL_OK, or CL_ERR_INVALID with the reason in
 * err (an empty or non-numeric edge, a value beyond 2^32 - 1, edges that do not ascend, no edge above 0, more than 64).
 * dut_depth_bed_write: one contig's runs as tab-separated lines, no header, as mosdepth's per-base.bed and quantized.bed:
 *     contig\tstart\tend\tDEPTH          r->n_edges == 0
 *     contig\tstart\tend\tLO:HI          the value's band: 0:e_0 for value 0, e_v-1:e_v, and e_k-1:inf for the last
 * with end = the next run's start, r->extent for the last run.  edges: the r->n_edges edges the runs were taken with. */
int dut_quantize_parse(const char *spec, uint32_t *edges, uint32_t *n_edges, char *err, size_t err_len);
int dut_depth_bed_write(FILE *f, const char *contig, const cl_depth_runs *r, const uint32_t *edges);

/* ---- targets: a BED of regions in, the table of cl_contig_targets' records out (host code only) ---------------
 * dut_targets_parse: BED text.  A line wants at least 3 tab- or blank-separated columns, contig start end, 0-based half
 * open, whole numbers up to 2^32 - 1, start <= end; column 4 is the target's name, else ".".  Blank lines and lines that
 * start with `#`, `track` or `browser` are skipped; a line may end in CR LF.  The targets are grouped by contig, the
 * contigs in the order they first appear, a contig's targets in file order.  NULL with the reason, line number first,
 * in err for a malformed line (fewer than 3 columns, a malformed or too large number, start > end); an empty file is a
 * valid list without contigs.  dut_targets_read: the same of a file (NULL also when it cannot be read).
 * dut_targets_get: contig c's arrays, context-owned: starts, ends, names, and the 1-based line of every target.
 * dut_thresholds_parse: `--target-thresholds LIST`, comma separated whole numbers that ascend strictly, the first at
 * least 1, at most CL_TARGET_MAX_THRESHOLDS of them; NULL or empty text: 1,10,20,30.  CL_OK, or CL_ERR_INVALID with the
 * reason in err.
 * The table (tab separated):
 *     #contig start end name length mean_raw mean_qc callable callable_frac ref_n no_coverage low_coverage
 *     excessive_coverage poor_mapping_quality raw_ge_T... qc_ge_T...      (T: each threshold)
 * one line per target, start, end and length clipped to the contig's extent; the means are sum / length in f64 as %.4f,
 * callable_frac callable / length as %.6f, both `NA` for length 0; everything else is a count of positions.
 * dut_targets_write adds every record to *total (may be NULL); dut_targets_write_total writes the last line, `total . . .`
 * and the column sums -- targets that overlap count twice there -- with the means and the fraction taken over the sums. */
typedef struct dut_targets dut_targets;
dut_targets *dut_targets_parse(const char *text, size_t len, char *err, size_t err_len);
dut_targets *dut_targets_read(const char *path, char *err, size_t err_len);
void dut_targets_free(dut_targets *t);
size_t dut_targets_n_contigs(const dut_targets *t);
const char *dut_targets_contig(const dut_targets *t, size_t c, size_t *n_targets);
int dut_targets_get(const dut_targets *t, size_t c, const uint32_t **starts, const uint32_t **ends, const char *const **names,
                    const uint32_t **lines);
int dut_thresholds_parse(const char *spec, uint32_t *thresholds, uint32_t *n_thresholds, char *err, size_t err_len);
typedef struct dut_target_total {
    uint64_t n_targets, len, sum_raw, sum_qc, state[6];
    uint64_t ge_raw[CL_TARGET_MAX_THRESHOLDS], ge_qc[CL_TARGET_MAX_THRESHOLDS];
} dut_target_total;
int dut_targets_write_header(FILE *f, const uint32_t *thresholds, uint32_t n_thresholds);
int dut_targets_write(FILE *f, const char *contig, const cl_target_stats *stats, const char *const *names, size_t n,
                      uint32_t n_thresholds, dut_target_total *total);
int dut_targets_write_total(FILE *f, const dut_target_total *total, uint32_t n_thresholds);
/* The same table with the order statistics of cl_contig_target_order behind the existing columns, ten more:
 *     raw_min raw_q1 raw_median raw_q3 raw_max qc_min qc_q1 qc_median qc_q3 qc_max
 * whole numbers; `NA` for a target of length 0 and on the `total` line (quantiles do not add).  order_columns != 0 asks
 * for the ten in the header and on the total line; dut_targets_write_ex writes them when `order` is not NULL: n records
 * of the same targets as stats (CL_ERR_INVALID where a record's clipped start or end differs from its partner's).  With
 * order_columns == 0 and order == NULL the three are the functions above, which forward here and write the bytes they
 * always wrote. */
int dut_targets_write_header_ex(FILE *f, const uint32_t *thresholds, uint32_t n_thresholds, int order_columns);
int dut_targets_write_ex(FILE *f, const char *contig, const cl_target_stats *stats, const cl_target_order *order,
                         const char *const *names, size_t n, uint32_t n_thresholds, dut_target_total *total);
int dut_targets_write_total_ex(FILE *f, const dut_target_total *total, uint32_t n_thresholds, int order_columns);

/* ---- GC bias: sums, statistics and text files of cl_contig_gc_bias' records (host code only) -----------------
 * dut_gc_bias_add: total += part, bin by bin and n_skipped (plain counts: contigs, devices and ranks add up); extent
 * is added too and saturates at 2^32 - 1.  A total whose window is 0 (a zeroed record) takes the part's window and
 * max_invalid; otherwise CL_ERR_INVALID where they differ, the total unchanged.
 * dut_gc_bias_stats, all in f64, each operand converted from its exact 64-bit integer first, sums taken in ascending
 * bin order from 0.0:
 *   P = sum positions, S_raw = sum sum_raw, S_qc = sum sum_qc                 (64-bit integers, exact)
 *   mean_raw[b] = sum_raw[b] / positions[b], mean_qc[b] likewise, zero_frac[b] = zero_raw[b] / positions[b]
 *   total_mean_raw = S_raw / P, total_mean_qc = S_qc / P
 *   norm_raw[b] = mean_raw[b] / total_mean_raw, norm_qc[b] likewise
 *   at_dropout_raw = 100 * (sum over b = 0..50 of max(0, positions[b] / P - sum_raw[b] / S_raw))
 *   gc_dropout_raw the same over b = 51..100; both likewise for qc with sum_qc and S_qc      (Picard's AT_DROPOUT, GC_DROPOUT)
 * A quotient whose denominator is 0, and whatever is computed from one, is "not available": DUT_GC_NA (every
 * available figure is >= 0).
 * The bias table (tab separated), one line per non-empty bin (positions[b] > 0) in ascending gc:
 *     #contig gc positions mean_raw mean_qc norm_raw norm_qc zero_frac
 * the means as %.4f, norm_* and zero_frac as %.6f, `NA` where not available.  The summary, one line per record:
 *     #contig window max_invalid positions skipped mean_raw mean_qc at_dropout_raw gc_dropout_raw at_dropout_qc gc_dropout_qc
 * positions = P, skipped = n_skipped, the means (total_mean_*) as %.4f, the dropouts as %.6f, `NA` where not available. */
#define DUT_GC_NA (-1.0)
typedef struct dut_gc_stats {
    uint64_t positions, sum_raw, sum_qc;           /* P, S_raw, S_qc */
    double total_mean_raw, total_mean_qc;
    double at_dropout_raw, gc_dropout_raw, at_dropout_qc, gc_dropout_qc;
    double mean_raw[CL_GC_BINS], mean_qc[CL_GC_BINS], norm_raw[CL_GC_BINS], norm_qc[CL_GC_BINS], zero_frac[CL_GC_BINS];
} dut_gc_stats;
int dut_gc_bias_add(cl_gc_bias *total, const cl_gc_bias *part);
int dut_gc_bias_stats(const cl_gc_bias *g, dut_gc_stats *out);
int dut_gc_bias_write_header(FILE *f);
int dut_gc_bias_write(FILE *f, const char *contig, const cl_gc_bias *g);
int dut_gc_summary_write_header(FILE *f);
int dut_gc_summary_write(FILE *f, const char *contig, const cl_gc_bias *g);

/* Debug names of CalledState (types.rs:36-43) */
const char *dut_state_name(uint32_t state);

#ifdef __cplusplus
}
#endif
#endif /* DUT_COVERAGE_H */
