/*
 * dut_bam.h -- alignment / reference file input for the coverage path, in C.
 *
 * Replaces what the reference gets from rust-htslib before the hot path starts:
 *   BamReaderFactory::open_indexed            src/utils/bam_reader.rs:7-14
 *   bam.fetch((tid, 0, contig_len)) + records src/callable_loci/mod.rs:53-55
 *   faidx::Reader::from_path / fetch_seq      src/api/coverage.rs:73, mod.rs:79-80
 * and the file-level driver CoverageAnalyzer::run_analysis (src/api/coverage.rs:53-115), BamStats, the
 * coverage figures and the HTML report included (dut_report.h, dut_coverage.h).
 *
 * BAM only (BGZF + BAM records; a .bai or .csi beside the file is used to seek to a contig when present,
 * otherwise the file is read forward).  CRAM is not supported.
 */
#ifndef DUT_BAM_H
#define DUT_BAM_H

#include "dut_coverage.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dut_bam dut_bam;
typedef struct dut_fasta dut_fasta;

/* Opens a BAM file and parses its header.  NULL on failure (message in err). */
dut_bam *dut_bam_open(const char *path, char *err, size_t err_len);
void dut_bam_close(dut_bam *b);
const char *dut_bam_error(const dut_bam *b);
int dut_bam_n_ref(const dut_bam *b);
const char *dut_bam_ref_name(const dut_bam *b, int tid);      /* header.tid2name */
uint32_t dut_bam_ref_len(const dut_bam *b, int tid);          /* header.target_len */
const char *dut_bam_header_text(const dut_bam *b, size_t *len);
int dut_bam_has_index(const dut_bam *b);
/* Mapped reads of a reference as the .bai metadata pseudo-bin records them (samtools idxstats), -1 when
 * there is no index or it carries no metadata.  Used to balance contigs over GPUs before decoding. */
int64_t dut_bam_ref_mapped(const dut_bam *b, int tid);

/* All records with refID == tid, file order, decoded into reader-owned SoA buffers that stay
 * valid until the next call on this reader.  seq_off (in bases) / seq4 (4-bit codes, two per
 * byte, continuous) are filled when non-NULL.  Returns 0 or a negative cl_status. */
int dut_bam_read_contig(dut_bam *b, int tid, dut_records *out, const uint64_t **seq_off, const uint8_t **seq4);
/* The same with the base-quality test of mod.rs:33 taken while the records are parsed (their bytes are in the cache
 * then): out->qual is NULL, out->pass_bits / out->pass_sum are filled (dut_records, dut_coverage.h) -- one bit per
 * base instead of one byte leaves the reader: what the file-level coverage path uses in the default pass-bit form. */
int dut_bam_read_contig_bits(dut_bam *b, int tid, uint8_t min_base_quality, dut_records *out);

/* `bam.records()` on a plain reader (utils/bam_reader.rs:16-24): every record of the file, mapped or
 * not, from the first one, until fn returns 0 or the file ends.  index = 0-based ordinal; qname
 * without its NUL; tlen = the template length field.  The reader is left at the first record. */
typedef int (*dut_bam_sample_fn)(void *ud, uint64_t index, uint16_t flag, uint32_t l_seq,
                                 const uint8_t *qname, size_t qname_len, int32_t tlen);
int dut_bam_sample(dut_bam *b, dut_bam_sample_fn fn, void *ud);

/* Every record of the file from the first one, mapped or not, in file order, without the index (the
 * `fingerprint` reader, readers/bam.rs:94-133; dut_fingerprint.h), a batch at a time: *n_seq records whose
 * bases total at most max_bases (at least one record), their sequences as 4-bit codes, two per byte,
 * continuous over the records (first base in the high nibble of byte 0), record i at bases
 * [base_off[i], base_off[i+1]).  Reader-owned until the next call on this reader; *n_seq = 0 at the end.
 * The first call -- and the first after dut_bam_read_contig -- starts at the first record. */
int dut_bam_next_seqs(dut_bam *b, uint64_t max_bases, uint64_t *n_seq, const uint64_t **base_off, const uint8_t **seq4);

/* FASTA with a faidx index (faidx::Reader::from_path, api/coverage.rs:73): the .fai beside the file is read and
 * validated, or built (and written there when possible) when it is missing.  NULL on failure. */
dut_fasta *dut_fasta_open(const char *path, char *err, size_t err_len);
void dut_fasta_close(dut_fasta *f);
/* The bases of one sequence, case preserved, reader-owned until the next call (fetch_seq, mod.rs:79).  A name the
 * index does not hold, a failed seek or read: negative cl_status, text in dut_fasta_error -- the reference fails
 * the contig there ("Error processing contig: ...").  A file shorter than its index says yields the bases that
 * are there (the rest reads as 'N', mod.rs:80). */
int dut_fasta_fetch(dut_fasta *f, const char *name, const uint8_t **bases, uint64_t *len);
const char *dut_fasta_error(const dut_fasta *f);

/* `coverage <bam> -r <fasta> -o <bed> -s <html> [-L contig]...` on one GPU: BamStats over the first
 * 10000 records, then per selected contig (ascending tid) read, admit, run the engine, append BED
 * lines; then write the CoverageOutput JSON (dut_report.h, what main.rs:68-69 puts in
 * ./summary.json) to summary_json (may be NULL).  The per-contig coverage figures `<contig>_coverage.svg` are
 * written beside the BED file (callable_profiler.rs:64-84) and, when summary_html is given, the HTML report
 * (api/coverage.rs:104; dut_report.h) to that path; NULL: no report, the JSON names "summary.html".
 * files.coverage_plots of the JSON lists the figures that exist relative to the working directory
 * (api/coverage.rs:263-274), in tid order.
 * contigs == NULL selects every header contig.  With a .bai and more than one selected contig the next
 * contig's records and bases are read ahead on a second reader while the current one is processed
 * (environment DUT_PIPELINE=0 turns that off; the output is the same either way).
 * Errors: negative cl_status, message in err ("None of the specified contigs (...) were found in
 * the BAM file" for an -L list that matches nothing, api/coverage.rs:187-204). */
int dut_coverage_files(const char *bam_path, const char *fasta_path, const char *bed_path,
                       const char *summary_json, const char *summary_html, const cl_options *opt,
                       const char *const *contigs, size_t n_contigs, int device_id, char *err, size_t err_len);


/* The same over SEVERAL devices of one node, below any Python or torch.distributed layer -- what a Rust caller of
 * process_contigs_api (api/coverage.rs:221-252) can bind: one host thread, one BAM / FASTA reader pair and one engine
 * context per entry of `devices` (HIP ordinals; the same ordinal may appear more than once: several contexts on one
 * device); the selected contigs are dealt to them by longest-processing-time-first on the index's mapped-read counts
 * (contig lengths when the index does not record them); every contig's runs, state counts and ContigProfiler numbers
 * come back through host memory and the BED is written by the calling thread in tid order with the duplicated last line
 * per contig (callable_profiler.rs:64-66), so the files are byte for byte those of the one-device call.  One process,
 * no collective.  The first error in tid order aborts the analysis, as the serial loop's `?` does.
 * flags: DUT_FILES_LEAVE_TO_EXIT -- the caller leaves the process right after the call (the command line tool): the
 * contexts, readers and decode buffers are not given back one by one.  n_devices == 1, flags == 0: dut_coverage_files. */
#define DUT_FILES_LEAVE_TO_EXIT 1u
int dut_coverage_files_multi(const char *bam_path, const char *fasta_path, const char *bed_path,
                             const char *summary_json, const char *summary_html, const cl_options *opt,
                             const char *const *contigs, size_t n_contigs, const int *devices, size_t n_devices,
                             unsigned flags, char *err, size_t err_len);

/* dut_coverage_files_multi that also writes the depth profile of every selected contig (cl_contig_depth_profile,
 * callable_loci.h; the statistics and the three file formats: dut_coverage.h, dut_depth_acc): the profile is taken on the
 * device while the contig is resident -- one more kernel per contig --, travels to the calling thread with the contig's
 * runs and is written in tid order, so one device and several give the same bytes; the files are complete when the call
 * returns.  BED, figures and summaries are those of dut_coverage_files_multi.  depth == NULL or no path given: exactly
 * that call.  Pass-bit form only (DUT_QUAL_FORM=bytes: CL_ERR_INVALID).
 *   n_bins        histogram bins, 2 .. 4096: depths 0 .. n_bins - 2 exactly, the last bin "n_bins - 1 or more"
 *   window        positions per window of windows_path, >= 16 (ignored without windows_path)
 * A bad n_bins or window is refused (CL_ERR_INVALID, message) before any file or device is touched; a depth file that
 * cannot be written is named in the message.
 *   dist_path, windows_path, summary_path    any may be NULL */
typedef struct dut_depth_options {
    uint32_t n_bins, window;
    const char *dist_path, *windows_path, *summary_path;
} dut_depth_options;
int dut_coverage_files_ex(const char *bam_path, const char *fasta_path, const char *bed_path,
                          const char *summary_json, const char *summary_html, const cl_options *opt,
                          const char *const *contigs, size_t n_contigs, const int *devices, size_t n_devices,
                          unsigned flags, const dut_depth_options *depth, char *err, size_t err_len);

/* dut_coverage_files_ex that also writes the depth BED of every selected contig: its per-base depth as runs of equal
 * value (cl_contig_depth_runs, callable_loci.h; the text: dut_depth_bed_write, dut_coverage.h), contig after contig in tid
 * order into one file, no header.  The runs are taken on the device while the contig is resident -- two more launches
 * and a scan per contig --, copied on the device's thread, and written by the calling thread behind the contig's BED
 * lines, so one device and several give the same bytes.  Both option sets work in one run.  bed == NULL or no path:
 * exactly dut_coverage_files_ex.  Pass-bit form only (DUT_QUAL_FORM=bytes: CL_ERR_INVALID).
 *   path      the depth BED
 *   kind      CL_DEPTH_RAW or CL_DEPTH_QC
 *   edges     n_edges band edges (dut_quantize_parse), strictly ascending, the first above 0, at most CL_RUNS_MAX_EDGES;
 *             n_edges == 0: exact depth
 * Bad options are refused (CL_ERR_INVALID, message) before any file or device is touched; a depth BED that cannot be
 * created or written is named in the message. */
typedef struct dut_depth_bed_options {
    const char *path;
    uint32_t kind;
    const uint32_t *edges;
    uint32_t n_edges;
} dut_depth_bed_options;
int dut_coverage_files_ex2(const char *bam_path, const char *fasta_path, const char *bed_path,
                           const char *summary_json, const char *summary_html, const cl_options *opt,
                           const char *const *contigs, size_t n_contigs, const int *devices, size_t n_devices,
                           unsigned flags, const dut_depth_options *depth, const dut_depth_bed_options *bed,
                           char *err, size_t err_len);

/* dut_coverage_files_ex2 that also writes the per-target table of a BED of regions (cl_contig_targets, callable_loci.h;
 * the BED reader and the table: dut_targets_*, dut_coverage.h).  Every selected contig's targets are taken on the device
 * while the contig is resident -- three more launches per contig that has targets --, copied on the device's thread, and
 * written by the calling thread behind the contig's BED lines: contigs in the order of the BED output, a contig's targets
 * in file order, a `total` line last; one device and several give the same bytes.  Combines with both other option sets
 * in one run.  targets == NULL or no bed_path: exactly dut_coverage_files_ex2.  Pass-bit form only.
 *   bed_path      the regions
 *   out_path      the table
 *   thresholds    n_thresholds depths (dut_thresholds_parse), strictly ascending, the first at least 1, at most
 *                 CL_TARGET_MAX_THRESHOLDS
 * A malformed BED, bad thresholds or a missing out_path are refused (CL_ERR_INVALID, message) before any device is
 * touched; so is a target on a contig the BAM header does not have (the message names its line).  Targets on contigs
 * the selection leaves out are skipped. */
typedef struct dut_target_options {
    const char *bed_path;
    const char *out_path;
    const uint32_t *thresholds;
    uint32_t n_thresholds;
} dut_target_options;
int dut_coverage_files_ex3(const char *bam_path, const char *fasta_path, const char *bed_path,
                           const char *summary_json, const char *summary_html, const cl_options *opt,
                           const char *const *contigs, size_t n_contigs, const int *devices, size_t n_devices,
                           unsigned flags, const dut_depth_options *depth, const dut_depth_bed_options *bed,
                           const dut_target_options *targets, char *err, size_t err_len);

/* dut_coverage_files_ex3 with flags for the per-target table.  DUT_TARGETS_ORDER: every contig's targets also go through
 * cl_contig_target_order while the contig is resident, and the table gets the ten columns raw_min ... qc_max behind the
 * others (dut_targets_write_*_ex, dut_coverage.h).  BED, summaries and every other output are what they are without the
 * flag; one device and several give the same bytes.  target_flags == 0: exactly dut_coverage_files_ex3.  The flag without
 * targets (targets == NULL or no bed_path), or an unknown flag, is refused (CL_ERR_INVALID, message) before any file or
 * device is touched. */
#define DUT_TARGETS_ORDER 1u
int dut_coverage_files_ex4(const char *bam_path, const char *fasta_path, const char *bed_path,
                           const char *summary_json, const char *summary_html, const cl_options *opt,
                           const char *const *contigs, size_t n_contigs, const int *devices, size_t n_devices,
                           unsigned flags, const dut_depth_options *depth, const dut_depth_bed_options *bed,
                           const dut_target_options *targets, unsigned target_flags, char *err, size_t err_len);

/* dut_coverage_files_ex4 that also takes every selected contig's GC-bias record (cl_contig_gc_bias, callable_loci.h)
 * while the contig is resident, from the FASTA bases the run holds for it anyway -- one more upload of 2 bits a position
 * and one more launch per contig --, and writes the bias table and / or the summary of dut_coverage.h: the contigs in the
 * order of the BED output, then the sum of their records (dut_gc_bias_add) as `total`; one device and several give the
 * same bytes.  Combines with every other option set in one run; BED, summaries and every other output are what they are
 * without it.  gc == NULL or neither path: exactly dut_coverage_files_ex4.  Pass-bit form only.
 *   bias_path, summary_path   either may be NULL
 *   window                    1 to CL_GC_MAX_WINDOW positions (the command line's default: 100)
 *   max_invalid               below window (the command line's default: 4)
 * A window or max_invalid outside these is refused (CL_ERR_INVALID, message) before any file or device is touched. */
typedef struct dut_gc_options {
    const char *bias_path;
    const char *summary_path;
    uint32_t window, max_invalid;
} dut_gc_options;
int dut_coverage_files_ex5(const char *bam_path, const char *fasta_path, const char *bed_path,
                           const char *summary_json, const char *summary_html, const cl_options *opt,
                           const char *const *contigs, size_t n_contigs, const int *devices, size_t n_devices,
                           unsigned flags, const dut_depth_options *depth, const dut_depth_bed_options *bed,
                           const dut_target_options *targets, unsigned target_flags, const dut_gc_options *gc,
                           char *err, size_t err_len);

#ifdef __cplusplus
}
#endif
#endif /* DUT_BAM_H */
