/*
 * callable_loci.h -- C ABI of the MI355X (gfx950) callable-loci engine.
 *
 * This is the drop-in boundary for the per-contig hot path of DecodingUsTools' `coverage`
 * subcommand.  The reference has no FFI here: the seam is the Rust function
 *     callable_loci::process_single_contig            (src/callable_loci/mod.rs:44-52)
 * called by process_single_contig_api                 (src/api/coverage.rs:238-252).
 * Everything that function computes per reference position -- the htslib pileup columns
 * (mod.rs:65-71), process_position (mod.rs:17-42), CallableProfiler::process_position /
 * process_state (profilers/callable_profiler.rs:89-155) and ContigProfiler::process_position
 * (profilers/contig_profiler.rs:47-83) -- is replaced by the calls below.  What stays on the
 * caller's side (host code, above this ABI): BAM/FASTA decoding, the FUNMAP / maxcnt read
 * admission rule, the unique-read-name count, the BED text writer with its duplicate-line
 * behaviour (callable_profiler.rs:39-66) and the f64 summary derivation (report.rs:15-134).
 *
 * Plain C types only; no exceptions cross the boundary.  Every function returns CL_OK (0) or a
 * negative cl_status; cl_last_error() returns the message of the last failure on that context.
 * A context is bound to one HIP device and is NOT thread-safe: one host thread drives one
 * context (the reference is single-threaded, src/main.rs:63-67).  There is no CPU fallback: if
 * no HIP device is usable cl_create() fails.
 */
#ifndef CALLABLE_LOCI_H
#define CALLABLE_LOCI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CL_ABI_VERSION 1

typedef enum cl_status {
    CL_OK = 0,
    CL_ERR_INVALID = -1,      /* bad argument / call out of sequence                        */
    CL_ERR_DEVICE = -2,       /* HIP runtime error (message has the hipError string)        */
    CL_ERR_UNSORTED = -3,     /* reads not coordinate sorted (htslib: "unsorted input")     */
    CL_ERR_CIGAR = -4,        /* malformed CIGAR (the cases htslib asserts on)              */
    CL_ERR_NOMEM = -5,
    CL_ERR_RANGE = -6,        /* coordinate beyond what the engine addresses (2^32-1)       */
    CL_ERR_INTERNAL = -7      /* a device-side consistency check failed (nothing was written out of range) */
} cl_status;

/* CallableOptions, src/callable_loci/options.rs:2-9 (CLI defaults src/cli.rs:34-60:
 * 4, 500, 10, 20, 10, 1, 0.1).  selected_contigs stays with the caller. */
typedef struct cl_options {
    uint32_t min_depth;
    uint32_t max_depth;
    uint8_t  min_mapping_quality;
    uint8_t  min_base_quality;
    uint32_t min_depth_for_low_mapq;
    uint8_t  max_low_mapq;
    double   max_low_mapq_fraction;
} cl_options;

/* CalledState discriminants, src/callable_loci/types.rs:36-43 */
enum {
    CL_REF_N = 0, CL_CALLABLE = 1, CL_NO_COVERAGE = 2, CL_LOW_COVERAGE = 3,
    CL_EXCESSIVE_COVERAGE = 4, CL_POOR_MAPPING_QUALITY = 5
};

/* One tile of ACCEPTED reads of the current contig, structure-of-arrays, coordinate sorted
 * (tiles are pushed in order; the first read of a tile must not start before the last read of
 * the previous one).  "Accepted" = what htslib's bam_plp_push keeps: the caller has dropped
 * BAM_FUNMAP reads and applied the maxcnt rule (the host library's dut_admit_reads does both).
 * Fields are the ones the path consumes (mod.rs:22-37, contig_profiler.rs:54-76):
 *   pos        0-based leftmost reference coordinate (record.pos())
 *   mapq       record.mapq()
 *   cigar      BAM encoding len<<4|op, op codes M0 I1 D2 N3 S4 H5 P6 =7 X8
 *   qual       record.qual(): raw Phred bytes, l_seq per read, 0xFF when absent
 * The caller owns the buffers; they are copied before the call returns. */
typedef struct cl_read_tile {
    uint64_t        n_reads;
    const int32_t  *pos;        /* n_reads                       */
    const uint8_t  *mapq;       /* n_reads                       */
    const uint32_t *cigar_off;  /* n_reads + 1, cigar_off[0] may be non-zero (tile-relative base) */
    const uint32_t *cigar;      /* indexed by cigar_off          */
    const uint64_t *qual_off;   /* n_reads + 1                   */
    const uint8_t  *qual;       /* indexed by qual_off           */
} cl_read_tile;

/* What the caller reads back per contig (report.rs:40-86):
 *   state_counts      CallableProfiler::get_contig_counts, callable_profiler.rs:158-160
 *   the next five     ContigProfiler fields, contig_profiler.rs:11-15
 *   extent            number of positions classified: max(contig_len, largest read end)
 *                     (a read overhanging the contig end makes the reference walk past it)
 *   max_raw_depth     largest pileup column
 * n_reads (distinct read names) is a host-side count and not part of this struct. */
typedef struct cl_contig_summary {
    uint64_t state_counts[6];
    uint64_t n_covered_bases;
    uint64_t summed_coverage;
    uint64_t summed_baseq;
    uint64_t summed_mapq;
    uint64_t quality_bases;
    uint64_t extent;
    uint64_t max_raw_depth;
    uint64_t n_intervals;
} cl_contig_summary;

/* One run of equal state: [start, end) 0-based half open, exactly one BED line of
 * callable_profiler.rs:42-46 */
typedef struct cl_interval {
    uint32_t start;
    uint32_t end;
    uint32_t state;
} cl_interval;

typedef struct cl_ctx cl_ctx;

/* ---- lifecycle ------------------------------------------------------------------------- */
int  cl_abi_version(void);
int  cl_device_count(void);
/* device_id: HIP ordinal.  stream: an existing hipStream_t to enqueue on (e.g. the caller's
 * current stream), or NULL to let the context create its own. */
cl_status cl_create(const cl_options *opt, int device_id, void *stream, cl_ctx **out);
void cl_destroy(cl_ctx *ctx);
const char *cl_last_error(const cl_ctx *ctx);

/* ---- per contig: the replacement of process_single_contig ------------------------------- */
/* Starts a contig.  ref_bases: the contig_len FASTA bytes, case preserved (mod.rs:79-80: a
 * missing base reads as 'N'); ref_len < contig_len is allowed, the rest is 'N'. */
cl_status cl_contig_begin(cl_ctx *ctx, int32_t tid, uint32_t contig_len,
                          const uint8_t *ref_bases, uint64_t ref_len);
/* Optional size hint for the contig that was just begun: totals over all tiles that will be pushed.
 * Saves regrowing the staging / device buffers; never required.  Given before the first tile, it also lets the engine
 * allocate the contig's device buffers on a thread of its own while the caller admits and pushes the reads
 * (cl_contig_upload, cl_contig_abort, cl_contig_begin and cl_destroy wait for that thread). */
cl_status cl_contig_reserve(cl_ctx *ctx, uint64_t n_reads, uint64_t n_cigar_ops, uint64_t n_qual_bytes);
/* Optional, byte forms only (DUT_QUAL_FORM=bytes; a no-op in the default pass-bit form, where no quality byte goes to
 * the device): starts sending quality bytes to the device before their tile is pushed, so that the transfer runs
 * beside the caller's own work on the records (the host driver's read admission, say).  `qual` must be exactly
 * the bytes the NEXT cl_push_reads will present (tile.qual + tile.qual_off[0], tile.qual_off[n] - tile.qual_off[0]
 * of them) and must stay valid until that call returns; a push that presents anything else simply sends its own
 * bytes (the prefetch is dropped).  Blocks of less than 4 MiB are ignored.  Never required. */
cl_status cl_contig_prefetch_qual(cl_ctx *ctx, const uint8_t *qual, uint64_t n_bytes);
/* Appends a tile (coordinate order across tiles).  The caller's buffers are free again on return.  The base-quality
 * test of mod.rs:33 is taken here, where the quality bytes are read once ("or a packed pass-bitmask
 * variant"; 8d: q = 1/8): one bit per base stays in host staging, together with the tile's share of summed_baseq
 * (contig_profiler.rs:65-70, a per-read separable sum); cl_contig_upload lays the bits out as the rows the pileup
 * kernel counts.  With DUT_QUAL_FORM=bytes in the environment of cl_create the quality bytes themselves go to HBM
 * (small tiles via host staging, tiles of >= 4 MiB through a pinned staging ring) and are tested on the device. */
cl_status cl_push_reads(cl_ctx *ctx, const cl_read_tile *tile);
/* The packed pass-bitmask variant of cl_push_reads: for a caller that has taken the base-quality test of
 * mod.rs:33 itself, where it decodes the records (the library's own BAM reader does: dut_bam_read_contig_bits).  Same
 * tile, with instead of the quality bytes
 *   qual_off   n_reads + 1 offsets of the reads' quality VALUES, as in cl_read_tile -- now bit offsets into pass_bits
 *   pass_bits  bit g (word g / 64, bit g % 64) = 1 iff quality value g >= min_base_quality of the context's options
 *              (an absent quality string, 0xFF bytes, passes); bits beyond qual_off[n] are ignored
 *   pass_sum   per read: the sum of the quality values that pass, over the bases of its M/=/X operations that have a
 *              quality value (its share of summed_baseq, contig_profiler.rs:65-70; a read's sum is below 2^32)
 * Pass-bit form only (the default): with DUT_QUAL_FORM=bytes the engine needs the bytes and refuses with
 * CL_ERR_INVALID.  Tiles of both kinds may be mixed within a contig. */
typedef struct cl_read_tile_bits {
    uint64_t        n_reads;
    const int32_t  *pos;
    const uint8_t  *mapq;
    const uint32_t *cigar_off;
    const uint32_t *cigar;
    const uint64_t *qual_off;
    const uint64_t *pass_bits;
    const uint32_t *pass_sum;
} cl_read_tile_bits;
cl_status cl_push_reads_bits(cl_ctx *ctx, const cl_read_tile_bits *tile);
/* upload + run + collect in one call.  *intervals points at context-owned memory, valid until
 * the next cl_contig_begin / cl_destroy. */
cl_status cl_contig_finish(cl_ctx *ctx, cl_contig_summary *out,
                           const cl_interval **intervals, size_t *n_intervals);
/* Abandons the contig that was begun (the error path of a caller: mod.rs:79 `?` leaves process_single_contig the same
 * way).  A quality prefetch that no tile has claimed is waited for and discarded -- no copy reads the caller's buffer
 * once this returns, and the device's staging ring is free for other contexts --, staged reads are dropped.  The
 * message of cl_last_error() survives.  cl_contig_begin and cl_destroy imply it. */
cl_status cl_contig_abort(cl_ctx *ctx);

/* ---- the same, split so that a caller can keep a contig resident in HBM and re-run it ---- */
cl_status cl_contig_upload(cl_ctx *ctx);      /* H2D of everything pushed; synchronous     */
cl_status cl_contig_run(cl_ctx *ctx);         /* enqueue all kernels on the stream; async  */
cl_status cl_contig_collect(cl_ctx *ctx, cl_contig_summary *out,
                            const cl_interval **intervals, size_t *n_intervals);
cl_status cl_sync(cl_ctx *ctx);
/* device pointer + byte size of the resident per-contig summary record (cl_contig_summary
 * layout, valid after cl_contig_run completes) -- for gathering summaries across GPUs with a
 * collective without a host round trip */
cl_status cl_device_summary(cl_ctx *ctx, void **dev_ptr, size_t *bytes);

/* ---- depth distribution of the resident contig ------------------------------------------ */
/* What a coverage tool reports beside the intervals: the histogram of the per-position depths, their exact sums and
 * the sum per fixed window.  With raw[p] and qc[p], 0 <= p < extent, the raw_depth and qc_depth of mod.rs:17-42 (what
 * cl_debug_depths dumps; deletions and reference skips count in raw only):
 *   hist_raw[b], hist_qc[b]   positions with min(depth, n_bins - 1) == b: the last bin saturates
 *   sum_raw, sum_qc           the sums of all depths, exact whatever n_bins is
 *   win_raw[i], win_qc[i]     window > 0: the sums over [i * window, min((i + 1) * window, extent)),
 *                             n_windows = ceil(extent / window); window == 0: no table (NULL, n_windows 0)
 * so that sum hist == extent, extent - hist_raw[0] == n_covered_bases, sum_raw == summed_coverage, sum_qc ==
 * quality_bases and sum win == sum.  Every figure is a plain count: profiles of contigs, devices or ranks add up.
 * Reduced on the device by one extra kernel over the resident contig -- no per-position array exists anywhere --, taken
 * only when asked: cl_contig_run enqueues what it always did.  Any number of calls per resident contig, after
 * cl_contig_run (or cl_contig_finish); the call waits for the stream.  The arrays are context-owned host memory, valid
 * until the next cl_contig_depth_profile, cl_contig_begin or cl_destroy.
 * CL_ERR_INVALID: n_bins outside [CL_DEPTH_MIN_BINS, CL_DEPTH_MAX_BINS]; a window of 1 to CL_DEPTH_MIN_WINDOW - 1
 * positions (per-base output is not this call); no contig has been run; a context of the byte forms
 * (DUT_QUAL_FORM=bytes: pass-bit form only, like cl_push_reads_bits).  CL_ERR_DEVICE: a host-only debug context. */
#define CL_DEPTH_MIN_BINS 2u
#define CL_DEPTH_MAX_BINS 4096u
#define CL_DEPTH_MIN_WINDOW 16u
typedef struct cl_depth_profile {
    uint32_t n_bins, window;
    uint64_t n_windows, extent, sum_raw, sum_qc;
    const uint64_t *hist_raw, *hist_qc;   /* n_bins each             */
    const uint64_t *win_raw, *win_qc;     /* n_windows each, or NULL */
} cl_depth_profile;
cl_status cl_contig_depth_profile(cl_ctx *ctx, uint32_t n_bins, uint32_t window, cl_depth_profile *out);
/* Measurement: the kernel of the last cl_contig_depth_profile by device events, milliseconds; 0 unless cl_set_profiling
 * was on for that call. */
cl_status cl_contig_depth_profile_ms(cl_ctx *ctx, double *kernel_ms);

/* ---- GC bias: depth of the resident contig by the GC content around each position -------------------------------- */
/* What a WGS report shows right after the mean depth (Picard CollectGcBiasMetrics, the AT and GC dropout figures,
 * deepTools computeGCBias), per position and with a centred window.  ref[0, ref_len) are reference bytes; a base is GC
 * (one of G C g c), AT (one of A T a t) or invalid (every other byte: N, n, the IUPAC codes, S among them; and every
 * position < 0 or >= ref_len).  For every position p of [0, extent), with the window [p - window / 2, p - window / 2 +
 * window), g(p) its GC bases and v(p) its invalid bases:
 *   v(p) > max_invalid   p is skipped (n_skipped)
 *   otherwise            p is counted in bin b = 100 g(p) / (window - v(p)) (integer division, 0 <= b <= 100):
 *                        positions[b] += 1, sum_raw[b] += raw[p], sum_qc[b] += qc[p], zero_raw[b] += (raw[p] == 0)
 * with raw and qc the two depths of the depth profile above, so that sum positions + n_skipped == extent.  Every figure
 * is a plain count: records of contigs, devices or ranks add up (dut_gc_bias_add, dut_coverage.h), and two calls return
 * the same bytes.  ref_len may be smaller or larger than the extent; no base at or beyond the extent rounded up to 2048
 * is read; ref == NULL with ref_len == 0 is valid (everything is skipped).  The reference crosses the link as two bits
 * per position, packed on the host (gc_bits.h) and sent through the staging ring by EVERY call: nothing is cached across
 * calls (a caller that wants several windows pays the upload for each).  Reduced on the device by one kernel
 * (gc_bias.hip.h) -- no per-position array exists anywhere --, taken only when asked: cl_contig_run enqueues what it always
 * did.  Any number of calls per resident contig, after cl_contig_run (or cl_contig_finish), collected or not, in any
 * order with the other depth calls and cl_contig_run; the call waits for the stream and drops an unclaimed
 * cl_contig_prefetch_qual of the context (it holds the ring).  `out` is the caller's.
 * CL_ERR_INVALID: null out; null ref with ref_len > 0; window outside [1, CL_GC_MAX_WINDOW]; max_invalid >= window; no
 * contig has been run; a context of the byte forms.  CL_ERR_DEVICE: a host-only debug context. */
#define CL_GC_BINS 101
#define CL_GC_MAX_WINDOW 1024
typedef struct cl_gc_bias {
    uint32_t window, max_invalid, extent, pad_;
    uint64_t n_skipped;
    uint64_t positions[CL_GC_BINS], sum_raw[CL_GC_BINS], sum_qc[CL_GC_BINS], zero_raw[CL_GC_BINS];
} cl_gc_bias;
cl_status cl_contig_gc_bias(cl_ctx *ctx, const uint8_t *ref, uint64_t ref_len, uint32_t window, uint32_t max_invalid, cl_gc_bias *out);
/* Measurement: the kernel of the last cl_contig_gc_bias by device events (0 unless cl_set_profiling was on for that
 * call) and its pack + upload by the host's clock, milliseconds.  upload_ms may be NULL. */
cl_status cl_contig_gc_bias_ms(cl_ctx *ctx, double *kernel_ms, double *upload_ms);

/* ---- per-base depth of the resident contig, run-length encoded ---------------------------- */
/* What a coverage tool writes as its per-base and quantized depth BED: one run per stretch of equal value.  For the depth
 * kind of the call (CL_DEPTH_RAW: raw_depth, CL_DEPTH_QC: qc_depth of mod.rs:17-42, as above) every position p of
 * [0, extent) has a value:
 *   n_edges == 0                   the depth itself
 *   edges e_0 < e_1 < ... < e_k-1  the number of edges <= depth, 0 .. k: the band [e_v-1, e_v) the depth falls in
 *                                  (band 0 starts at depth 0, band k has no upper end)
 * and a run starts at p == 0 and wherever value(p) != value(p - 1).  The runs are maximal, ascending and cover
 * [0, extent): start[0] == 0, value[i] != value[i + 1], run i = [start[i], i + 1 < n_runs ? start[i + 1] : extent);
 * extent == 0 gives no run.  Built on the device from the resident rows and heads in two passes over the windows (count,
 * then write at the scanned offsets: the order does not depend on timing, two calls give the same arrays); only the runs
 * cross the link, no per-position array exists anywhere.  Taken only when asked: cl_contig_run enqueues what it always
 * did.  Any number of calls per resident contig, with any kinds and edge sets, after cl_contig_run (or cl_contig_finish),
 * interleaved with cl_contig_depth_profile and cl_contig_run; the call waits for the stream.  The arrays are
 * context-owned host memory, valid until the next cl_contig_depth_runs, cl_contig_begin or cl_destroy.
 * CL_ERR_INVALID (with a message): an unknown kind; n_edges > CL_RUNS_MAX_EDGES; edges == NULL with n_edges > 0; edges
 * that are not strictly ascending, or a first edge of 0; no contig has been run; a context of the byte forms
 * (DUT_QUAL_FORM=bytes).  CL_ERR_DEVICE: a host-only debug context.  CL_ERR_INTERNAL: the write pass met a slot beyond
 * what the count pass counted (it stores nothing out of range). */
#define CL_RUNS_MAX_EDGES 64u
enum { CL_DEPTH_RAW = 0, CL_DEPTH_QC = 1 };
typedef struct cl_depth_runs {
    uint32_t kind, n_edges;
    uint64_t extent, n_runs;
    const uint32_t *start, *value;   /* n_runs each; run i = [start[i], i + 1 < n_runs ? start[i+1] : extent) */
} cl_depth_runs;
cl_status cl_contig_depth_runs(cl_ctx *ctx, uint32_t kind, const uint32_t *edges, uint32_t n_edges, cl_depth_runs *out);
/* Measurement: both launches and the scan of the last cl_contig_depth_runs by device events, milliseconds; 0 unless
 * cl_set_profiling was on for that call. */
cl_status cl_contig_depth_runs_ms(cl_ctx *ctx, double *kernel_ms);

/* ---- targets: depth and callable-base summaries of the resident contig over a list of regions ---------------- */
/* What a coverage tool reports per region of a BED (exome or panel targets; mosdepth --by, Picard HsMetrics).  With raw[p]
 * and qc[p] as above and state[p] the position's CalledState (what the intervals say), for n targets [start_i, end_i),
 * 0-based half open, start_i <= end_i, in any order, overlapping, nested or repeated at will, and up to
 * CL_TARGET_MAX_THRESHOLDS depth thresholds t_0 < t_1 < ..., t_0 >= 1: with e_i = min(end_i, extent) and
 * s_i = min(start_i, e_i), record i holds
 *   start, end, len      s_i, e_i and e_i - s_i: a target at or beyond the extent has length 0 and zeros everywhere else
 *   sum_raw, sum_qc      the sums of raw[p] and qc[p] over [s_i, e_i), exact
 *   state[6]             the positions of each CalledState; they add up to len
 *   ge_raw[k], ge_qc[k]  the positions with raw[p] >= t_k and with qc[p] >= t_k, k < n_thresholds (0 beyond)
 * Every target is independent of the others; the records come in the order the targets were given; every figure is an
 * integer count and two calls return the same bytes (no count crosses workgroups through an atomic).  Three launches over
 * the resident contig (depth_targets.hip.h): per engine window the totals of the depth fields and their prefix at the
 * targets' ends inside it, a scan of the windows' totals, and one wave per target that also sums the states out of the
 * device's interval array.  Only the records cross the link.  Taken only when asked: cl_contig_run enqueues what it always
 * did.  Any number of calls per resident contig, interleaved with cl_contig_depth_profile, cl_contig_depth_runs and
 * cl_contig_run -- but the call reads the intervals of the last run, so the contig must have been collected
 * (cl_contig_collect or cl_contig_finish) since its last cl_contig_run: that is where counter-width re-runs and a too small
 * interval buffer are settled.  n_targets == 0 is valid (*out = NULL).  *out points at context-owned host memory, valid until
 * the next cl_contig_targets, cl_contig_begin or cl_destroy.
 * CL_ERR_INVALID (with a message; the context stays usable): a null out; null starts / ends with n_targets > 0; a target
 * with start > end; n_targets > CL_TARGETS_MAX; n_thresholds > CL_TARGET_MAX_THRESHOLDS; null thresholds with
 * n_thresholds > 0; thresholds that are not strictly ascending, or a first threshold of 0; no contig collected since its
 * last run; a context of the byte forms (DUT_QUAL_FORM=bytes).  CL_ERR_DEVICE: a host-only debug context.
 * CL_ERR_INTERNAL: a device-side check of an uploaded index failed (nothing was read or stored out of range). */
#define CL_TARGET_MAX_THRESHOLDS 8u
#define CL_TARGETS_MAX (1u << 24)
typedef struct cl_target_stats {
    uint32_t start, end;          /* clipped to the extent */
    uint32_t len, reserved;
    uint64_t sum_raw, sum_qc;
    uint32_t state[6];            /* types.rs:36-43 order */
    uint32_t ge_raw[CL_TARGET_MAX_THRESHOLDS], ge_qc[CL_TARGET_MAX_THRESHOLDS];
} cl_target_stats;
cl_status cl_contig_targets(cl_ctx *ctx, const uint32_t *starts, const uint32_t *ends, size_t n_targets,
                            const uint32_t *thresholds, uint32_t n_thresholds, const cl_target_stats **out);
/* Measurement: the three launches of the last cl_contig_targets by device events, milliseconds: their sum in *kernel_ms
 * and, when launch_ms is not NULL, k_target_depth, k_target_scan and k_target_finish apart; 0 unless cl_set_profiling was
 * on for that call. */
cl_status cl_contig_targets_ms(cl_ctx *ctx, double *kernel_ms, double launch_ms[3]);

/* ---- targets: minimum, quartiles and maximum of the depths per region ------------------------------------------- */
/* What a per-target table shows beside the mean (Picard HsMetrics min_coverage / max_coverage, mosdepth --use-median,
 * GATK DepthOfCoverage Q1 / median / Q3), and what the sums of cl_contig_targets cannot give.  Targets and clipping as
 * there: e_i = min(end_i, extent), s_i = min(start_i, e_i), len = e_i - s_i.  For each kind (raw, qc), with d[p] the depth
 * of that kind for p in [s_i, e_i), the five values are
 *   [0], [4]   the smallest and the largest d[p]
 *   [j]        j = 1, 2, 3 ([2] is the median): the smallest depth v with #{p : d[p] <= v} >= ceil(j * len / 4), i.e. the
 *              element (j * len + 3) / 4 - 1 of the sorted depths -- the quartile rule of dut_depth_stats (dut_coverage.h):
 *              for an even len the median is the lower middle value.  Whole numbers, exact.
 * A target of length 0 has all ten values 0.  Targets come in any order, overlapping, nested or repeated; the records come
 * in the order given; two calls return the same bytes (integer atomics only).  The host cuts the targets at the engine's
 * windows of 2048 positions into pieces, at most CL_TARGET_ORDER_MAX_PIECES of them (8 bytes each on the host and the
 * device); k_target_order (target_order.hip.h) rebuilds both depths per window and takes the extremes, the host reads one
 * word -- the largest raw depth of any target, the only synchronisation before the result -- and one more pass over the
 * windows follows per bit of it (about seven at 30x), each settling one bit of all six quartiles of every target.  No
 * per-position array exists on the device or the host; only the records cross the link.  Taken only when asked:
 * cl_contig_run enqueues what it always did.  Any number of calls per resident contig after cl_contig_run or
 * cl_contig_finish, interleaved with cl_contig_targets, cl_contig_depth_profile, cl_contig_depth_runs and cl_contig_run;
 * the call reads only the residents of the run, as cl_contig_depth_profile does, so the contig need not have been
 * collected.  n_targets == 0 is valid (*out = NULL).  *out points at context-owned host memory, valid until the next
 * cl_contig_target_order, cl_contig_begin or cl_destroy.
 * CL_ERR_INVALID (with a message; the context stays usable): a null out; null starts / ends with n_targets > 0; a target
 * with start > end (the message names it); n_targets > CL_TARGETS_MAX; no contig has been run; a context of the byte
 * forms (DUT_QUAL_FORM=bytes); more than CL_TARGET_ORDER_MAX_PIECES pieces (the message gives the count and the limit;
 * refused before anything is allocated or uploaded).  CL_ERR_DEVICE: a host-only debug context.  CL_ERR_INTERNAL: a
 * device-side check of an uploaded index failed (nothing was read or stored out of range). */
typedef struct cl_target_order {
    uint32_t start, end, len;     /* clipped to the extent */
    uint32_t raw[5], qc[5];       /* min, q1, median, q3, max */
} cl_target_order;                /* 52 bytes */
#define CL_TARGET_ORDER_MAX_PIECES (1u << 26)
cl_status cl_contig_target_order(cl_ctx *ctx, const uint32_t *starts, const uint32_t *ends, size_t n_targets,
                                 const cl_target_order **out);
/* Measurement: all launches of the last cl_contig_target_order by device events, milliseconds (0 unless cl_set_profiling
 * was on for that call), and, when n_rounds is not NULL, how many bit rounds it took: the bit length of the largest raw
 * depth of any target. */
cl_status cl_contig_target_order_ms(cl_ctx *ctx, double *kernel_ms, uint32_t *n_rounds);

/* ---- measurement ------------------------------------------------------------------------ */
enum { CL_K_PREP = 0, CL_K_BOUNDS = 1, CL_K_PILEUP = 2, CL_K_RLE = 3, CL_K_COUNT = 4 };
/* When on, every cl_contig_run brackets each kernel group with hipEvents on the stream. */
cl_status cl_set_profiling(cl_ctx *ctx, int on);
/* Accumulated milliseconds per kernel group and number of runs since the last reset.  The per-read index (read
 * ends, CIGAR checkpoints) and the window bounds are built on the host at cl_contig_upload, not in a run: CL_K_PREP
 * and CL_K_BOUNDS read 0 (the slots are kept so that the table's layout does not change). */
cl_status cl_get_kernel_ms(cl_ctx *ctx, double ms[CL_K_COUNT], uint64_t *n_runs);
cl_status cl_reset_kernel_ms(cl_ctx *ctx);
/* Bytes of the resident inputs the pileup kernel of the contig's form must read at least once, counted strictly --
 * the array elements that kernel addresses: pass-bit rows or quality bytes, read records or run-table entries and
 * per-read fields, reference bases, window records; no CIGAR word (none is resident) -- and of the intervals it leaves
 * behind (12 bytes each; the per-position counters and states never reach HBM): the traffic one cl_contig_run cannot
 * do without. */
cl_status cl_contig_bytes(cl_ctx *ctx, uint64_t *input_bytes, uint64_t *output_bytes);
/* What is resident for the uploaded contig: the form of the pileup kernel (3 pass-bit rows; 0 records + quality bytes,
 * 2 run table + quality bytes: DUT_QUAL_FORM=bytes), element counts, and the HBM the context holds. */
typedef struct cl_layout_info {
    int32_t  form;
    uint32_t counter_planes;      /* pass-bit form: 8, 16 or 32 bit-sliced counter planes                        */
    uint64_t n_reads, n_records, n_windows;
    uint64_t n_qual;              /* quality bytes of the contig (on the device only in the byte forms)          */
    uint64_t n_cigar;             /* CIGAR operations of the contig (never on the device)                        */
    uint64_t row_groups;          /* pass-bit form: UNITS of 128 bytes, 4 rows of one 256-position segment       */
    uint64_t max_groups;          /* ... most groups of 4 rows in any segment of any window                      */
    uint64_t run_table_entries;   /* byte form 2                                                                 */
    uint64_t device_bytes;        /* capacity of every device buffer of the context                              */
    uint64_t upload_h2d_bytes;    /* what cl_contig_upload (byte forms: and cl_push_reads) sent over the link    */
    uint32_t tail_wpc;            /* windows per chunk of the tail kernel, and how many chunks it launches (0, 0  */
    uint32_t tail_chunks;         /* for a contig without windows); DUT_TAIL_CHUNKS caps the chunks: a test hook   */
} cl_layout_info;
cl_status cl_contig_layout(cl_ctx *ctx, cl_layout_info *out);

/* ---- test hooks ------------------------------------------------------------------------- */
/* Re-runs the resident contig with per-position dumps: raw_depth, qc_depth, low_mapq_count
 * (mod.rs:17-42) and state, each `cap` entries (cap >= extent), host buffers, any may be NULL. */
cl_status cl_debug_depths(cl_ctx *ctx, uint32_t *raw, uint32_t *qc, uint32_t *low,
                          uint8_t *state, uint64_t cap);

/* The records the short-read form of the pileup kernel reads for ONE read (host code only, no device needed): what the
 * upload walk makes of a read at `pos` with the given CIGAR, mapping quality and quality-string length, the quality
 * bytes starting at offset `qual_off` -- a head {pos, span, qual offset of its run, mapq | 0x100 | run length << 16}
 * and a piece {pos of the run, 0, qual offset, mapq | run length << 16} per further M/=/X run (mod.rs:22-37: the read is
 * in every column of its span, the bases of its match operations that have a quality byte are tested).  Writes up to
 * `cap` records of four 32-bit words each to `out`, the count to *n_records (also when it exceeds cap) and the
 * phase (reference position - query offset of the first run, mod 16) to *phase.  Reads below min_mapping_quality get
 * the head alone; a read without a reference span gets no record. */
cl_status cl_debug_read_records(int32_t pos, const uint32_t *cigar, uint32_t n_ops, uint8_t mapq, uint8_t min_mapping_quality,
                                uint64_t qual_off, uint64_t qual_len, uint32_t *out, uint32_t cap,
                                uint32_t *n_records, uint32_t *phase);

/* Host only: the pass bits of n quality bytes (words_out: ceil(n / 64) 64-bit words, bit i of word i / 64 <-> byte i,
 * zeros above byte n) and the sum of the passing bytes, as cl_push_reads takes them -- at `level` 0 scalar, 1 SSE2,
 * 2 AVX2 where the CPU has it (else SSE2); 10, 11, 12: the same levels through the one-pass form (bits and sum together). */
cl_status cl_debug_qual_pack(const uint8_t *qual, uint64_t n, uint8_t min_base_quality, int level, uint64_t *words_out,
                             uint64_t *sum_out);
/* Host only: the reference's "is N" bits as cl_contig_upload sends them in the pass-bit form (mod.rs:100-101: a base
 * that is 'N' or 'n'; mod.rs:79-80: positions beyond the reference read as 'N'): bit i of word w <-> position 64 w + i,
 * n_words words for n_bases bases (levels as above). */
cl_status cl_debug_ref_n_bits(const uint8_t *ref, uint64_t n_bases, uint64_t n_words, int level, uint64_t *words_out);
/* Host only: the reference's two bit planes as cl_contig_gc_bias sends them (gc: the byte is one of G C g c; valid: one
 * of A C G T a c g t; both 0 for every other byte and beyond the bases): bit i of word w <-> position 64 w + i, n_words
 * words a plane for n_bases bases (levels as above). */
cl_status cl_debug_gc_bits(const uint8_t *ref, uint64_t n_bases, uint64_t n_words, int level, uint64_t *gc_out, uint64_t *valid_out);
/* A context WITHOUT a device, for the CPU test suite only: cl_contig_begin / cl_push_reads (pass-bit form) stage a
 * contig on the host exactly as a device context does, and cl_debug_pass_rows runs the upload's row builder over it.
 * Every call that needs a device fails with CL_ERR_DEVICE: there is no CPU pileup. */
cl_status cl_debug_host_create(const cl_options *opt, cl_ctx **out);
/* The pass-bit rows of the staged contig with ONE row stack per window (pass_rows.h: rows_window, the layout the
 * upload's is held against): n_groups[w] groups of 4 rows
 * per window of 2048 positions (n_win_cap entries at most; *n_windows = how many there are), the groups themselves window
 * after window in rows[0, cap_words) (256 words each: word (block << 2) | (row & 3) of group row >> 2; *n_words = how
 * many words there are, also when that exceeds cap_words), and the contig's share of summed_baseq from the push walk. */
cl_status cl_debug_pass_rows(cl_ctx *ctx, uint32_t *n_groups, uint32_t n_win_cap, uint32_t *rows, uint64_t cap_words,
                             uint64_t *n_words, uint32_t *n_windows, uint64_t *summed_baseq);

/* The pass-bit rows of the staged contig as cl_contig_upload builds them (pass_rows.h: rows_window_segments): a row stack
 * per SEGMENT of 256 positions, 8 segments per window.  heights[8 w + s] = units of segment s of window w (a unit = 4
 * rows x 8 blocks of 32 positions = 32 words: word ((block & 7) << 2) | (row & 3)), height_words[w] = the eight heights
 * as the window's record carries them, one byte each, segment 0 lowest -- or 0, the equal-heights form: a segment beyond
 * 255 units, or DUT_ROWS_UNIFORM=1 when the context was made -- (n_win_cap windows at most; *n_windows = how many there
 * are), and the units themselves, window after window and segment after segment, in units[0, cap_words) (*n_words = how
 * many words there are, also when that exceeds cap_words). */
cl_status cl_debug_pass_rows_segments(cl_ctx *ctx, uint32_t *heights, uint64_t *height_words, uint32_t n_win_cap, uint32_t *units,
                                      uint64_t cap_words, uint64_t *n_words, uint32_t *n_windows);

/* ---- config 5: site-list pileup (haplogroup::caller::process_region,
 *      src/haplogroup/caller.rs:62-152) ---------------------------------------------------- */
typedef struct cl_site_tile {
    uint64_t        n_reads;    /* ALL fetched records of the contig, no flag filter (:75-80) */
    const int32_t  *pos;
    const uint8_t  *mapq;
    const uint32_t *cigar_off;
    const uint32_t *cigar;
    const uint64_t *seq_off;    /* n_reads + 1, in BASES                                    */
    const uint8_t  *seq4;       /* BAM 4-bit packed bases, high nibble first                */
} cl_site_tile;
/* hist[n_sites*16]: per site (1-based vcf_pos, caller.rs:94) the number of reads with
 * mapq >= min_quality showing each 4-bit base code at an M/=/X position.
 * Only the reads that can add to the histogram are sent to the device (position inside the contig, mapq >= min_quality,
 * a site inside the reference span: two short reads in five at one site per ~300 bases); tiles with a read of 255
 * CIGAR operations or 65 535 bases and more travel whole.  The tile this call leaves on the device therefore serves this
 * call only: cl_site_run after it is refused (cl_site_upload gives a tile that serves any list). */
cl_status cl_site_pileup(cl_ctx *ctx, uint8_t min_quality, uint32_t contig_len,
                         uint64_t ref_len, const cl_site_tile *tile,
                         const uint32_t *sites, size_t n_sites, uint32_t *hist);

/* The same in two steps: the tile goes to HBM once (through the pinned staging ring) and stays resident -- until the
 * next cl_site_upload or cl_destroy -- and any number of site lists are run over it (find-y-branch --show-snps asks the
 * same reads about several lists; caller.rs:8-59 fetches the region again each time).  cl_site_pileup = both, for one
 * list (and sends less: above).
 * Every entry of the list gets its row, hist[i * 16 .. i * 16 + 15] for sites[i]: a row depends on the tile, on
 * min_quality and on the site's own value, never on the rest of the list -- not on its order, not on what else is in it,
 * not on whether the same site is entered again (each of its entries gets the same row).  A site of 0 and a site beyond
 * the contig or ref_len get a row of zeros.  The same holds for cl_site_pileup. */
cl_status cl_site_upload(cl_ctx *ctx, uint32_t contig_len, uint64_t ref_len, const cl_site_tile *tile);
cl_status cl_site_run(cl_ctx *ctx, uint8_t min_quality, const uint32_t *sites, size_t n_sites, uint32_t *hist);

/* Measurement: duration of the last cl_site_pileup's kernel (HIP events on the context's stream, milliseconds)
 * and its algorithmic bytes (4-bit bases, per-read fields and CIGAR words read, the sites'
 * counters written). */
cl_status cl_site_pileup_stats(cl_ctx *ctx, double *kernel_ms, uint64_t *bytes);

/* ---- the dense form: base counts and SNV calls at every position of a range of the resident tile ------------- */
/* Relative to the tile cl_site_upload left resident (a tile cl_site_pileup filtered for its own list does not serve:
 * CL_ERR_INVALID, as for cl_site_run), for every position p of [start, end), 0-based half open, end <= contig_len:
 *   hist[p][c]   what cl_site_run(ctx, min_quality, {p + 1}, 1, ...) returns for the 1-based site p + 1
 *   a c g t      hist[p][1], [2], [4], [8];  depth = the sum of all 16 codes (bases.len(), caller.rs:133)
 *   refbase      ref_bases[p] upper-cased if that is one of ACGT, else "other" (N, IUPAC codes, p >= ref_len)
 *   called       depth >= min_depth and largest hist[p][c] / depth >= 0.7 (caller.rs:132-149; the device takes the
 *                test as 10 * m >= 7 * depth in 64 bits, which is the same for every depth below 2^32)
 * and p falls in exactly one class: low_depth (depth < min_depth); mixed (deep enough, not called); uncomparable (called,
 * but the called code is not A/C/G/T or refbase is "other"); match (called, equal to refbase); variant (called, A/C/G/T
 * on both sides, different).  The five counts add up to end - start.  The positions of class variant come back as
 * candidates, all of them, ascending; the counting and the call happen on the device (k_site_scan), what crosses the
 * link is the reference bytes of the range going in and the candidates coming out.  The call at a position equals what
 * dut_call_sites makes of cl_site_run's histogram there.  Reads need not be coordinate sorted: counts are exact for any
 * order (a sorted tile is faster: a window's reads are then a short run of the tile).
 * ref_len must be the one given to cl_site_upload.  CL_ERR_INVALID (with a message): no resident tile, a filtered
 * tile, start > end, end > contig_len, min_depth == 0, another ref_len, a null argument; an empty range answers zeros.
 * CL_ERR_DEVICE: a host-only debug context.  out->candidates is context-owned, valid until the next cl_site_scan,
 * cl_site_upload or cl_destroy.  Any number of scans per resident tile, interleaved with cl_site_run. */
typedef struct cl_scan_candidate {
    uint32_t pos;                 /* 1-based */
    uint8_t  ref, alt, pad[2];    /* 'A' 'C' 'G' 'T' */
    uint32_t a, c, g, t, depth;
} cl_scan_candidate;
typedef struct cl_scan_result {
    uint32_t start, end;
    uint64_t n_low_depth, n_mixed, n_uncomparable, n_match, n_variant;   /* sum == end - start */
    const cl_scan_candidate *candidates;                                 /* n_variant, ascending position */
} cl_scan_result;
cl_status cl_site_scan(cl_ctx *ctx, uint8_t min_quality, uint32_t min_depth, const uint8_t *ref_bases,
                       uint64_t ref_len, uint32_t start, uint32_t end, cl_scan_result *out);
/* The counters themselves for a short range (at most CL_SCAN_MAX_DENSE positions): counts[(p - start) * 5 + 0..4] =
 * a, c, g, t, depth, into the caller's array.  Same tile, same refusals. */
#define CL_SCAN_MAX_DENSE (1u << 20)
cl_status cl_site_scan_counts(cl_ctx *ctx, uint8_t min_quality, uint32_t start, uint32_t end, uint32_t *counts);
/* Measurement: the kernel of the last scan of either form by device events (milliseconds) and its algorithmic bytes
 * (4-bit bases, records and CIGAR words read, reference bytes read, candidates or counters written; for the filtered form
 * also the pass bits and the flags). */
cl_status cl_site_scan_stats(cl_ctx *ctx, double *kernel_ms, uint64_t *bytes);

/* ---- the filtered, strand-aware form of the dense scan ------------------------------------------------------------ */
/* The attachment of the resident tile: per read its BAM flag, per base one pass bit, qual >= min_base_quality, taken on
 * the host by this call.  Base i of read r has the quality value qual[qual_off[r] + i] when
 * i < qual_off[r + 1] - qual_off[r], otherwise none; a base without a value passes, and so does 0xFF (absent qualities).
 * One bit per base (in the numbering of seq_off, to which the host realigns per read) and two bytes per read go to HBM
 * through the staging ring, never the quality bytes.  seq_off must be the array that was given to cl_site_upload (the
 * engine keeps no copy of the tile's host arrays; its length and total are checked).  A new attachment replaces the
 * earlier one; the next cl_site_upload or cl_site_pileup drops it.  CL_ERR_INVALID (with a message): no resident tile,
 * a tile cl_site_pileup filtered, another n_reads or another number of bases than the tile's, a null array, offsets
 * that decrease.  CL_ERR_DEVICE: a host-only debug context. */
typedef struct cl_site_quals {
    uint64_t        n_reads;
    const uint16_t *flag;
    const uint64_t *qual_off;   /* n_reads + 1 */
    const uint8_t  *qual;       /* may be NULL when qual_off[n_reads] == 0 */
    const uint64_t *seq_off;    /* n_reads + 1: cl_site_tile.seq_off of the resident tile */
} cl_site_quals;
cl_status cl_site_attach_quals(cl_ctx *ctx, const cl_site_quals *quals, uint8_t min_base_quality);

/* cl_site_scan / cl_site_scan_counts under a filter, by strand.  Relative to the definitions above:
 *   a read counts only if it counts there and (flag & exclude_flags) == 0;
 *   a base of it counts only if it counts there and (!use_base_quality or its pass bit is set);
 *   the read is reverse iff flag & 0x10, else forward;
 *   depth = all counted bases of all 16 codes, both strands; classes, the call (10 m >= 7 depth over the 16 codes summed
 *   over the strands) and the candidate order are those of cl_site_scan applied to the filtered counts.
 * With exclude_flags == 0 and use_base_quality == 0 the result equals cl_site_scan's (strands summed).  Positions the
 * device's counter planes cannot classify are settled with a 16-code count under the same filter.  Same refusals as
 * cl_site_scan, plus: nothing attached, a null filter.  Interleaves freely with cl_site_run, cl_site_scan and other
 * filters on one resident tile.  out->candidates is context-owned, valid until the next cl_site_scan_ex, cl_site_upload
 * or cl_destroy. */
typedef struct cl_scan_filter {
    uint16_t exclude_flags;       /* e.g. 0x704: unmapped, secondary, QC fail, duplicate (samtools --ff default) */
    uint8_t  use_base_quality;    /* 0 / 1 */
    uint8_t  pad;
} cl_scan_filter;
typedef struct cl_scan_candidate_ex {
    uint32_t pos;                 /* 1-based */
    uint8_t  ref, alt, pad[2];
    uint32_t a, c, g, t, depth;   /* both strands */
    uint32_t alt_fwd, alt_rev, ref_fwd, ref_rev;
} cl_scan_candidate_ex;
typedef struct cl_scan_result_ex {
    uint32_t start, end;
    uint64_t n_low_depth, n_mixed, n_uncomparable, n_match, n_variant;
    const cl_scan_candidate_ex *candidates;
} cl_scan_result_ex;
cl_status cl_site_scan_ex(cl_ctx *ctx, uint8_t min_quality, uint32_t min_depth, const cl_scan_filter *filter,
                          const uint8_t *ref_bases, uint64_t ref_len, uint32_t start, uint32_t end, cl_scan_result_ex *out);
/* counts[(p - start) * 9 + 0..8] = a_fwd a_rev c_fwd c_rev g_fwd g_rev t_fwd t_rev depth; at most CL_SCAN_MAX_DENSE
 * positions. */
cl_status cl_site_scan_counts_ex(cl_ctx *ctx, uint8_t min_quality, const cl_scan_filter *filter, uint32_t start,
                                 uint32_t end, uint32_t *counts);
/* ---- the minor mode of the dense scan: a second allele beside the most frequent one ------------------------------ */
/* Over the counters of cl_site_scan (filter == NULL) or cl_site_scan_ex (a filter; needs cl_site_attach_quals), for
 * every position p of [start, end):
 *   A C G T      the four counters, strands summed;  depth = the depth of the scan there (N and every other code included)
 *   major, c1    the largest of A C G T, the first in that order among equals, and its count
 *   minor, c2    the largest of the other three, the first in that order among equals, and its count
 *   low_depth    depth < min_depth
 *   minor        not low, c2 >= min_minor_count and 10000 * c2 >= min_minor_per_10k * depth (taken in 64 bits)
 *   single       everything else
 * The three counts add up to end - start.  The positions of class minor come back as candidates, all of them, ascending.
 * major_fwd .. minor_rev are the strand counts of the two bases under a filter and 0 without one.  ref is the upper-cased
 * reference byte ('N' at and beyond ref_len); it takes no part in the rule.
 * Refusals: those of cl_site_scan / cl_site_scan_ex, and CL_ERR_INVALID (with a message) for null params,
 * min_depth == 0, min_minor_count == 0, min_minor_per_10k outside [1, 5000].  out->candidates is context-owned, valid
 * until the next cl_site_scan_minor, cl_site_upload or cl_destroy; the candidates of cl_site_scan and cl_site_scan_ex
 * live elsewhere and stay valid across this call.  Interleaves freely with cl_site_run and every other scan;
 * cl_site_scan_stats speaks of this scan after it. */
typedef struct cl_minor_params { uint32_t min_depth, min_minor_count, min_minor_per_10k; } cl_minor_params;
typedef struct cl_minor_candidate {
    uint32_t pos;                         /* 1-based */
    uint8_t  ref, major, minor, pad;      /* major, minor: 'A' 'C' 'G' 'T' */
    uint32_t a, c, g, t, depth;           /* both strands */
    uint32_t major_fwd, major_rev, minor_fwd, minor_rev;
} cl_minor_candidate;
typedef struct cl_minor_result {
    uint32_t start, end;
    uint64_t n_low_depth, n_single, n_minor;      /* sum == end - start */
    const cl_minor_candidate *candidates;         /* n_minor, ascending position */
} cl_minor_result;
cl_status cl_site_scan_minor(cl_ctx *ctx, uint8_t min_quality, const cl_scan_filter *filter /* NULL: unfiltered form */,
                             const cl_minor_params *params, const uint8_t *ref_bases, uint64_t ref_len,
                             uint32_t start, uint32_t end, cl_minor_result *out);

/* ---- the deletion mode of the dense scan: per-position deletion counts and calls --------------------------------- */
/* The read gates are those of cl_site_scan (filter == NULL) or cl_site_scan_ex (a filter, exclude_flags included; needs
 * cl_site_attach_quals).  For every position p of [start, end):
 *   depth        the scan's depth: every base of an M/=/X operation, all 16 codes; under use_base_quality only bases whose
 *                pass bit is set.  Exactly the depth of cl_site_scan_counts / cl_site_scan_counts_ex at p.
 *   del          the reads passing the same gates that have a D operation (CIGAR op 2; N, op 3, is no deletion) covering
 *                p, with p < min(contig_len, ref_len), and whose carrier base exists.  The carrier is the read's last
 *                query base before the operation: query index y - 1, y = the query bases the operations before it consume
 *                (M I S = X), 1 <= y <= l_seq.  A leading D (y == 0), a D behind the point where the read has run out of
 *                bases (y > l_seq) and every D of a read with l_seq == 0 do not count.  Under use_base_quality the
 *                deletion counts only if the carrier's pass bit is set (a carrier without a quality value passes).
 *   span         depth + del, strands summed
 *   low_depth    span < min_depth
 *   deleted      not low, del >= min_del_count and 10000 * del >= min_del_per_10k * span (taken in 64 bits)
 *   kept         everything else
 * The three counts add up to end - start.  The positions of class deleted come back as candidates, all of them,
 * ascending.  del_fwd .. depth_rev are the strand counts under a filter and 0 without one.  ref is the upper-cased
 * reference byte ('N' at and beyond ref_len); it takes no part in the rule.  min_del_per_10k = 7000 is the calling
 * rule's 0.7 applied to the deletion.
 * Refusals: those of cl_site_scan / cl_site_scan_ex, and CL_ERR_INVALID (with a message) for null params,
 * min_depth == 0, min_del_count == 0, min_del_per_10k outside [1, 10000].  out->candidates is context-owned, valid until
 * the next cl_site_scan_dels, cl_site_upload or cl_destroy; the candidates of the other scans live elsewhere and stay
 * valid across this call.  Interleaves freely with cl_site_run and every other scan; cl_site_scan_stats speaks of this
 * scan after it. */
typedef struct cl_del_params { uint32_t min_depth, min_del_count, min_del_per_10k; } cl_del_params;
typedef struct cl_del_candidate {
    uint32_t pos;                         /* 1-based */
    uint8_t  ref, pad[3];
    uint32_t del, depth;                  /* both strands */
    uint32_t del_fwd, del_rev, depth_fwd, depth_rev;
} cl_del_candidate;
typedef struct cl_del_result {
    uint32_t start, end;
    uint64_t n_low_depth, n_kept, n_deleted;      /* sum == end - start */
    const cl_del_candidate *candidates;           /* n_deleted, ascending position */
} cl_del_result;
cl_status cl_site_scan_dels(cl_ctx *ctx, uint8_t min_quality, const cl_scan_filter *filter /* NULL: unfiltered form */,
                            const cl_del_params *params, const uint8_t *ref_bases, uint64_t ref_len,
                            uint32_t start, uint32_t end, cl_del_result *out);

/* ---- the insertion mode of the dense scan: per-position insertion counts, calls and the inserted sequences ---------- */
/* The read gates are those of cl_site_scan (filter == NULL) or cl_site_scan_ex (a filter; needs cl_site_attach_quals).
 * For every position p of [start, end):
 *   depth        the scan's depth, exactly that of cl_site_scan_counts / cl_site_scan_counts_ex at p.
 *   ins          the reads passing the same gates with a counting I operation (CIGAR op 1) anchored at p.  The anchor of
 *                an I operation is the reference position of the last base of the operation directly before it, which
 *                must be M, = or X with at least one base (VCF's placement: the base before the insertion).  A first
 *                operation and an I directly behind S H P D N or another I do not count.  The anchor base and every
 *                inserted base must exist in the read (query index < l_seq), p < min(contig_len, ref_len), and under
 *                use_base_quality the anchor's pass bit must be set (an anchor without a quality value passes; the
 *                inserted bases' qualities take no part).  At most one per read and position, so ins <= depth by strand.
 *   low_depth    depth < min_depth
 *   inserted     not low, ins >= min_ins_count and 10000 * ins >= min_ins_per_10k * depth (taken in 64 bits)
 *   kept         everything else
 * The three counts add up to end - start; the reference base takes no part.  The positions of class inserted come back
 * as candidates, all of them, ascending; ins_fwd .. depth_rev are the strand counts under a filter and 0 without one.
 * For every candidate, each counting insertion there comes back as one observation (a second launch over the candidates
 * only): key holds the 4-bit codes of the first min(len, 32) inserted bases as they stand in seq4, base j in key[j / 16]
 * at bits 60 - 4 * (j % 16), unused nibbles 0, so (key[0], key[1]) compares in sequence order.  Insertions longer than 32
 * bases that agree in length and in their first 32 bases cannot be told apart.  strand is 1 for a reverse read (flag &
 * 0x10) and 0 without a filter.  Observations are sorted by (pos, len, key, strand); n_obs == the sum of the candidates' ins.
 * Refusals: those of cl_site_scan_dels under the same checks, with min_ins_count / min_ins_per_10k (1..10000) in the
 * messages.  CL_ERR_INTERNAL (with a message): the second launch found another number of insertions at a candidate than
 * the first; nothing was stored out of range.  candidates and obs are context-owned, in storage of their own, valid
 * until the next cl_site_scan_ins, cl_site_upload or cl_destroy; any order of the other scans and this call on one tile
 * is allowed.  cl_site_scan_stats speaks of both launches after it; cl_site_scan_ins_stats tells them apart. */
typedef struct cl_ins_params { uint32_t min_depth, min_ins_count, min_ins_per_10k; } cl_ins_params;
typedef struct cl_ins_candidate {
    uint32_t pos;                         /* 1-based anchor */
    uint8_t  ref, pad[3];
    uint32_t ins, depth;                  /* both strands */
    uint32_t ins_fwd, ins_rev, depth_fwd, depth_rev;
} cl_ins_candidate;
typedef struct cl_ins_obs {
    uint32_t pos, len;                    /* 1-based anchor; inserted bases */
    uint64_t key[2];
    uint32_t strand, pad;
} cl_ins_obs;
typedef struct cl_ins_result {
    uint32_t start, end;
    uint64_t n_low_depth, n_kept, n_inserted;     /* sum == end - start */
    const cl_ins_candidate *candidates;           /* n_inserted, ascending position */
    uint64_t n_obs;
    const cl_ins_obs *obs;                        /* n_obs, by (pos, len, key, strand) */
} cl_ins_result;
cl_status cl_site_scan_ins(cl_ctx *ctx, uint8_t min_quality, const cl_scan_filter *filter /* NULL: unfiltered form */,
                           const cl_ins_params *params, const uint8_t *ref_bases, uint64_t ref_len,
                           uint32_t start, uint32_t end, cl_ins_result *out);
/* The kernel milliseconds of the last cl_site_scan_ins: its window scan and its allele launch (0 without candidates). */
cl_status cl_site_scan_ins_stats(cl_ctx *ctx, double *scan_ms, double *alleles_ms);

/* ---- the consensus mode of the dense scan: one byte per position, the called sequence with its deletions ------------ */
/* The read gates are those of cl_site_scan (filter == NULL) or cl_site_scan_ex (a filter; needs cl_site_attach_quals); the
 * carrier's pass bit gates a deletion exactly as in cl_site_scan_dels.  For every position p of [start, end): a, c, g, t
 * and depth are those of cl_site_scan_counts(_ex) at p (strands summed, depth over all 16 codes), del is the count of
 * cl_site_scan_dels there, span = depth + del, m the largest of a, c, g, t (the first in that order among equals).  The
 * first class whose condition holds:
 *   low_depth    span < min_depth                                                                     byte n
 *   deleted      del >= min_del_count and 10000 * del >= min_del_per_10k * span (in 64 bits)          byte -
 *   low_depth    depth < min_depth (enough reads span it, too few carry a base)                       byte n
 *   ref / alt    10 * m >= 7 * depth (in 64 bits): ref when the called base equals the upper-cased
 *                reference byte, else alt (also for a reference byte that is not A/C/G/T)             byte A C G T
 *   no_call      everything else: mixed columns, columns where N or an IUPAC code holds the majority  byte N
 * The five counts add up to end - start.  Positions at and beyond ref_len hold no counts and come out low_depth.  A
 * position is deleted exactly when cl_site_scan_dels lists it under the same gates and parameters.
 * cons holds end - start bytes, cons[p - start] for position p: context-owned, in storage of its own, valid until the next
 * cl_site_scan_consensus, cl_site_upload or cl_destroy.  There is no CL_SCAN_MAX_DENSE limit: any end <= contig_len is
 * accepted; start == end returns an empty result without a launch.
 * Refusals: those of cl_site_scan_dels, with its messages for the parameters.  Any order of this call and the other
 * scans on one tile is allowed; cl_site_scan_stats speaks of this scan after it. */
typedef struct cl_cons_params { uint32_t min_depth, min_del_count, min_del_per_10k; } cl_cons_params;
typedef struct cl_cons_result {
    uint32_t start, end;
    uint64_t n_low_depth, n_deleted, n_no_call, n_ref, n_alt;     /* sum == end - start */
    const uint8_t *cons;                                          /* end - start bytes of "n-ACGTN" */
} cl_cons_result;
cl_status cl_site_scan_consensus(cl_ctx *ctx, uint8_t min_quality, const cl_scan_filter *filter /* NULL: unfiltered form */,
                                 const cl_cons_params *params, const uint8_t *ref_bases, uint64_t ref_len,
                                 uint32_t start, uint32_t end, cl_cons_result *out);

/* ---- short tandem repeats: the length of the sample's sequence over whole intervals of the resident tile -------------- */
/* The unit is a locus [start, end) on the tile's contig, 0-based half open, with a flank F, not a position: how many bases
 * a read holds between the two flanks does not depend on where its aligner placed the gaps inside the repeat.
 * A read takes part iff it passes the gates of cl_site_scan (read start < contig_len, mapq >= min_quality; under a filter
 * (flag & exclude_flags) == 0, reverse iff flag & 0x10), has a reference span and overlaps the locus (pos < end and
 * pos + span > start).  Its CIGAR is walked with x, the reference position reached, from pos:
 *   M = X of length l    qlen += |[x, x+l) cut with [s, e)|; m_left += |... cut with [s-F, s)|; m_right += |... cut with
 *                        [e, e+F)|; x += l
 *   I of length l at x   s <= x <= e: qlen += l (both borders belong to the locus); s-F < x < s: i_left += l;
 *                        e < x < e+F: i_right += l; elsewhere nothing
 *   D                    x += l, nothing else (the deleted positions are simply not in qlen)
 *   N                    x += l; skipped = true if it overlaps [s, e)
 *   S H P                take no part
 * Stored bases take no part: neither seq4 nor pass bits are read, and a read with fewer stored bases than its CIGAR
 * consumes counts by its CIGAR.  The read is spanning iff m_left == F, m_right == F, i_left == 0, i_right == 0 and not
 * skipped -- both flanks matched base by base with no gap inside them (so pos <= s - F and pos + span >= e + F; a locus
 * with s < F has no spanning read) -- and partial otherwise.  A spanning read adds one to bin delta + 63 of its strand for
 * delta = qlen - (e - s) in [-63, 63], and to bin 127 ("other") for every other delta.
 * hist[(i * strands + strand) * CL_STR_BINS + bin] and partial[i] for loci[i], in the caller's order; loci may overlap,
 * repeat and come in any order.  strands is 1 without a filter and 2 with one, forward first.  The arrays are context-owned,
 * in storage of their own, valid until the next cl_site_str_lengths, cl_site_upload or cl_destroy; any order of this call,
 * cl_site_run and the scans on one tile is allowed, and the call builds the read index itself when it is the first on a
 * fresh tile.  n_loci == 0 returns an empty result without a launch.  cl_site_scan_stats speaks of this launch after it.
 * CL_ERR_INVALID (with a message, the context stays usable): no resident tile, a tile cl_site_pileup filtered, a filter
 * with nothing attached, filter->use_base_quality != 0 (base qualities take no part), flank outside
 * [1, CL_STR_MAX_FLANK], n_loci > CL_STR_MAX_LOCI, a locus with start >= end, end > contig_len or
 * end - start > CL_STR_MAX_SPAN, null loci with n_loci > 0, null out.  CL_ERR_DEVICE: a host-only debug context. */
#define CL_STR_BINS      128
#define CL_STR_MAX_FLANK 64
#define CL_STR_MAX_LOCI  65536
#define CL_STR_MAX_SPAN  1024
typedef struct cl_str_locus  { uint32_t start, end; } cl_str_locus;
typedef struct cl_str_result {
    size_t          n_loci;
    const uint32_t *hist;       /* n_loci * strands * CL_STR_BINS */
    const uint32_t *partial;    /* n_loci */
    uint32_t        strands;
} cl_str_result;
cl_status cl_site_str_lengths(cl_ctx *ctx, uint8_t min_quality, const cl_scan_filter *filter /* NULL: one strand */,
                              uint32_t flank, const cl_str_locus *loci, size_t n_loci, cl_str_result *out);

/* ---- error profile: substitutions and indels by read cycle, over a range of the resident tile --------------------------- */
/* One small table for the whole range [start, end) (0-based half open, end <= contig_len; hi = min(end, ref_len)), keyed
 * by where in the read a base stood instead of where on the contig: what `samtools stats` (mismatches per cycle) and
 * mapDamage (misincorporation by distance from either end) tabulate.  C = n_cycles.
 * A read takes part iff its start is < contig_len, mapq >= min_quality, its reference span is not empty and overlaps
 * [start, hi) and, under a filter, (flag & exclude_flags) == 0.  It is reverse iff a filter is given and flag & 0x10;
 * without a filter no flag is read and every read is forward.  L is its stored base count.  Its CIGAR is walked from pos
 * with x, the reference position reached (64 bits), and y, the stored bases consumed (M I S = X consume; D N H P do not).
 * For a query index q < L: d5 = q (forward) or L - 1 - q (reverse), d3 = L - 1 - d5; soft-clipped bases count towards q.
 *   aligned base   a base of an M/=/X operation at a position p of [start, hi) with query index q < L; under
 *                  use_base_quality its pass bit must be set.  c = its 4-bit code, R = the upper-cased reference byte at p.
 *                  c not one of 1 2 4 8 or R not one of ACGT: n_uncomparable += 1.  Otherwise f, t = the indices of R and c
 *                  in A C G T, both complemented for a reverse read (3 - f, 3 - t: the table is in the orientation the
 *                  molecule was sequenced in): total[4 f + t] += 1; d5 < C: from5[d5 * 16 + 4 f + t] += 1; d3 < C:
 *                  from3[d3 * 16 + 4 f + t] += 1
 *   insertion      an I operation of length l >= 1 directly behind an M/=/X operation of at least one base whose last
 *                  position x - 1 (the anchor) lies in [start, hi), when the anchor base (query index y - 1) and all l
 *                  inserted bases exist (y + l <= L) and, under use_base_quality, the anchor's pass bit is set:
 *                  n_ins += 1, ins_bases += l, ins5[d5] += 1 if d5 < C, ins3[d3] += 1 if d3 < C, by the anchor base
 *   deletion       a D operation (op 2, not N) of length l >= 1 whose first deleted position x lies in [start, hi) and
 *                  whose carrier, query index y - 1, exists (1 <= y <= L) and, under use_base_quality, passes:
 *                  n_del += 1, del_bases += l, del5 / del3 by the carrier's cycle under the same conditions
 * n_reads counts the reads that take part, each once; n_bases = the sum of total.  Every count is exact for any depth.
 * For a <= b <= c every count but n_reads over [a, c) is the sum of those over [a, b) and [b, c).
 * The arrays are context-owned, in storage of their own, valid until the next cl_site_error_profile, cl_site_upload or
 * cl_destroy; any order of this call, cl_site_run, the scans and cl_site_str_lengths on one tile is allowed, and the call
 * builds the read index itself when it is the first on a fresh tile.  start == end returns zeros without a launch.  Two
 * calls return identical bytes (no count crosses workgroups through an atomic).  cl_site_scan_stats speaks of both
 * launches, the table kernel and the sum of its workgroups' slices, after the call.
 * CL_ERR_INVALID (with a message, the context stays usable): everything cl_site_scan / cl_site_scan_ex refuse (no resident
 * tile, a tile cl_site_pileup filtered, start > end, end > contig_len, another ref_len, a null reference, a filter with
 * nothing attached), n_cycles outside [1, CL_EP_MAX_CYCLES], null out.  CL_ERR_DEVICE: a host-only debug context. */
#define CL_EP_MAX_CYCLES 256
typedef struct cl_ep_result {
    uint32_t start, end, n_cycles, pad;
    uint64_t n_reads, n_bases, n_uncomparable, n_ins, ins_bases, n_del, del_bases;
    uint64_t total[16];                       /* [4 * from + to], A C G T */
    const uint64_t *from5, *from3;            /* n_cycles * 16 */
    const uint64_t *ins5, *ins3, *del5, *del3;/* n_cycles */
} cl_ep_result;
cl_status cl_site_error_profile(cl_ctx *ctx, uint8_t min_quality, const cl_scan_filter *filter /* NULL: unfiltered, all forward */,
                                uint32_t n_cycles, const uint8_t *ref_bases, uint64_t ref_len,
                                uint32_t start, uint32_t end, cl_ep_result *out);
/* Measurement: the two launches of the last cl_site_error_profile apart, in milliseconds (their sum is what
 * cl_site_scan_stats reports): the table kernel, and the sum of the workgroups' slices. */
cl_status cl_site_error_profile_stats(cl_ctx *ctx, double *table_ms, double *sum_ms);

/* ---- linked sites: what one read observes at two positions of the resident tile --------------------------------------- */
/* Every scan above counts a column and forgets which read held which base; this call keeps, per pair of nearby sites, the
 * 6 x 6 table of the classes A C G T del other one read observes at both.
 * sites[0..n_sites): 0-based positions, strictly ascending, each < min(contig_len, ref_len) of the upload.  The pair set:
 * for anchor i the partners are j = i+1, i+2, ... while j <= i + max_partners and sites[j] - sites[i] <= max_dist;
 * first[i] is the CSR offset, pair first[i] + (j - i - 1) is (i, j), first[n_sites] = n_pairs.
 * A read takes part for anchor a = sites[i] iff it passes the gates of cl_site_scan (read start < contig_len,
 * mapq >= min_quality; under a filter (flag & exclude_flags) == 0) and its reference span covers a.  Its CIGAR is walked
 * from pos with x, the reference position, and y, the stored bases consumed (M I S = X consume); L is the stored base count.
 * Its observation at a site p:
 *   p in an M = X operation, q = y + (p - x) < L and (no use_base_quality or the pass bit of q set): the class of the 4-bit
 *     code at q -- 1 -> A (0), 2 -> C (1), 4 -> G (2), 8 -> T (3), every other code -> other (5); none when q >= L or the
 *     pass bit is clear
 *   p in a D operation (op 2) whose carrier y - 1 exists (1 <= y <= L) and, under use_base_quality, passes: del (4); none
 *     when the carrier does not exist or does not pass
 *   p in an N, or outside the read's span: none
 * -- the conventions of cl_site_scan_counts[_ex] for bases and of cl_site_scan_dels for deletions.
 * site_counts[i * 6 + c]: the reads that take part for site i and observe class c there.  tables[pair * 36 + 6 * ca + cb]:
 * the reads that take part for anchor i and observe ca at sites[i] and cb at sites[j]; a read with no observation at
 * either site adds nothing to the pair.  Mates are two reads.  Exact counts; two calls return identical bytes.
 * The arrays are context-owned, in storage of their own, valid until the next cl_site_link_counts, cl_site_upload or
 * cl_destroy; any order of this call, cl_site_run, the scans, cl_site_str_lengths and cl_site_error_profile on one tile is
 * allowed, and the call builds the read index itself when it is the first on a fresh tile.  n_sites == 0 returns an empty
 * result without a launch.  cl_site_scan_stats speaks of this launch after it.
 * CL_ERR_INVALID (with a message, the context stays usable): no resident tile, a tile cl_site_pileup filtered, a filter
 * with nothing attached, null sites with n_sites > 0, null out, n_sites > CL_LINK_MAX_SITES, sites not strictly ascending
 * (the message names the index), a site >= min(contig_len, ref_len), max_dist == 0, max_partners outside
 * [1, CL_LINK_MAX_PARTNERS], a pair set above CL_LINK_MAX_PAIRS (the message gives the count).  CL_ERR_DEVICE: a host-only
 * debug context.  The checks come before any device work. */
#define CL_LINK_CLASSES      6          /* A C G T del other */
#define CL_LINK_MAX_PARTNERS 15
#define CL_LINK_MAX_SITES    (1u << 20)
#define CL_LINK_MAX_PAIRS    (1u << 20)
typedef struct cl_link_result {
    size_t          n_sites, n_pairs;
    const uint32_t *first;         /* n_sites + 1 */
    const uint32_t *tables;        /* n_pairs * 36 */
    const uint32_t *site_counts;   /* n_sites * 6  */
} cl_link_result;
cl_status cl_site_link_counts(cl_ctx *ctx, uint8_t min_quality, const cl_scan_filter *filter /* NULL: unfiltered */,
                              const uint32_t *sites, size_t n_sites, uint32_t max_dist, uint32_t max_partners,
                              cl_link_result *out);

/* Host only: the pass bits of an attachment as cl_site_attach_quals builds them, words [0, n_words): bit i of word w
 * <-> base 64 w + i in seq_off numbering; bits of no read are zero. */
cl_status cl_debug_site_pass_bits(const cl_site_quals *quals, uint8_t min_base_quality, uint64_t *words_out, uint64_t n_words);

#ifdef __cplusplus
}
#endif
#endif /* CALLABLE_LOCI_H */
