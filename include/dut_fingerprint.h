/*
 * dut_fingerprint.h -- the `fingerprint` subcommand of the reference (commands/fingerprint.rs,
 * collectors/fingerprint/): a scaled k-mer MinHash sketch of every read of a BAM or FASTQ file.
 *
 * Per window of k bases: windows with an uppercase 'N' are skipped; the rest are hashed as
 * SeaHash(min(kmer, revcomp(kmer))) (byte order; revcomp maps every byte outside ACGT to 'N'), and a
 * hash h <= max_hash is counted.  The sketch is the sorted (h, count) table; its digest is SHA-256 over
 * h (8 bytes LE) || count (4 bytes LE) of every entry with count <= max_frequency.
 *
 * The hashing, the compaction of the survivors and the sorted table live on the device (fingerprint.hip).
 * Limits of this implementation: 1 <= k <= 64 (CL_ERR_INVALID otherwise); no CRAM, no GAM.
 * Errors are negative cl_status values (callable_loci.h); dut_fp_last_error gives the message.
 */
#ifndef DUT_FINGERPRINT_H
#define DUT_FINGERPRINT_H

#include "callable_loci.h"
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dut_fp_options {
    uint32_t ksize;                 /* 1..64 (reference default 31)                                   */
    uint64_t scaled;                /* max_hash = u64::MAX / scaled, saturating (0 and 1: u64::MAX)     */
    uint32_t max_frequency;         /* entries with count > max_frequency are left out of the output    */
    int32_t has_max_frequency;      /* 0: no frequency filter                                           */
} dut_fp_options;

typedef struct dut_fp_result {
    uint64_t processed;             /* sequences with length >= ksize                                   */
    uint64_t n_distinct;            /* distinct hashes kept, before the frequency filter                */
    uint64_t n_entries;             /* entries of hashes / counts (after the filter), ascending hash    */
    const uint64_t *hashes;         /* valid until dut_fp_destroy                                       */
    const uint32_t *counts;
    char hexdigest[65];             /* lowercase, NUL terminated                                        */
} dut_fp_result;

typedef struct dut_fp_ctx dut_fp_ctx;

/* stream: an existing hipStream_t to enqueue on, or NULL for a stream of the context's own. */
int dut_fp_create(const dut_fp_options *opt, int device_id, void *stream, dut_fp_ctx **out);
/* n_seq sequences; sequence i is bases [base_off[i], base_off[i+1]) (base_off has n_seq + 1 entries,
 * ascending).  seq4: BAM's 4-bit codes (=ACMGRSVTWYHKDBN), two per byte, first base in the high nibble of
 * byte 0, continuous over the sequences.  bytes: one byte per base.  Synchronous: the batch is hashed and
 * merged into the device table when the call returns.  Offsets that are not ascending: CL_ERR_INVALID. */
int dut_fp_push_seq4(dut_fp_ctx *ctx, const uint8_t *seq4, const uint64_t *base_off, uint64_t n_seq);
int dut_fp_push_bytes(dut_fp_ctx *ctx, const uint8_t *bytes, const uint64_t *base_off, uint64_t n_seq);
/* The sketch so far (may be called again after more pushes). */
int dut_fp_finish(dut_fp_ctx *ctx, dut_fp_result *out);
void dut_fp_destroy(dut_fp_ctx *ctx);
/* Device time of the pushes so far, from events (ms): the uploads, the hash kernel, the sort / reduce / merge;
 * the windows walked and the batches launched.  Any pointer may be NULL. */
int dut_fp_stats(const dut_fp_ctx *ctx, double *h2d_ms, double *hash_ms, double *reduce_ms, uint64_t *n_windows,
                 uint64_t *n_batches);
const char *dut_fp_last_error(const dut_fp_ctx *ctx);

/* `fingerprint <input> [-r reference] [-o output] [-R region]`: the reader by the file's extension
 * (bam -> BAM, fastq / fq / gz -> FASTQ, plain or gzip; cram and gam: not supported), every sequence
 * through one device context, the output file (when output != NULL) in the reference's format with
 * `#region=<region>` as a label only.  digest_out: 65 bytes.  reference is accepted and unused (CRAM).
 * The output file is written last: when only that fails, digest_out and processed_out are filled all the same.
 * DUT_TIMING=1: one line per batch on stderr with the host decode time beside the device time. */
int dut_fp_files(const char *input, const char *reference, const char *output, const dut_fp_options *opt,
                 const char *region, int device_id, char *digest_out, uint64_t *processed_out, char *err, size_t err_len);
/* The file-format check of dut_fp_files alone (no file is opened): 1 BAM, 2 FASTQ, or a negative
 * cl_status with the reference's message in err. */
int dut_fp_input_kind(const char *input, char *err, size_t err_len);

/* ---- host-only entry points (no device) ---- */
/* The shared __host__ __device__ hash code over one sequence of bytes: out[i] = hash of window i
 * (len - k + 1 windows), has_n[i] = 1 where window i holds an 'N' (out[i] is 0 there). */
int dut_fp_kmer_hashes_host(const uint8_t *bytes, uint64_t len, uint32_t k, uint64_t *out, uint8_t *has_n);
/* The same over len bases of BAM 4-bit codes (two per byte, first base in the high nibble). */
int dut_fp_kmer_hashes_host_seq4(const uint8_t *seq4, uint64_t len, uint32_t k, uint64_t *out, uint8_t *has_n);
uint64_t dut_fp_max_hash(uint64_t scaled);
void dut_fp_sha256(const uint8_t *data, size_t len, uint8_t out32[32]);

/* FASTQ reader (4-line records, plain or gzip incl. multi-member): batches of whole records.
 * dut_fastq_next fills *n_seq sequences of at most max_bases bases in total (at least one record);
 * *n_seq = 0 at the end.  The buffers stay valid until the next call.  Reading stops at a record with an
 * empty id or a malformed record (one warning line on stderr), as the reference's reader does. */
typedef struct dut_fastq dut_fastq;
dut_fastq *dut_fastq_open(const char *path, char *err, size_t err_len);
int dut_fastq_next(dut_fastq *f, uint64_t max_bases, uint64_t *n_seq, const uint64_t **base_off, const uint8_t **bytes);
void dut_fastq_close(dut_fastq *f);

/* ---- fingerprint-compare: similarity of many sketches (fingerprint_compare.hip) ----
 * A sketch is ksize, scaled, max_hash = dut_fp_max_hash(scaled) and n entries (hash, count >= 1) with strictly
 * ascending hashes.  A pair (a, b) is compared at cut = min(max_hash_a, max_hash_b) (two different `scaled` values: at
 * the coarser one): every field is taken over the entries with hash <= cut, a prefix of each sketch.  Hashes compare
 * as unsigned 64-bit integers.  Ratios (jaccard = n_common / (n_a + n_b - n_common), containment_a = n_common / n_a,
 * weighted_jaccard = sum_min / (sum_a + sum_b - sum_min)) are derived by the text writer only. */
typedef struct dut_fpc_record {
    uint64_t n_a, n_b;              /* entries of a and of b within the cut                              */
    uint64_t n_common;              /* hashes present in both                                            */
    uint64_t sum_a, sum_b;          /* sums of the counts within the cut                                 */
    uint64_t sum_min;               /* sum over the common hashes of min(count_a, count_b)               */
} dut_fpc_record;

#define DUT_FPC_MAX_PAIRS (1u << 24)
#define DUT_FPC_MAX_TILES 0x7FFFFFFFu

typedef struct dut_fpc_ctx dut_fpc_ctx;

/* A set of sketches resident on the device.  device_id == -1: a host-only context (dut_fpc_add validates and keeps
 * the sizes; compare answers CL_ERR_DEVICE).  stream as for dut_fp_create. */
int dut_fpc_create(int device_id, void *stream, dut_fpc_ctx **out);
void dut_fpc_destroy(dut_fpc_ctx *ctx);
const char *dut_fpc_last_error(const dut_fpc_ctx *ctx);
/* Adds one sketch (n == 0 is valid); *id = 0, 1, 2 ...  CL_ERR_INVALID, with the index in the message and the set
 * unchanged: hashes not strictly ascending, a count of 0, hashes[n - 1] > dut_fp_max_hash(scaled), ksize outside 1..64,
 * null arrays with n > 0. */
int dut_fpc_add(dut_fpc_ctx *ctx, uint32_t ksize, uint64_t scaled, const uint64_t *hashes, const uint32_t *counts,
                uint64_t n, uint32_t *id);
/* n_pairs records in the order given; pairs may repeat, be (i, i), and come in any order.  *out is context-owned, valid
 * until the next compare, add or destroy (NULL for n_pairs == 0, which launches nothing).  CL_ERR_INVALID with a message,
 * the context still usable: an id out of range, null arrays with n_pairs > 0, a null out, a pair of two ksize values (the
 * message names it), more than DUT_FPC_MAX_PAIRS pairs, more than DUT_FPC_MAX_TILES tiles (the message gives the
 * count; the tile count needs the prefix lengths, so cuts below a sketch's max_hash are resolved first -- a small query
 * table and one launch -- and the refusal comes before the pair table, the partials or the records are allocated).  CL_ERR_DEVICE: a host-only context. */
int dut_fpc_compare(dut_fpc_ctx *ctx, const uint32_t *pairs_a, const uint32_t *pairs_b, uint64_t n_pairs,
                    const dut_fpc_record **out);
/* The pairs i < j in row-major order; *n_pairs_out (may be NULL) = n (n - 1) / 2. */
int dut_fpc_compare_all(dut_fpc_ctx *ctx, const dut_fpc_record **out, uint64_t *n_pairs_out);
/* Of the last compare: the device time from events (ms: the tile kernel and the per-pair sum), its tiles and the
 * bytes its pairs span, sum of 12 (n_a + n_b).  Any pointer may be NULL. */
int dut_fpc_stats(const dut_fpc_ctx *ctx, double *kernel_ms, uint64_t *n_tiles, uint64_t *bytes);
/* Merged elements per tile of the device kernel (one workgroup per tile). */
uint32_t dut_fpc_tile(void);

/* ---- host only (no device) ---- */
typedef struct dut_fpc_sketch {
    uint32_t ksize;
    uint64_t scaled;
    uint64_t n;
    const uint64_t *hashes;         /* n, strictly ascending                                            */
    const uint32_t *counts;
    char region[32];                /* `#region=` of the file ("" when absent)                          */
    uint32_t max_frequency;
    int32_t has_max_frequency;
    void *owner;                    /* dut_fp_file_read: what dut_fp_file_free releases                 */
} dut_fpc_sketch;

/* The same records by a plain two-pointer merge (csrc/fp_compare.h) on DUT_THREADS threads: the yardstick.  The
 * sketches are validated as by dut_fpc_add; the refusals are those of dut_fpc_compare, the message in err. */
int dut_fpc_compare_host(const dut_fpc_sketch *sketches, uint64_t n_sketches, const uint32_t *pairs_a,
                         const uint32_t *pairs_b, uint64_t n_pairs, dut_fpc_record *out, char *err, size_t err_len);
/* Reads a file `fingerprint -o` (or the reference) wrote: leading `#key=value` lines (ksize and scaled required,
 * region and max_frequency kept, other keys ignored), then `hash\tcount` in decimal; CR LF accepted; no entry lines:
 * an empty sketch.  Refused as "<path>:<line>: <what>": a malformed or overflowing number, a count of 0, hashes not
 * strictly ascending, a hash above max_hash(scaled), a missing key (line = the first entry line). */
int dut_fp_file_read(const char *path, dut_fpc_sketch *out, char *err, size_t err_len);
void dut_fp_file_free(dut_fpc_sketch *sketch);
/* The text form (README "fingerprint-compare"): `##sketches=`, `##pairs=`, `##ksize=`, the `#a b scaled ...` header, one
 * line per pair with names[pairs_a[p]] and names[pairs_b[p]]; ratios %.6f, NA where the denominator is 0.
 * has_min_jaccard: lines with jaccard < min_jaccard (or NA) are left out; `##pairs=` stays n_pairs. */
int dut_fpc_write(FILE *f, const char *const *names, uint64_t n_sketches, uint32_t ksize, const uint32_t *pairs_a,
                  const uint32_t *pairs_b, const uint64_t *pair_scaled, const dut_fpc_record *records, uint64_t n_pairs,
                  double min_jaccard, int has_min_jaccard);
/* The square Jaccard matrix from the records of the pairs i < j in row-major order: `#name` and the names, then one
 * row per sketch; the diagonal is 1.000000, NA for a sketch of no entries (n_entries[i] == 0). */
int dut_fpc_write_matrix(FILE *f, const char *const *names, const uint64_t *n_entries, uint64_t n_sketches,
                         const dut_fpc_record *records);

typedef struct dut_fpc_file_options {
    const char *query;              /* NULL: all pairs i < j of paths; else this file against each of paths   */
    double min_jaccard;
    int32_t has_min_jaccard;
} dut_fpc_file_options;
/* `fingerprint-compare`: read, compare on the device, write out_path (and matrix_path when not NULL; not with a query).
 * Fewer than two sketches in all, a matrix with a query: CL_ERR_INVALID.  Two files of different max_frequency: one
 * warning line on stderr.  Mixed ksize and unreadable or malformed files: CL_ERR_INVALID with the file in err. */
int dut_fingerprint_compare_files(const char *const *paths, uint64_t n, const dut_fpc_file_options *options,
                                  const char *out_path, const char *matrix_path, int device_id, char *err, size_t err_len);

#ifdef __cplusplus
}
#endif
#endif /* DUT_FINGERPRINT_H */
