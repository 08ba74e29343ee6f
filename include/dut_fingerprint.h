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

#ifdef __cplusplus
}
#endif
#endif /* DUT_FINGERPRINT_H */
