// fp_readers_host.cpp -- the two readers of the `fingerprint` path as a program of their own, for the sanitizers
// (tests/test_fingerprint_host.py): walks dut_fastq_next or dut_bam_next_seqs to the end of a file and prints what it read.
//
//   fp_readers_host <path> fastq|bam <max_bases>
//
// stdout: "<records> <bases> <checksum> <batches>", the checksum over the decoded bases b_i (i counted over the whole file)
// and the records' lengths len_r:  sum (i + 1) * (b_i + 1)  +  sum (r + 1) * len_r * 2^32   (mod 2^64).
#include "../../include/dut_bam.h"
#include "../../include/dut_fingerprint.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: fp_readers_host <path> fastq|bam <max_bases>\n"); return 2; }
    const bool bam = strcmp(argv[2], "bam") == 0;
    if (!bam && strcmp(argv[2], "fastq") != 0) { fprintf(stderr, "kind must be fastq or bam\n"); return 2; }
    const uint64_t cap = strtoull(argv[3], nullptr, 10);
    char err[512] = {0};
    dut_bam *b = bam ? dut_bam_open(argv[1], err, sizeof(err)) : nullptr;
    dut_fastq *f = bam ? nullptr : dut_fastq_open(argv[1], err, sizeof(err));
    if (!b && !f) { fprintf(stderr, "cannot open %s: %s\n", argv[1], err); return 1; }
    static const char letters[] = "=ACMGRSVTWYHKDBN";
    uint64_t records = 0, bases = 0, sum = 0, batches = 0;
    int rc = 0;
    for (;;) {
        uint64_t n = 0;
        const uint64_t *off = nullptr;
        const uint8_t *d = nullptr;
        rc = bam ? dut_bam_next_seqs(b, cap, &n, &off, &d) : dut_fastq_next(f, cap, &n, &off, &d);
        if (rc != 0) { fprintf(stderr, "read failed (%d): %s\n", rc, bam ? dut_bam_error(b) : ""); break; }
        if (n == 0) break;
        batches += 1;
        if (off[0] != 0) { fprintf(stderr, "a batch that does not begin at offset 0\n"); rc = 1; break; }
        if (n > 1 && off[n] > cap) { fprintf(stderr, "a batch of several records beyond max_bases\n"); rc = 1; break; }
        for (uint64_t r = 0; r < n; ++r) {
            if (off[r + 1] < off[r]) { fprintf(stderr, "offsets not ascending\n"); rc = 1; break; }
            for (uint64_t i = off[r]; i < off[r + 1]; ++i) {
                const uint8_t c = bam ? (uint8_t)letters[(d[i >> 1] >> ((~i & 1u) * 4u)) & 15u] : d[i];
                bases += 1;
                sum += bases * ((uint64_t)c + 1);
            }
            records += 1;
            sum += (records * (off[r + 1] - off[r])) << 32;
        }
        if (rc) break;
    }
    if (b) dut_bam_close(b);
    if (f) dut_fastq_close(f);
    if (rc) return 1;
    printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", records, bases, sum, batches);
    return 0;
}
