// kernels.hip.h -- what the gfx950 (MI355X / CDNA4) kernels of the callable-loci engine share: the constants, the records
// that pass between kernels and host, the wave primitives, and the two kernels behind the pileup.
//
// Data flow of one contig (all arrays resident in HBM, layouts in DESIGN.md section 3):
//
//   (host, at upload: per window of T reference positions the [lo,hi) range of candidates that can touch it -- an
//                    index of the resident layout, like the offsets; WinMeta below)
//   (host, at upload, in the one walk over every CIGAR that validates a tile: every read's end, and for reads of
//                    more than kLongOps operations a (reference, query) checkpoint before every 64th operation, where
//                    the host's later walks enter such a read)
//   a pileup kernel  one workgroup per window: the three per-position counters of
//                    process_position (mod.rs:17-42) are built in LDS (never in HBM), classified
//                    (callable_profiler.rs:100-116) and reduced to the window's run list (the
//                    positions inside the window where the state changes) and its totals.  Two kernels, which share
//                    nothing but what is in this file:
//                      k_pileup_rows  (pileup_rows.hip.h)   the pass-bit form, the product
//                      k_pileup       (pileup_bytes.hip.h)  the byte forms of rounds 1-3 (DUT_QUAL_FORM=bytes), kept as
//                                                           they were so that their measurements stay reproducible
//   k_fin_windows    run counts per window (inner starts + the seam with the previous window) ->
//                    exclusive offsets inside blocks of kFinBlock windows
//   k_rle_write      run lists -> (start,end,state) intervals (callable_profiler.rs:122-155), one wave
//                    per window; its last workgroup reduces the partials to the contig summary
//
// Integer / byte work throughout: HBM-bound, no MFMA.  Wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "engine_limits.h"

namespace clk {

constexpr int kBlock = 256;          // threads per workgroup (4 waves) of k_pileup and k_rle_write
constexpr int kQualPad = 32;         // bytes of padding in front of / behind the quality array
constexpr uint32_t kLutSize = 65536; // low-MAPQ threshold table entries (raw depth 0..65535)
// (kLongOps, kWideSpan, kHeadSpanMax and the kErr* / kNeed* bits: engine_limits.h, shared with the host's tile walk)

// per-window output of a pileup kernel (k_pileup_rows or k_pileup)
struct WinPartial {
    unsigned long long cnt[6];       // state counts
    unsigned long long n_cov;        // positions with raw_depth > 0
    unsigned long long sum_qc;       // -> quality_bases
    unsigned long long sum_q;        // -> summed_baseq
    unsigned long long sum_reflen;   // reads that START in this window: sum of reference spans (-> summed_coverage) ...
    unsigned long long sum_mapq_reflen;   // ... and of mapq * span over those with mapq >= min (-> summed_mapq)
    uint32_t n_inner;                // run boundaries strictly inside the window
    uint32_t max_raw;
};

// mirrors cl_contig_summary (include/callable_loci.h) + engine-private tail
struct DevSummary {
    unsigned long long state_counts[6];
    unsigned long long n_covered_bases;
    unsigned long long summed_coverage;
    unsigned long long summed_baseq;
    unsigned long long summed_mapq;
    unsigned long long quality_bases;
    unsigned long long extent;
    unsigned long long max_raw_depth;
    unsigned long long n_intervals;
    // private
    unsigned long long max_end;
    unsigned long long err;
};

struct Interval { uint32_t start, end, state; };

// 16 bytes at any byte address (compiles to one unaligned dwordx4 load): k_pileup's quality bytes, the site engine's CIGAR words
struct __attribute__((packed, aligned(1))) Q16 { uint32_t w[4]; };

__device__ __forceinline__ bool op_match(uint32_t op) { return op == 0u || op == 7u || op == 8u; }
__device__ __forceinline__ bool op_del(uint32_t op) { return op == 2u || op == 3u; }
__device__ __forceinline__ bool op_ins(uint32_t op) { return op == 1u || op == 4u; }

// ---------------------------------------------------------------------------------------------
// wave / block reductions and scans (wave64)
// ---------------------------------------------------------------------------------------------
// Inclusive prefix sum over the 64 lanes with DPP row shifts / row broadcasts (VALU only; __shfl_up
// compiles to ds_bpermute_b32, an LDS-pipe instruction with far higher latency).
//   row_shr:1,2,4,8 (0x111..0x118, zero fill) scan each row of 16 lanes,
//   row_bcast:15 (0x142, rows 1 and 3) adds the previous row's total,
//   row_bcast:31 (0x143, rows 2 and 3) adds the total of lanes 0..31.
__device__ __forceinline__ uint32_t dpp_incl_scan_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}
// inclusive prefix sum within each row of 16 lanes (the first four steps of the above)
__device__ __forceinline__ uint32_t dpp_row_incl_scan_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    return v;
}
// the maximum over the wave, in every lane (same DPP pattern; the zero fill is the identity of an unsigned max)
__device__ __forceinline__ uint32_t dpp_wave_max_u32(uint32_t v)
{
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); v = t > v ? t : v;
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// the sum over the wave, in every lane (lane 63 of the scan, read through an SGPR)
__device__ __forceinline__ uint32_t dpp_wave_sum_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)dpp_incl_scan_u32(v), 63);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return dpp_wave_max_u32(v); }
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v)
{
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// 64-bit sum over the wave, in every lane: three exact 32-bit DPP sums over 24/24/16-bit limbs
// (64 lanes x 2^24 < 2^32), instead of twelve ds_bpermute round trips
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
    const unsigned long long a = dpp_wave_sum_u32((uint32_t)v & 0xFFFFFFu);
    const unsigned long long b = dpp_wave_sum_u32((uint32_t)(v >> 24) & 0xFFFFFFu);
    const unsigned long long c = dpp_wave_sum_u32((uint32_t)(v >> 48));
    return a + (b << 24) + (c << 48);
}

// What a pileup kernel (either one) needs to start on a window: one 32-byte record, one scalar load.  The candidate reads of a window --
// reads [lo, hi) with pos < W + T and pos + span_n > W (span_n: the longest ordinary span), and the wide reads (span >
// kWideSpan) that start before them -- depend on the resident reads and the extent only: the host builds the records at
// upload (callable_loci.hip: host_window_bounds), flags windows whose candidates' quality bytes do not fit 32-bit
// offsets (kErrRange) and windows with more than 32 767 candidates (kNeedDeep: the 32-bit counter form).
struct __attribute__((aligned(32))) WinMeta {
    uint32_t lo, hi;                   // ordinary candidates: reads [lo, hi)
    uint32_t wlo, wn;                  // wide candidates: wide_idx[wlo .. wlo+wn)
    unsigned long long q0;             // byte forms: qual_off of the window's first candidate read; pass-bit form: the
                                       // heights of its eight segments, a byte each (0: all rn; pileup_rows.hip.h: row_lane)
    uint32_t rlo, rn;                  // run-table form: the window's entries are runtab[rlo .. rlo + rn);
                                       // pass-bit form: its units start at rows[8 rlo], rn = those of its highest segment
};

// ---------------------------------------------------------------------------------------------
// k_fin_windows / fin_summary: exclusive scan of the run starts per window inside blocks of kFinBlock
// windows (inner boundaries + the seam with the previous window) and reduction of the window
// partials to the contig summary (fin_summary runs as the last workgroup of k_rle_write).
// ---------------------------------------------------------------------------------------------
constexpr int kFinBlock = 1024;

struct FinPartial {
    unsigned long long acc[11];      // cnt[6], n_cov, sum_qc, sum_q, sum_reflen, sum_mapq_reflen
    uint32_t n_runs;
    uint32_t max_raw;
};

__global__ __launch_bounds__(kFinBlock) void k_fin_windows(const WinPartial *__restrict__ winpart,
                                                            const uint8_t *__restrict__ first_state,
                                                            const uint8_t *__restrict__ last_state, uint32_t T,
                                                            uint32_t n_win, uint32_t extent,
                                                            uint32_t *__restrict__ win_off,
                                                            FinPartial *__restrict__ fin)
{
    __shared__ uint32_t s_w[kFinBlock / 64], s_m[kFinBlock / 64];
    __shared__ unsigned long long s_red[11][kFinBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t w = blockIdx.x * kFinBlock + tid;
    unsigned long long acc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t c = 0, maxraw = 0;
    if (w < n_win) {
        const WinPartial wp = winpart[w];
        c = wp.n_inner;
        const uint32_t p = w * T;
        if (p < extent) c += (w == 0) ? 1u : (first_state[w] != last_state[w - 1] ? 1u : 0u);
        for (int i = 0; i < 6; ++i) acc[i] = wp.cnt[i];
        acc[6] = wp.n_cov; acc[7] = wp.sum_qc; acc[8] = wp.sum_q;
        acc[9] = wp.sum_reflen; acc[10] = wp.sum_mapq_reflen;
        maxraw = wp.max_raw;
    }
    const uint32_t inc = dpp_incl_scan_u32(c);
    if (lane == 63) s_w[wv] = inc;
#pragma unroll
    for (int i = 0; i < 11; ++i) {
        const unsigned long long v = wave_sum_u64(acc[i]);
        if (lane == 0) s_red[i][wv] = v;
    }
    maxraw = wave_max_u32(maxraw);
    if (lane == 0) s_m[wv] = maxraw;
    __syncthreads();
    uint32_t off = inc - c;
    for (int i = 0; i < wv; ++i) off += s_w[i];
    if (w < n_win) win_off[w] = off;                 // relative to this block's first window
    if (tid == 0) {
        FinPartial fp;
        fp.n_runs = 0; fp.max_raw = 0;
        for (int j = 0; j < kFinBlock / 64; ++j) { fp.n_runs += s_w[j]; fp.max_raw = s_m[j] > fp.max_raw ? s_m[j] : fp.max_raw; }
        for (int i = 0; i < 11; ++i) { unsigned long long v = 0; for (int j = 0; j < kFinBlock / 64; ++j) v += s_red[i][j]; fp.acc[i] = v; }
        fin[blockIdx.x] = fp;
    }
}

// The contig summary: reduction of the per-block window partials.  Run by
// one workgroup of kBlock threads (the extra, last workgroup of k_rle_write).
__device__ __forceinline__ void fin_summary(const FinPartial *__restrict__ fin, uint32_t n_fin,
                                            uint32_t extent, uint32_t *__restrict__ err_flag,
                                            DevSummary *__restrict__ out, unsigned long long host_sum_q,
                                            unsigned long long host_sum_cov, unsigned long long host_sum_mapq)
{
    __shared__ unsigned long long s_red[12][kBlock / 64];
    __shared__ uint32_t s_u[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // [11]: number of runs
    uint32_t maxraw = 0;
    for (uint32_t b = tid; b < n_fin; b += kBlock) {
        const FinPartial fp = fin[b];
        acc[11] += fp.n_runs;
        for (int i = 0; i < 11; ++i) acc[i] += fp.acc[i];        // [9], [10]: over the reads each window owns
        maxraw = fp.max_raw > maxraw ? fp.max_raw : maxraw;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const unsigned long long v = wave_sum_u64(acc[i]);
        if (lane == 0) s_red[i][wv] = v;
    }
    maxraw = wave_max_u32(maxraw);
    if (lane == 0) s_u[wv] = maxraw;
    __syncthreads();
    if (tid == 0) {
        unsigned long long tot[12];
        for (int i = 0; i < 12; ++i) { tot[i] = 0; for (int j = 0; j < kBlock / 64; ++j) tot[i] += s_red[i][j]; }
        uint32_t mr = 0;
        for (int j = 0; j < kBlock / 64; ++j) mr = s_u[j] > mr ? s_u[j] : mr;
        for (int i = 0; i < 6; ++i) out->state_counts[i] = tot[i];
        out->n_covered_bases = tot[6];
        out->quality_bases = tot[7];
        // (pass-bit form: the kernels see bits, the sum of the passing qualities comes from the host's walk over the bytes)
        out->summed_baseq = tot[8] + host_sum_q;
        // (pass-bit form: so do the reads' reference spans and mapq x span, contig_profiler.rs:74, 79-82)
        out->summed_coverage = tot[9] + host_sum_cov;
        out->summed_mapq = tot[10] + host_sum_mapq;
        out->extent = extent;
        out->max_raw_depth = mr;
        out->n_intervals = tot[11];
        out->max_end = 0;                    // read ends come from the host's walk (cl_push_reads)
        out->err = err_flag[0];
        // every kernel of the run is done with the flags: clear them for the next run (saves a memset launch)
        err_flag[0] = 0; err_flag[1] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// k_rle_write: one wave per window turns the window's run list into intervals.  The lane that writes
// the start of run i also closes run i-1.  The extra last workgroup computes the contig summary.
// ---------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(kBlock) void k_rle_write(const uint16_t *__restrict__ runs,
                                                       const uint8_t *__restrict__ first_state,
                                                       const uint8_t *__restrict__ last_state,
                                                       const WinPartial *__restrict__ winpart,
                                                       const uint32_t *__restrict__ win_off,
                                                       const FinPartial *__restrict__ fin, uint32_t n_fin,
                                                       uint32_t *__restrict__ err_flag,
                                                       DevSummary *__restrict__ summary,
                                                       uint32_t n_win, uint32_t extent,
                                                       Interval *__restrict__ iv, uint32_t iv_cap,
                                                       unsigned long long host_sum_q, unsigned long long host_sum_cov,
                                                       unsigned long long host_sum_mapq)
{
    if (blockIdx.x == gridDim.x - 1) {                     // the extra workgroup: the contig summary
        fin_summary(fin, n_fin, extent, err_flag, summary, host_sum_q, host_sum_cov, host_sum_mapq);
        return;
    }
    // one wave per window: its seam run (if the first state differs from the previous window's last)
    // and the run starts of its list; a run start also closes the run before it
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (w >= n_win) return;
    const uint32_t W = w * (uint32_t)T;
    if (W >= extent) return;
    // (everything this wave needs is requested at once: the first 64 entries of the run list too -- the list has T slots,
    // what lies behind its n_inner entries is never used -- so that one memory round trip stands between launch and stores)
    const uint16_t *rl = runs + (size_t)w * T;
    const uint32_t e0 = rl[lane];
    const uint32_t n_inner = winpart[w].n_inner;
    const uint32_t seam = (w == 0 || first_state[w] != last_state[w - 1]) ? 1u : 0u;
    // runs before this window: those of the earlier k_fin_windows blocks + the offset inside its block
    uint32_t before = 0;
    for (uint32_t b = lane; b < w / kFinBlock; b += 64u) before += fin[b].n_runs;
    const uint32_t idx0 = dpp_wave_sum_u32(before) + win_off[w];
    if (lane == 0 && seam) {
        if (idx0 < iv_cap) { iv[idx0].start = W; iv[idx0].state = first_state[w]; }
        if (idx0 > 0 && idx0 - 1 < iv_cap) iv[idx0 - 1].end = W;
    }
    for (uint32_t i = lane; i < n_inner; i += 64u) {
        const uint32_t e = i < 64u ? e0 : (uint32_t)rl[i];
        const uint32_t idx = idx0 + seam + i, start = W + (e & 0xFFFu);
        if (idx < iv_cap) { iv[idx].start = start; iv[idx].state = e >> 12; }
        if (idx > 0 && idx - 1 < iv_cap) iv[idx - 1].end = start;
    }
    if (w == n_win - 1 && lane == 0) {                     // the last run ends where classification ends
        const uint32_t last = idx0 + seam + n_inner;
        if (last > 0 && last - 1 < iv_cap) iv[last - 1].end = extent;
    }
}

} // namespace clk
