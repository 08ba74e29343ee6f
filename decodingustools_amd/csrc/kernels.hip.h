// kernels.hip.h -- what the gfx950 (MI355X / CDNA4) kernels of the callable-loci engine share: the constants, the records
// that pass between kernels and host, the wave primitives, and the one kernel behind the pileup.
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
//                    positions inside the window where the state changes), its totals and its packed word
//                    (win_word below).  The workgroup of window 0 also writes the start values of the contig summary.
//                    Two kernels, which share nothing but what is in this file:
//                      k_pileup_rows  (pileup_rows.hip.h)   the pass-bit form, the product
//                      k_pileup       (pileup_bytes.hip.h)  the byte forms of rounds 1-3 (DUT_QUAL_FORM=bytes), kept as
//                                                           they were so that their measurements stay reproducible
//   k_tail           one launch: a workgroup owns a chunk of consecutive windows, sums the run counts of every window
//                    before its chunk from the packed words itself (no workgroup waits for another) and turns its windows'
//                    run lists into (start,end,state) intervals (callable_profiler.rs:122-155), one wave per window; a
//                    few workgroups in front of the grid do nothing but add the windows' totals to the contig summary
//                    with atomics
//
// Integer / byte work throughout: HBM-bound, no MFMA.  Wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "engine_limits.h"

namespace clk {

constexpr int kBlock = 256;          // threads per workgroup (4 waves) of k_pileup
constexpr int kQualPad = 32;         // bytes of padding in front of / behind the quality array
constexpr uint32_t kLutSize = 65536; // low-MAPQ threshold table entries (raw depth 0..65535)
// (kLongOps, kWideSpan, kHeadSpanMax and the kErr* / kNeed* bits: engine_limits.h, shared with the host's tile walk)

// per-window output of k_pileup (the byte forms)
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

// per-window output of k_pileup_rows: the same totals as the wave's reductions leave them, 32 bytes that one lane stores
// with two 16-byte stores.  A state count and n_cov are at most T = 2 048 (16-bit halves, no carry between them); the
// pass-bit form has no sum_q / sum_reflen / sum_mapq_reflen of a window (the host's walk adds them up) and keeps n_inner
// in the window's packed word alone (win_word below).  The tail unpacks (tail_summary_rows).
struct __attribute__((aligned(16))) WinRecord {
    uint32_t cnt01, cnt23, cnt45;    // state counts: cnt[2 k] | cnt[2 k + 1] << 16
    uint32_t cov_qc;                 // n_cov | sum_qc << 12 with 8 counter planes (255 x 2 048 < 2^19), n_cov alone with more
    uint32_t qc_lo, qc_hi;           // sum_qc with 16 or 32 planes (zero with 8): quality_bases = (cov_qc >> 12) + this
    uint32_t max_raw;
    uint32_t pad;
};
static_assert(sizeof(WinRecord) == 32 && alignof(WinRecord) == 16 && offsetof(WinRecord, cnt01) == 0 && offsetof(WinRecord, cnt23) == 4 &&
              offsetof(WinRecord, cnt45) == 8 && offsetof(WinRecord, cov_qc) == 12 && offsetof(WinRecord, qc_lo) == 16 &&
              offsetof(WinRecord, qc_hi) == 20 && offsetof(WinRecord, max_raw) == 24, "WinRecord as two 16-byte words");

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
// The record is sixteen 8-byte words: the pileup's workgroup of window 0 copies the run's start values into it, a lane a
// word (summary_start below), and k_tail adds to the words by their position
constexpr int kSummaryWords = 16;
static_assert(sizeof(DevSummary) == kSummaryWords * 8 && offsetof(DevSummary, n_covered_bases) == 48 && offsetof(DevSummary, summed_coverage) == 56 &&
              offsetof(DevSummary, summed_baseq) == 64 && offsetof(DevSummary, summed_mapq) == 72 && offsetof(DevSummary, quality_bases) == 80 &&
              offsetof(DevSummary, max_raw_depth) == 96 && offsetof(DevSummary, n_intervals) == 104, "DevSummary as sixteen 8-byte words");

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
// the same maximum as an inclusive scan: lane 63 holds the wave's, and may store it without a trip through an SGPR
__device__ __forceinline__ uint32_t dpp_incl_max_u32(uint32_t v)
{
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); v = t > v ? t : v;
    return v;
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
// What the pileup leaves per window for the tail, beside the run list and the WinPartial or WinRecord: one packed word,
//   n_inner | first_state << 16 | last_state << 24      (n_inner <= T - 1 = 2047; a state is 3 bits)
// Everything the tail needs to place a window's intervals -- how many runs every window before it starts -- follows from
// these words alone: c(v) = n_inner(v) + seam(v), seam(0) = 1, seam(v) = first(v) != last(v - 1).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t win_word(uint32_t n_inner, uint32_t first, uint32_t last) { return n_inner | (first << 16) | (last << 24); }
__device__ __forceinline__ uint32_t ww_inner(uint32_t w) { return w & 0xFFFFu; }
__device__ __forceinline__ uint32_t ww_first(uint32_t w) { return (w >> 16) & 0xFFu; }
__device__ __forceinline__ uint32_t ww_last(uint32_t w) { return w >> 24; }
// runs that start in window v: `word` its packed word, `prev` that of window v - 1 (not looked at for v == 0)
__device__ __forceinline__ uint32_t ww_runs(uint32_t word, uint32_t prev, uint32_t v)
{
    return ww_inner(word) + ((v == 0u || ww_first(word) != ww_last(prev)) ? 1u : 0u);
}

// The start values of a run's contig summary (callable_loci.hip fills the 16-word record at upload: zero counts, the
// host's separable sums, the extent): copied into the summary by the pileup's workgroup of window 0, a lane a word, so
// that k_tail's atomics find them -- stream order stands between the two kernels.
__device__ __forceinline__ void summary_start(unsigned long long *__restrict__ summary, const unsigned long long *__restrict__ start, uint32_t tid)
{
    if (tid < (uint32_t)kSummaryWords) summary[tid] = start[tid];
}

// ---------------------------------------------------------------------------------------------
// k_tail: everything behind the pileup, one launch.  Workgroup c owns the windows [c wpc, (c + 1) wpc) of the contig
// (wpc: a multiple of 16, at most kTailMaxWpc, chosen by the host so that there are at most kTailMaxChunks workgroups:
// callable_loci.hip, launch_tail).  No workgroup waits for another one: what a workgroup needs of the windows before its
// own -- the number of runs that start there -- it sums itself from their packed words (4 bytes a window, from L2; bounded
// by the cap on the workgroups: at most about 1 KB per window of the contig).  There is no spin loop, no look-back, no
// ticket, no fence; the contig summary is accumulated, by workgroups that do nothing else, with relaxed agent-scope
// atomics whose results nobody reads (integer sums and a maximum: the same bytes in whatever order).
//
// The first n_sum workgroups of the grid do nothing but the summary (tail_summary below), the others are the chunks.
// A chunk, in this order, every load of step 1 requested before anything waits:
//   1. loads: the own chunk's packed words (thread t: the four words of windows v0 + 4t .., and the word before them),
//      the first 64 run-list entries of the first kTailAhead windows the wave will write, and the packed words of
//      windows [0, v0) in trips of 4 096 windows
//   2. runs_before = the block's sum of c(v) over v < v0 (DPP per wave, 16 values through LDS); the exclusive scan of
//      c over the own chunk and the chunk's words go into LDS; ONE __syncthreads()
//   3. wave k writes the intervals of windows v0 + k, v0 + k + 16, ...: the seam run, the inner runs; a run start also
//      closes the run before it, across window and chunk borders, by index alone; every store under idx < iv_cap
//   4. the last chunk knows the number of runs (those before it + its own) and stores it: no atomic
// ---------------------------------------------------------------------------------------------
constexpr int kTailBlock = 1024;               // 16 waves
constexpr uint32_t kTailMinWpc = 64;           // windows per workgroup while the contig needs no more than kTailMaxChunks of them
constexpr uint32_t kTailMaxChunks = 512;       // (DUT_TAIL_CHUNKS replaces it: a test hook)
constexpr uint32_t kTailMaxWpc = 4 * kTailBlock;   // a thread holds four windows of the own chunk; 2^21 windows / 512 = 4 096
constexpr int kTailAhead = 4;                  // windows per wave whose run lists are requested together (wpc = 64: all of them)
constexpr uint32_t kTailSumWindows = 1024;     // windows per summary workgroup (callable_loci.hip: launch_tail), while there
constexpr uint32_t kTailMaxSum = 64;           // are no more than this many of them

// The contig summary.  Every atomic on the record goes to one 128-byte line and the memory system takes them one after the
// other (measured: about 3 ns each, profiles/r24_tail_chunks.json -- 13 from every chunk of 64 windows cost more than the
// launch they saved), so the windows' partials are summed by a few workgroups that do nothing else: workgroup s of n_sum
// takes the windows [s wps, (s + 1) wps), thread t < 768 the 8-byte words t, t + 768, ... of their WinPartials (its
// word of the twelve is t mod 12 throughout: 768 = 64 x 12; coalesced), the 768 sums go through LDS to waves 0..11, a
// word each, and 12 atomics per workgroup go to the summary -- a few hundred per contig.  Workgroup 0's thread 0 hands
// err_flag[0] to the summary and clears the flags for the next run: it is their only reader behind the pileup.
__device__ __forceinline__ void tail_flags(uint32_t *__restrict__ err_flag, DevSummary *__restrict__ summary)
{
    summary->err = err_flag[0];
    // every kernel of the run is done with the flags: clear them for the next run (saves a memset launch)
    err_flag[0] = 0; err_flag[1] = 0;
}
__device__ __forceinline__ void tail_summary(const WinPartial *__restrict__ winpart, uint32_t *__restrict__ err_flag,
                                             DevSummary *__restrict__ summary, uint32_t n_win, uint32_t wps)
{
    __shared__ unsigned long long s_acc[768];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t w0 = blockIdx.x * wps;
    const uint32_t nw = w0 >= n_win ? 0u : (n_win - w0 < wps ? n_win - w0 : wps);
    const unsigned long long *wpw = reinterpret_cast<const unsigned long long *>(winpart + (nw ? w0 : 0u));
    if (tid < 768u) {
        // (word 11 is {n_inner, max_raw}: the maximum of its high half is wanted; the others are 64-bit totals)
        const bool is_max = tid % 12u == 11u;
        unsigned long long acc = 0;
#pragma unroll 4
        for (uint32_t i = tid; i < nw * 12u; i += 768u) {
            const unsigned long long x = wpw[i];
            acc = is_max ? (x >> 32 > acc ? x >> 32 : acc) : acc + x;
        }
        s_acc[tid] = acc;
    }
    __syncthreads();
    unsigned long long *sw = reinterpret_cast<unsigned long long *>(summary);
    if (wv < 12u) {
        const unsigned long long x = s_acc[wv + 12u * lane];
        if (wv < 11u) {
            // WinPartial words 0..10 are cnt[6], n_cov, sum_qc, sum_q, sum_reflen, sum_mapq_reflen; their places in the
            // summary: state_counts[6], n_covered_bases (6), quality_bases (10), summed_baseq (8), summed_coverage (7),
            // summed_mapq (9)
            const uint32_t dst = wv < 7u ? wv : (wv == 7u ? 10u : (wv == 8u ? 8u : (wv == 9u ? 7u : 9u)));
            const unsigned long long tot = wave_sum_u64(x);
            if (lane == 0u && tot) (void)__hip_atomic_fetch_add(sw + dst, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const unsigned long long m = wave_max_u32((uint32_t)x);
            if (lane == 0u && m) (void)__hip_atomic_fetch_max(sw + 12, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (blockIdx.x == 0u && tid == 0u) tail_flags(err_flag, summary);
}
// The same for the records of k_pileup_rows (WinRecord above: 32 bytes a window, a third of the bytes).  Thread t takes the
// windows t, t + 1024, ... of the workgroup's share, both 16-byte words of a record, and unpacks them into sums of its
// own: a count is at most T a window and a thread has at most 32 windows (2^21 windows in kTailMaxSum workgroups of
// 1 024 threads), so 32 bits hold a thread's, a wave's and the workgroup's count; sum_qc is kept in 64.  Then one DPP
// reduction per total and wave, 16 values per total through LDS, and thread k adds total k to the summary: the same
// words as tail_summary's (state_counts, n_covered_bases, quality_bases, max_raw_depth), again only where there is something to add.
__device__ __forceinline__ void tail_summary_rows(const WinRecord *__restrict__ rec, uint32_t *__restrict__ err_flag,
                                                  DevSummary *__restrict__ summary, uint32_t n_win, uint32_t wps)
{
    constexpr int kWaves = kTailBlock / 64, kTot = 9;      // cnt[6], n_cov, sum_qc, max_raw
    __shared__ unsigned long long s_tot[kWaves][kTot];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t w0 = blockIdx.x * wps;
    const uint32_t nw = w0 >= n_win ? 0u : (n_win - w0 < wps ? n_win - w0 : wps);
    uint32_t f[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u}, mx = 0u;
    unsigned long long qc = 0;
    for (uint32_t i = tid; i < nw; i += (uint32_t)kTailBlock) {
        const uint4 *r = reinterpret_cast<const uint4 *>(rec + w0 + i);
        const uint4 x = r[0], y = r[1];
        f[0] += x.x & 0xFFFFu; f[1] += x.x >> 16; f[2] += x.y & 0xFFFFu; f[3] += x.y >> 16; f[4] += x.z & 0xFFFFu; f[5] += x.z >> 16;
        f[6] += x.w & 0xFFFu;
        qc += (unsigned long long)(x.w >> 12) + ((unsigned long long)y.x | ((unsigned long long)y.y << 32));
        mx = y.z > mx ? y.z : mx;
    }
    unsigned long long t[kTot];
#pragma unroll
    for (int k = 0; k < 7; ++k) t[k] = dpp_wave_sum_u32(f[k]);
    t[7] = wave_sum_u64(qc);
    t[8] = dpp_wave_max_u32(mx);
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < kTot; ++k) s_tot[wv][k] = t[k];
    }
    __syncthreads();
    if (tid < (uint32_t)kTot) {
        unsigned long long tot = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) { const unsigned long long v = s_tot[k][tid]; tot = tid == 8u ? (v > tot ? v : tot) : tot + v; }
        unsigned long long *sw = reinterpret_cast<unsigned long long *>(summary);
        // (state_counts[6] and n_covered_bases are words 0..6, quality_bases word 10, max_raw_depth word 12)
        if (tot) {
            if (tid == 8u) (void)__hip_atomic_fetch_max(sw + 12, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else (void)__hip_atomic_fetch_add(sw + (tid == 7u ? 10u : tid), tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (blockIdx.x == 0u && tid == 0u) tail_flags(err_flag, summary);
}

// (8 waves per SIMD, at most 64 vector registers: two workgroups per CU, so that the chunks of a chr21-sized contig --
// 357 and the summary's 23 on 256 CUs -- are resident at once; at one workgroup per CU they ran in two rounds)
// RECORD: the windows' totals are the WinRecords of k_pileup_rows; else the WinPartials of k_pileup (launch_tail chooses).
template <int T, bool RECORD>
__global__ __launch_bounds__(kTailBlock, 8) void k_tail(const uint16_t *__restrict__ runs, const uint32_t *__restrict__ win_words,
                                                      const void *__restrict__ winpart, uint32_t *__restrict__ err_flag,
                                                      DevSummary *__restrict__ summary, uint32_t n_win, uint32_t extent,
                                                      uint32_t wpc, uint32_t n_sum, uint32_t wps, Interval *__restrict__ iv, uint32_t iv_cap)
{
    if (blockIdx.x < n_sum) {
        if constexpr (RECORD) tail_summary_rows(static_cast<const WinRecord *>(winpart), err_flag, summary, n_win, wps);
        else tail_summary(static_cast<const WinPartial *>(winpart), err_flag, summary, n_win, wps);
        return;
    }
    constexpr int kWaves = kTailBlock / 64;
    __shared__ uint32_t s_off[kTailMaxWpc];                // own chunk: runs before window i, relative to its owner thread's wave
    __shared__ uint32_t s_word[kTailMaxWpc + 1];           // own chunk: [i + 1] the word of window v0 + i, [0] that of v0 - 1
    __shared__ uint32_t s_wpre[kWaves], s_wown[kWaves];    // per wave: its share of runs_before, its total of the own chunk
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t v0 = (blockIdx.x - n_sum) * wpc;
    if (v0 >= n_win) return;                               // (the whole workgroup: the grid is n_sum + ceil(n_win / wpc))
    const uint32_t n_own = n_win - v0 < wpc ? n_win - v0 : wpc;
    // c(v) of a window below `lim` (0 beyond it, and for a window that starts at or beyond the extent)
    auto runs_of = [&](uint32_t word, uint32_t prev, uint32_t v, uint32_t lim) -> uint32_t {
        return (v < lim && (unsigned long long)v * (uint32_t)T < extent) ? ww_runs(word, prev, v) : 0u;
    };
    // Four consecutive words and the one before them.  The address is clamped, not the load skipped, so that the loads
    // of a trip are straight code issued back to back; `b` is a multiple of 4 and the array is padded to whole quads
    // (callable_loci.hip: each_extent_buffer), so a quad that holds a window below n_win lies inside it.  What a
    // clamped load returns is never counted: runs_of() looks at the window numbers.
    auto quad_at = [&](uint32_t b, bool ok) -> uint4 { return *reinterpret_cast<const uint4 *>(win_words + (ok ? b : 0u)); };
    auto word_before = [&](uint32_t b, bool ok) -> uint32_t { return win_words[(ok && b > 0u) ? b - 1u : 0u]; };

    // ---- 1. loads ----
    const uint32_t ob = v0 + 4u * tid;                     // the own chunk: this thread's four windows
    const bool own = 4u * tid < n_own;
    const uint4 oq = quad_at(ob, own);
    const uint32_t op = word_before(ob, own);
    uint32_t e0[kTailAhead];                               // run lists: T slots a window, what lies behind its n_inner entries is never used
#pragma unroll
    for (int j = 0; j < kTailAhead; ++j) {
        const uint32_t i = wv + (uint32_t)(kWaves * j);
        e0[j] = runs[(size_t)(v0 + (i < n_own ? i : 0u)) * T + lane];
    }
    // the windows before the chunk: trips of 4 096 windows, two trips requested together (a third would cost the registers of the second workgroup per CU)
    uint32_t pre = 0;
    for (uint32_t t0 = 0; t0 < v0; t0 += 2u * kTailMaxWpc) {
        uint4 q[2];
        uint32_t p[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t b = t0 + (uint32_t)k * kTailMaxWpc + 4u * tid;
            q[k] = quad_at(b, b < v0);
            p[k] = word_before(b, b < v0);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t b = t0 + (uint32_t)k * kTailMaxWpc + 4u * tid;
            pre += runs_of(q[k].x, p[k], b, v0) + runs_of(q[k].y, q[k].x, b + 1u, v0) +
                   runs_of(q[k].z, q[k].y, b + 2u, v0) + runs_of(q[k].w, q[k].z, b + 3u, v0);
        }
    }

    // ---- 2. runs_before, the own chunk's scan ----
    {
        const uint32_t lim = v0 + n_own;
        const uint32_t c0 = runs_of(oq.x, op, ob, lim), c1 = runs_of(oq.y, oq.x, ob + 1u, lim),
                       c2 = runs_of(oq.z, oq.y, ob + 2u, lim), c3 = runs_of(oq.w, oq.z, ob + 3u, lim);
        const uint32_t t = c0 + c1 + c2 + c3;
        const uint32_t inc = dpp_incl_scan_u32(t);
        if (own) {                                         // (4 tid < n_own <= kTailMaxWpc: inside the arrays)
            const uint32_t x = inc - t;
            s_off[4u * tid] = x; s_off[4u * tid + 1u] = x + c0; s_off[4u * tid + 2u] = x + c0 + c1; s_off[4u * tid + 3u] = x + c0 + c1 + c2;
            s_word[4u * tid + 1u] = oq.x; s_word[4u * tid + 2u] = oq.y; s_word[4u * tid + 3u] = oq.z; s_word[4u * tid + 4u] = oq.w;
            if (tid == 0u) s_word[0] = op;
        }
        if (lane == 63u) s_wown[wv] = inc;
        const uint32_t ps = dpp_wave_sum_u32(pre);
        if (lane == 0u) s_wpre[wv] = ps;
    }
    __syncthreads();
    uint32_t before = 0, own_runs = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) { before += s_wpre[k]; own_runs += s_wown[k]; }

    // ---- 3. the intervals: wave wv writes windows v0 + wv, v0 + wv + 16, ... ----
    for (uint32_t j0 = 0; wv + (uint32_t)kWaves * j0 < n_own; j0 += (uint32_t)kTailAhead) {
        if (j0) {                                          // (wpc > 64: the next kTailAhead lists, requested together)
#pragma unroll
            for (int j = 0; j < kTailAhead; ++j) {
                const uint32_t i = wv + (uint32_t)kWaves * (j0 + (uint32_t)j);
                e0[j] = runs[(size_t)(v0 + (i < n_own ? i : 0u)) * T + lane];
            }
        }
        static_assert(kTailAhead == 4, "the select below");
#pragma unroll 1
        for (int j = 0; j < kTailAhead; ++j) {               // (not unrolled: four copies of the body cost the second workgroup per CU)
            const uint32_t i = wv + (uint32_t)kWaves * (j0 + (uint32_t)j);
            if (i >= n_own) break;
            const uint32_t e0j = j == 0 ? e0[0] : (j == 1 ? e0[1] : (j == 2 ? e0[2] : e0[3]));
            const uint32_t w = v0 + i;
            const uint32_t W = w * (uint32_t)T;
            if (W >= extent) continue;
            const uint32_t word = s_word[i + 1u], prev = s_word[i];
            const uint32_t n_inner = ww_inner(word);
            const uint32_t seam = ww_runs(word, prev, w) - n_inner;
            uint32_t idx0 = before + s_off[i];             // + the own chunk's waves below the one whose thread holds window i
            for (uint32_t k = 0; k < (i >> 8); ++k) idx0 += s_wown[k];
            if (lane == 0u && seam) {
                if (idx0 < iv_cap) { iv[idx0].start = W; iv[idx0].state = ww_first(word); }
                if (idx0 > 0u && idx0 - 1u < iv_cap) iv[idx0 - 1u].end = W;
            }
            const uint16_t *rl = runs + (size_t)w * T;
            for (uint32_t r = lane; r < n_inner; r += 64u) {
                const uint32_t e = r < 64u ? e0j : (uint32_t)rl[r];
                const uint32_t idx = idx0 + seam + r, start = W + (e & 0xFFFu);
                if (idx < iv_cap) { iv[idx].start = start; iv[idx].state = e >> 12; }
                if (idx > 0u && idx - 1u < iv_cap) iv[idx - 1u].end = start;
            }
            if (w == n_win - 1u && lane == 0u) {           // the last run ends where classification ends
                const uint32_t last = idx0 + seam + n_inner;
                if (last > 0u && last - 1u < iv_cap) iv[last - 1u].end = extent;
            }
        }
    }

    // ---- 4. the number of runs: the last chunk has it ----
    if (v0 + n_own == n_win && tid == 0u) summary->n_intervals = (unsigned long long)before + own_runs;
}

} // namespace clk
