// site_errors.hip.h -- the error profile of a range of the resident site tile (cl_site_error_profile; a textual part of
// site_engine.hip.h): substitutions by reference base and read base, the same by distance from either end of the read, and
// insertion and deletion events by the same distances.  Every other site kernel reduces per position and forgets where in
// the read a base stood; this one reduces the whole range into one small table keyed by the query index.  The rule per
// read is ep_walk_read (ep_walk.h), written there once.
//
// k_site_error_profile<FILTERED>: a bounded grid of workgroups of kEpBlock threads over the windows of the scan's read index
// (k_site_scan_index, kScanWin).  Workgroup g takes the g-th run of consecutive windows and owns slice g of a buffer of
// 64-bit partial tables.  The reads of a window are dealt to the WAVES; the 64 lanes of a wave take the bases of one M/=/X
// operation side by side (ep_walk_read's lanes), lane 0 the events.  Gates: scan_read_counts, the flag load and the
// pass-bit helper of the filtered scans; bases from seq4, reference bytes as site_scan_reference left them.
//
// The table lives in LDS as 32-bit words, plane by cell: from5[cell][cycle], from3[cell][cycle], then ins5, ins3, del5,
// del3 [cycle], then total[16], n_uncomparable, n_reads, n_ins, n_del -- kEpTail words -- and behind them two 64-bit words,
// ins_bases and del_bases, whose addends have no small bound.  A wave's lanes hold consecutive query indices, so their adds
// of one cell fall on consecutive cycles: consecutive banks, no two lanes on one word.  Only `total` has no cycle to spread
// it: there the wave counts its lanes per cell with a ballot and one lane adds the count.
//
// No 32-bit word can wrap: a read adds at most kScanWin to any one word per window visit (one per position: a base, an
// anchor or a first deleted position), so what a workgroup has added since its last flush is at most reads visited x
// kScanWin.  It visits the reads of a window in pieces of at most flush / kScanWin reads and adds its table into its slice
// (plain loads and stores: nobody else touches the slice) before the visited reads would pass that number; flush is
// 2^32 - 1, or DUT_EP_FLUSH.  k_site_error_profile_sum then adds the slices into the result, word by word.  No global
// atomic anywhere: two calls return identical bytes.
#pragma once

#include "ep_walk.h"

namespace clk {

static_assert(CL_EP_MAX_CYCLES == CL_EP_WALK_MAX_CYCLES, "ep_walk.h knows the largest table of cl_ep_result");

constexpr uint32_t kEpBlock = 1024;          // 16 waves on one table: one workgroup per CU hides its loads behind the other waves'
constexpr uint32_t kEpGroups = 256;          // workgroups of a launch (DUT_EP_GROUPS), each with a slice of 36 C + 22 64-bit words
constexpr uint32_t kEpGroupsMost = 4096;     // the most DUT_EP_GROUPS is taken for: 4 096 slices are 0.3 GB at C = 256
constexpr uint32_t kEpTail = 20;             // total[16], n_uncomparable, n_reads, n_ins, n_del
enum { EP_UNC = 16, EP_READS = 17, EP_INS = 18, EP_DEL = 19 };

// words of the table in LDS (32 bits each) and in a slice or the result (64 bits each: the two 64-bit sums behind them)
__host__ __device__ constexpr uint32_t ep_words32(uint32_t C) { return 36u * C + kEpTail; }
__host__ __device__ constexpr uint32_t ep_words64(uint32_t C) { return ep_words32(C) + 2u; }
__host__ __device__ constexpr size_t ep_lds_bytes(uint32_t C) { return (size_t)ep_words32(C) * 4u + 16u; }
static_assert(ep_words32(1) % 4u == 0u, "the 64-bit words behind the table are aligned for any C");

template <bool FILTERED> struct EpArgs {
    ScanArgs s;                                // the tile, the index, the gates and the reference, as site_scan_fill sets them
    typename ScanForm<FILTERED>::Filter f;
    void *cand;                                // (site_scan_fill's; unused)
    uint32_t n_cycles, n_groups, n_windows;    // windows win0 .. win0 + n_windows - 1 are dealt to n_groups workgroups
    uint32_t piece;                            // most reads between two flushes: flush / kScanWin, at least 1
    unsigned long long *part;                  // n_groups * ep_words64(n_cycles)
};

// what a wave does with the walk of one read: lanes side by side on the bases, lane 0 on the events
template <bool FILTERED> struct EpSink {
    const EpArgs<FILTERED> &ax;
    uint32_t *tab;                             // the table in LDS
    unsigned long long *wide;                  // ins_bases, del_bases
    unsigned long long s0;                     // the read's first base in the numbering of seq4
    uint32_t L, rev, lane, C;

    __device__ __forceinline__ void cycles(uint32_t plane5, uint32_t q) const
    {
        const uint32_t d5 = dut::ep_d5(q, L, rev), d3 = dut::ep_d3(q, L, rev);
        if (d5 < C) atomicAdd(&tab[plane5 + d5], 1u);
        if (d3 < C) atomicAdd(&tab[plane5 + 16u * C + d3], 1u);
    }
    __device__ __forceinline__ void base(uint32_t p, uint32_t q) const
    {
        const unsigned long long bi = s0 + q;
        if (!scan_pass_bit(ax.f, bi)) return;
        const uint32_t cell = dut::ep_cell(scan_base_code(ax.s.seq4, bi), ax.s.refb[p - ax.s.start], rev);
        if (cell < 16u) cycles(cell * C, q);
        // total and n_uncomparable: the lanes of one cell are counted with a ballot and their first lane adds the count
        for (bool done = false; !done;) {
            const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)cell);
            const bool mine = cell == k;
            const unsigned long long m = __ballot(mine);
            if (mine) {
                if (lane == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(&tab[36u * C + k], (uint32_t)__popcll(m));
                done = true;
            }
        }
    }
    __device__ __forceinline__ void event(uint32_t which, uint32_t q, uint32_t l) const         // which: 0 insertion, 1 deletion
    {
        if (!scan_pass_bit(ax.f, s0 + q)) return;
        atomicAdd(&tab[36u * C + EP_INS + which], 1u);
        atomicAdd(&wide[which], (unsigned long long)l);
        const uint32_t d5 = dut::ep_d5(q, L, rev), d3 = dut::ep_d3(q, L, rev);
        if (d5 < C) atomicAdd(&tab[(32u + 2u * which) * C + d5], 1u);
        if (d3 < C) atomicAdd(&tab[(33u + 2u * which) * C + d3], 1u);
    }
    __device__ __forceinline__ void ins(uint32_t, uint32_t q, uint32_t l) const { event(0u, q, l); }
    __device__ __forceinline__ void del(uint32_t, uint32_t q, uint32_t l) const { event(1u, q, l); }
};

template <bool FILTERED>
__global__ __launch_bounds__(kEpBlock) void k_site_error_profile(EpArgs<FILTERED> ax)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_ep[];
    const ScanArgs &a = ax.s;
    const uint32_t C = ax.n_cycles, n32 = ep_words32(C);
    unsigned long long *s_wide = reinterpret_cast<unsigned long long *>(s_ep + n32);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    // the table and the workgroup's own slice start from zero (thread i is the only one that ever touches word i of the slice)
    for (uint32_t i = tid; i < n32 + 4u; i += kEpBlock) s_ep[i] = 0;
    // (the address stays in the thread's own vector registers: the walk below takes every scalar register the kernel has)
    unsigned long long *slice = ax.part + (size_t)blockIdx.x * ep_words64(C);
    asm volatile("" : "+v"(slice));
    for (uint32_t i = tid; i < n32 + 2u; i += kEpBlock) slice[i] = 0;
    __syncthreads();
    // the table added into the slice and cleared; every thread of the workgroup calls, between two barriers of its own
    auto flush = [&]() {
        __syncthreads();
        for (uint32_t i = tid; i < n32 + 2u; i += kEpBlock) {
            const unsigned long long v = i < n32 ? (unsigned long long)s_ep[i] : s_wide[i - n32];
            if (v) slice[i] += v;
            if (i < n32) s_ep[i] = 0; else s_wide[i - n32] = 0;
        }
        __syncthreads();
    };
    const uint32_t w_first = a.win0 + (uint32_t)((unsigned long long)blockIdx.x * ax.n_windows / ax.n_groups);
    const uint32_t w_end = a.win0 + (uint32_t)((unsigned long long)(blockIdx.x + 1u) * ax.n_windows / ax.n_groups);
    uint32_t visited = 0;                                           // reads since the last flush: at most ax.piece
    for (uint32_t w = w_first; w < w_end; ++w) {
        const ScanWindow win = scan_window(a, w);
        const uint32_t lo = win.lo, hi = win.hi;
        const uint32_t r_first = a.wfirst[w], r_last = a.wlast[w];
        if (r_first >= r_last || lo >= hi) continue;
        for (uint32_t r0 = r_first; r0 < r_last;) {
            const uint32_t n = r_last - r0 < ax.piece ? r_last - r0 : ax.piece;
            if (visited + n > ax.piece) { flush(); visited = 0; }
            visited += n;
            for (uint32_t r = r0 + wave; r < r0 + n; r += kEpBlock / 64u) {
                const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
                if (!scan_read_counts(a, rr, a.end[r], lo, hi)) continue;
                uint32_t rev = 0;
                if constexpr (FILTERED) {
                    const uint32_t fl = ax.f.flag[r];
                    if (fl & ax.f.exclude_flags) continue;
                    rev = (fl >> 4) & 1u;
                }
                uint32_t k1; unsigned long long slen;
                scan_read_extent(a.rec, r, rr, k1, slen);
                const unsigned long long base = a.seq_base[r / kBlock];
                const unsigned long long s0 = base + (uint32_t)(rr.z - (uint32_t)base);
                // the read is counted in the window that holds the first position it shares with the range
                const uint32_t first = (uint32_t)rr.x > a.start ? (uint32_t)rr.x : a.start;
                if (lane == 0u && first >= lo) atomicAdd(&s_ep[36u * C + EP_READS], 1u);
                const EpSink<FILTERED> sink{ax, s_ep, s_wide, s0, (uint32_t)slen, rev, lane, C};
                dut::ep_walk_read((uint32_t)rr.x, a.cigar + rr.y, k1 - rr.y, (uint32_t)slen, lo, hi, lane, 64u, sink);
            }
            r0 += n;
        }
    }
    flush();
}

// result[i] = the sum of word i of the n_groups slices
__global__ __launch_bounds__(kBlock) void k_site_error_profile_sum(const unsigned long long *part, uint32_t n_groups, uint32_t n_words, unsigned long long *result)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_words) return;
    unsigned long long v = 0;
    for (uint32_t g = 0; g < n_groups; ++g) v += part[(size_t)g * n_words + i];
    result[i] = v;
}

} // namespace clk

// a test hook read at the call: name=value within [lo, hi], else dflt
static uint64_t ep_hook(const char *name, uint64_t dflt, uint64_t lo, uint64_t hi)
{
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const unsigned long long v = strtoull(e, nullptr, 0);
    return v < lo ? lo : v > hi ? hi : v;
}

// The host side: the checks of the scans, the index when this is the first call on a fresh tile, the reference in, the two
// launches, the table back into the context's own storage in the layout of cl_ep_result.
template <bool FILTERED>
static cl_status site_error_profile_run(SiteCtx *c, uint8_t min_quality, typename ScanHost<FILTERED>::Filter filter, uint32_t n_cycles,
                                        const uint8_t *ref_bases, uint64_t ref_len, uint32_t start, uint32_t end, cl_ep_result *out)
{
    static constexpr const char *kWho = "cl_site_error_profile";
    const std::string who = kWho;
    if (!c) return CL_ERR_INVALID;
    if (!out) return fail(c, CL_ERR_INVALID, who + ": null result");
    const char *fault = (n_cycles < 1 || n_cycles > CL_EP_MAX_CYCLES) ? "n_cycles must lie in 1..256" : nullptr;
    cl_status s = site_scan_enter<FILTERED>(c, kWho, filter, fault, ref_bases, ref_len, start, end);
    if (s != CL_OK) return s;
    SiteResident &S = c->site;
    const uint32_t C = n_cycles, n32 = ep_words32(C), n64 = ep_words64(C);
    // the context's storage in the result's layout: from5 and from3 [cycle][16], then ins5, ins3, del5, del3 [cycle]
    std::vector<uint64_t> &tab = S.ep_tab;
    tab.assign((size_t)36 * C, 0);
    memset(out, 0, sizeof(*out));
    out->start = start; out->end = end; out->n_cycles = C;
    out->from5 = tab.data(); out->from3 = tab.data() + 16 * (size_t)C;
    out->ins5 = tab.data() + 32 * (size_t)C; out->ins3 = out->ins5 + C; out->del5 = out->ins3 + C; out->del3 = out->del5 + C;
    S.t_scan.ms = 0.0; S.t_scan.bytes = 0; S.ep_sum_ms = 0.0;
    if (start == end) return CL_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    StageTimer tmr;
    if ((s = site_scan_index(c)) != CL_OK) return s;
    uint64_t n_ref = 0;
    if ((s = site_scan_reference(c, ref_bases, ref_len, start, end, n_ref)) != CL_OK) return s;
    const uint32_t n_windows = (end - 1) / kScanWin - start / kScanWin + 1;
    // DUT_EP_GROUPS, DUT_EP_FLUSH (test hooks): fewer workgroups, each with many windows; flushes between and inside windows.
    // At most kEpGroupsMost workgroups: a slice is up to 74 KB, and more of them gained nothing where it was measured
    const uint32_t n_groups = (uint32_t)std::min<uint64_t>(n_windows, ep_hook("DUT_EP_GROUPS", kEpGroups, 1, kEpGroupsMost));
    const uint64_t flush = ep_hook("DUT_EP_FLUSH", 0xFFFFFFFFull, kScanWin, 0xFFFFFFFFull);
    HIP_TRY(c, S.ep_part.reserve((size_t)n_groups * n64)); HIP_TRY(c, S.ep_sum.reserve(n64));
    S.ep_host.resize(n64);
    EpArgs<FILTERED> A;
    site_scan_fill<FILTERED>(c, A, filter, min_quality, 1, start, end);
    A.s.refb = S.sc_ref.p;
    A.n_cycles = C; A.n_groups = n_groups; A.n_windows = n_windows; A.piece = (uint32_t)(flush / kScanWin); A.part = S.ep_part.p;
    HIP_TRY(c, S.t_scan.start(c->stream));
    hipLaunchKernelGGL((k_site_error_profile<FILTERED>), dim3(n_groups), dim3(kEpBlock), ep_lds_bytes(C), c->stream, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, S.t_ep_sum.start(c->stream));
    hipLaunchKernelGGL(k_site_error_profile_sum, dim3((n64 + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, S.ep_part.p, n_groups, n64, S.ep_sum.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, S.t_ep_sum.stop(c->stream));
    HIP_TRY(c, S.t_scan.stop(c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.ep_host.data(), S.ep_sum.p, (size_t)n64 * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, S.t_scan.read()); HIP_TRY(c, S.t_ep_sum.read());
    S.ep_sum_ms = S.t_ep_sum.ms;
    // the tile as the filtered (unfiltered) calling scan reads it, the reference, the slices written and read, the table
    S.t_scan.bytes = ScanHost<FILTERED>::tile_bytes(S) + n_ref + 2ull * n_groups * n64 * 8 + (uint64_t)n64 * 8;
    tmr.lap("error profile: reference in, table kernel, sum, table back");
    const uint64_t *h = S.ep_host.data();
    for (uint32_t cell = 0; cell < 16u; ++cell)
        for (uint32_t d = 0; d < C; ++d) { tab[(size_t)d * 16 + cell] = h[(size_t)cell * C + d]; tab[((size_t)C + d) * 16 + cell] = h[((size_t)16 + cell) * C + d]; }
    memcpy(tab.data() + 32 * (size_t)C, h + 32 * (size_t)C, (size_t)4 * C * 8);
    const uint64_t *t = h + 36 * (size_t)C;
    for (int k = 0; k < 16; ++k) { out->total[k] = t[k]; out->n_bases += t[k]; }
    out->n_uncomparable = t[EP_UNC]; out->n_reads = t[EP_READS]; out->n_ins = t[EP_INS]; out->n_del = t[EP_DEL];
    out->ins_bases = h[n32]; out->del_bases = h[n32 + 1];
    return CL_OK;
}

extern "C" cl_status cl_site_error_profile(cl_ctx *h, uint8_t min_quality, const cl_scan_filter *filter, uint32_t n_cycles, const uint8_t *ref_bases,
                                           uint64_t ref_len, uint32_t start, uint32_t end, cl_ep_result *out)
{
    return site_entry(h, [&](SiteCtx *c) {
        if (filter) return site_error_profile_run<true>(c, min_quality, filter, n_cycles, ref_bases, ref_len, start, end, out);
        return site_error_profile_run<false>(c, min_quality, ScanNoFilter{}, n_cycles, ref_bases, ref_len, start, end, out);
    });
}

extern "C" cl_status cl_site_error_profile_stats(cl_ctx *h, double *table_ms, double *sum_ms)
{
    if (!h) return CL_ERR_INVALID;
    const SiteResident &S = site_ctx(h)->site;
    if (table_ms) *table_ms = S.t_scan.ms > S.ep_sum_ms ? S.t_scan.ms - S.ep_sum_ms : 0.0;
    if (sum_ms) *sum_ms = S.ep_sum_ms;
    return CL_OK;
}
