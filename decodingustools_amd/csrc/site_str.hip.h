// site_str.hip.h -- allele lengths of short tandem repeats over the resident site tile (cl_site_str_lengths; a textual
// part of site_engine.hip.h).  The unit of work is an interval with flanks instead of a position: per locus [s, e) the
// histogram of delta = (bases the read holds between the flanks) - (e - s) over the reads that span it, and the number of
// reads that take part without spanning it.  The rule per read is str_measure_read (str_walk.h), written there once.
//
// k_site_str_lengths<FILTERED>: one workgroup per locus, over the reads of the locus's windows in the scan's index
// (k_site_scan_index: the smallest wfirst and the largest wlast over the windows of [s, e), at most two of them since
// e - s <= CL_STR_MAX_SPAN = kScanWin).  A read takes part under the gates of scan_read_counts over [s, e) -- start inside
// the contig, mapq >= min_quality, a reference span that overlaps the locus -- and, in the filtered form, the flag load of
// the filtered scans: (flag & exclude_flags) == 0, reverse iff flag & 0x10.  It loads neither seq4 nor pass bits.  The
// histogram (CL_STR_BINS bins per strand: 512 B, or 1 KB under a filter) and the partial count live in LDS; at the end
// the workgroup stores its own slice of hist and its word of partial with plain stores: no global atomics, no grow loop,
// no candidate buffer.
#pragma once

#include "str_walk.h"

namespace clk {

static_assert(CL_STR_BINS == CL_STR_WALK_BINS, "str_walk.h bins the deltas of cl_str_result");
static_assert(CL_STR_MAX_SPAN <= kScanWin, "a locus lies in at most two windows of the scan's index");
static_assert(sizeof(cl_str_locus) == 8, "the device reads cl_str_locus");

template <bool FILTERED> struct StrArgs {
    ScanArgs s;                                // the tile, the index and the gates, as site_scan_fill sets them
    typename ScanForm<FILTERED>::Filter f;     // the flags and the mask (no pass bit is read)
    void *cand;                                // (site_scan_fill's; unused)
    const cl_str_locus *loci;
    uint32_t flank;
    uint32_t *hist;                            // n_loci * strands * CL_STR_BINS
    uint32_t *partial;                         // n_loci
};

template <bool FILTERED>
__global__ __launch_bounds__(kBlock) void k_site_str_lengths(StrArgs<FILTERED> ax)
{
    constexpr uint32_t kWords = ScanForm<FILTERED>::kStrands * (uint32_t)CL_STR_BINS;
    __shared__ uint32_t s_hist[kWords];
    __shared__ uint32_t s_partial;
    const ScanArgs &a = ax.s;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kWords; i += kBlock) s_hist[i] = 0;
    if (tid == 0) s_partial = 0;
    __syncthreads();
    const cl_str_locus lc = ax.loci[blockIdx.x];                        // 0 <= start < end <= contig_len: the host has checked
    const uint32_t w0 = lc.start / kScanWin, w1 = (lc.end - 1u) / kScanWin;
    const uint32_t f0 = a.wfirst[w0], f1 = a.wfirst[w1], l0 = a.wlast[w0], l1 = a.wlast[w1];
    const uint32_t r_first = f0 < f1 ? f0 : f1, r_last = l0 > l1 ? l0 : l1;   // (an empty window holds 0xFFFFFFFF / 0)
    for (uint32_t r = r_first + tid; r < r_last; r += kBlock) {         // (r_first >= r_last: no read overlaps the locus)
        const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
        if (!scan_read_counts(a, rr, a.end[r], lc.start, lc.end)) continue;
        uint32_t rev = 0;
        if constexpr (FILTERED) {
            const uint32_t fl = ax.f.flag[r];
            if (fl & ax.f.exclude_flags) continue;
            rev = (fl >> 4) & 1u;
        }
        uint32_t k1; unsigned long long slen;
        scan_read_extent(a.rec, r, rr, k1, slen);
        const dut::StrMeasure m = dut::str_measure_read((uint32_t)rr.x, a.cigar + rr.y, k1 - rr.y, lc.start, lc.end, ax.flank);
        if (m.spanning) atomicAdd(&s_hist[rev * (uint32_t)CL_STR_BINS + dut::str_bin(m.delta)], 1u);
        else atomicAdd(&s_partial, 1u);
    }
    __syncthreads();
    uint32_t *out = ax.hist + (size_t)blockIdx.x * kWords;
    for (uint32_t i = tid; i < kWords; i += kBlock) out[i] = s_hist[i];
    if (tid == 0) ax.partial[blockIdx.x] = s_partial;
}

} // namespace clk

// The host side: the checks, the index when this is the first call on a fresh tile, the loci in, one launch, the slices
// back into the context's own storage.
template <bool FILTERED>
static cl_status site_str_lengths_run(SiteCtx *c, uint8_t min_quality, typename ScanHost<FILTERED>::Filter filter, uint32_t flank,
                                      const cl_str_locus *loci, size_t n_loci, cl_str_result *out)
{
    static constexpr const char *kWho = "cl_site_str_lengths";
    const std::string who = kWho;
    if (!c) return CL_ERR_INVALID;
    if (!out) return fail(c, CL_ERR_INVALID, who + ": null result");
    cl_status s = site_scan_check(c, kWho, 0, 0);
    if (s != CL_OK) return s;
    SiteResident &S = c->site;
    if constexpr (FILTERED) {
        if (!S.attached) return fail(c, CL_ERR_INVALID, who + " without cl_site_attach_quals on the resident tile");
        if (filter->use_base_quality) return fail(c, CL_ERR_INVALID, who + ": use_base_quality must be 0 (base qualities take no part in a repeat's length)");
    }
    if (flank < 1 || flank > CL_STR_MAX_FLANK) return fail(c, CL_ERR_INVALID, who + ": flank must lie in 1.." + std::to_string(CL_STR_MAX_FLANK));
    if (n_loci > CL_STR_MAX_LOCI) return fail(c, CL_ERR_INVALID, who + ": more than CL_STR_MAX_LOCI loci");
    if (n_loci && !loci) return fail(c, CL_ERR_INVALID, who + ": null loci");
    for (size_t i = 0; i < n_loci; ++i) {
        const cl_str_locus &l = loci[i];
        const char *why = l.start >= l.end ? "start >= end" : l.end > S.contig_len ? "it ends beyond the contig"
                        : l.end - l.start > CL_STR_MAX_SPAN ? "it is longer than CL_STR_MAX_SPAN" : nullptr;
        if (why) return fail(c, CL_ERR_INVALID, who + ": locus " + std::to_string(i) + " [" + std::to_string(l.start) + ", " + std::to_string(l.end) + "): " + why);
    }
    constexpr uint32_t kStrands = ScanForm<FILTERED>::kStrands;
    const size_t n_hist = n_loci * kStrands * CL_STR_BINS;
    S.str_hist.resize(n_hist); S.str_partial.resize(n_loci);
    out->n_loci = n_loci; out->hist = S.str_hist.data(); out->partial = S.str_partial.data(); out->strands = kStrands;
    S.t_scan.ms = 0.0; S.t_scan.bytes = 0;
    if (n_loci == 0) return CL_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    StageTimer tmr;
    if ((s = site_scan_index(c)) != CL_OK) return s;
    HIP_TRY(c, S.st_loci.reserve(n_loci)); HIP_TRY(c, S.st_hist.reserve(n_hist)); HIP_TRY(c, S.st_partial.reserve(n_loci));
    HIP_TRY(c, hipMemcpyAsync(S.st_loci.p, loci, n_loci * sizeof(cl_str_locus), hipMemcpyHostToDevice, c->stream));
    StrArgs<FILTERED> A;
    site_scan_fill<FILTERED>(c, A, filter, min_quality, 1, 0, S.contig_len);
    A.loci = S.st_loci.p; A.flank = flank; A.hist = S.st_hist.p; A.partial = S.st_partial.p;
    HIP_TRY(c, S.t_scan.start(c->stream));
    hipLaunchKernelGGL((k_site_str_lengths<FILTERED>), dim3((uint32_t)n_loci), dim3(kBlock), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, S.t_scan.stop(c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.str_hist.data(), S.st_hist.p, n_hist * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.str_partial.data(), S.st_partial.p, n_loci * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, S.t_scan.read());
    // the loci read, their slices and partial counts written (of the tile a locus reads its windows' records, ends, CIGAR
    // words and flags: not counted, as for the insertion mode's allele launch)
    S.t_scan.bytes = n_loci * (sizeof(cl_str_locus) + 4) + n_hist * 4;
    tmr.lap("repeat lengths: loci in, kernel, histograms back");
    return CL_OK;
}

extern "C" cl_status cl_site_str_lengths(cl_ctx *h, uint8_t min_quality, const cl_scan_filter *filter, uint32_t flank, const cl_str_locus *loci,
                                         size_t n_loci, cl_str_result *out)
{
    return site_entry(h, [&](SiteCtx *c) {
        if (filter) return site_str_lengths_run<true>(c, min_quality, filter, flank, loci, n_loci, out);
        return site_str_lengths_run<false>(c, min_quality, ScanNoFilter{}, flank, loci, n_loci, out);
    });
}
