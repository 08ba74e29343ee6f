// site_links.hip.h -- joint allele counts of pairs of sites per read over the resident site tile (cl_site_link_counts; a
// textual part of site_engine.hip.h).  Every other site kernel counts a column and forgets which read held which base;
// this one keeps, for an anchor site and its partners, the 6 x 6 table of what one read observes at both.  The rule per
// read is link_observe_read (link_walk.h), written there once.
//
// k_site_links<FILTERED>: one workgroup per anchor (one without partners too: it owns site_counts[i]), over the reads of
// the anchor's window in the scan's index (k_site_scan_index).  Only reads that cover the anchor matter, so that one
// window holds them all whatever max_dist is.  A read takes part under the gates of scan_read_counts over
// [anchor, anchor + 1) and, in the filtered form, the flag load of the filtered scans; bases come from seq4, pass bits
// from the attachment.  The table -- 6 words of site counts, then 36 per partner: at most 2 184 B -- lives in LDS.  A deep
// column puts most lanes of a wave on one cell, so a wave counts its lanes per cell with a ballot and one lane adds the
// count.  At the end the workgroup stores its slice of tables (first[i] gives the place) and of site_counts with plain
// stores: no global atomics, no grow loop, no candidate buffer, and two calls return identical bytes.
#pragma once

#include "link_walk.h"

namespace clk {

static_assert(CL_LINK_CLASSES == CL_LINK_WALK_CLASSES && CL_LINK_MAX_PARTNERS == CL_LINK_WALK_MAX_PARTNERS, "link_walk.h packs the observations of cl_link_result");
static_assert(CL_LINK_MAX_PARTNERS + 1 <= 16, "an anchor and its partners fit the nibbles of one 64-bit word");

constexpr uint32_t kLinkCells = CL_LINK_CLASSES * CL_LINK_CLASSES;               // words of one pair's table
constexpr uint32_t kLinkWords = CL_LINK_CLASSES + kLinkCells * CL_LINK_MAX_PARTNERS; // the largest table of a workgroup
constexpr uint32_t kLinkNoCell = 0xFFFFFFFFu;

template <bool FILTERED> struct LinkArgs {
    ScanArgs s;                                // the tile, the index and the gates, as site_scan_fill sets them
    typename ScanForm<FILTERED>::Filter f;     // the flags, the mask and the pass bits
    void *cand;                                // (site_scan_fill's; unused)
    const uint32_t *sites;                     // n_sites, strictly ascending, each < min(contig_len, ref_len)
    const uint32_t *first;                     // n_sites + 1
    uint32_t *tables;                          // first[n_sites] * 36
    uint32_t *site_counts;                     // n_sites * 6
};

// the stored bases of one read as link_observe_read asks for them
template <bool FILTERED> struct LinkSource {
    const LinkArgs<FILTERED> &ax;
    unsigned long long s0;                     // the read's first base in the numbering of seq4
    __device__ __forceinline__ uint32_t code(uint32_t q) const { return scan_base_code(ax.s.seq4, s0 + q); }
    __device__ __forceinline__ bool passes(uint32_t q) const { return scan_pass_bit(ax.f, s0 + q); }
};

// One more read in `cell` of the table for every calling lane that has one (kLinkNoCell: none).  The lanes of one cell are
// counted with a ballot and their first lane adds the count; only the lanes active at the call take part.
__device__ __forceinline__ void link_add(uint32_t *tab, uint32_t cell, uint32_t lane)
{
    for (bool done = cell == kLinkNoCell; !done;) {
        const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)cell);
        const bool mine = cell == k;
        const unsigned long long m = __ballot(mine);
        if (mine) {
            if (lane == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(&tab[k], (uint32_t)__popcll(m));
            done = true;
        }
    }
}

template <bool FILTERED>
__global__ __launch_bounds__(kBlock) void k_site_links(LinkArgs<FILTERED> ax)
{
    __shared__ uint32_t s_tab[kLinkWords];
    __shared__ uint32_t s_sites[CL_LINK_MAX_PARTNERS + 1];
    const ScanArgs &a = ax.s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, i = blockIdx.x;
    const uint32_t pair0 = ax.first[i], n_part = ax.first[i + 1u] - pair0;       // n_part <= CL_LINK_MAX_PARTNERS: the host built first
    const uint32_t n_words = CL_LINK_CLASSES + kLinkCells * n_part;
    for (uint32_t k = tid; k < n_words; k += kBlock) s_tab[k] = 0;
    if (tid <= n_part) s_sites[tid] = ax.sites[i + tid];                          // i + n_part < n_sites
    __syncthreads();
    const uint32_t anchor = s_sites[0];
    const uint32_t w = anchor / kScanWin;
    const uint32_t r_first = a.wfirst[w], r_last = a.wlast[w];                    // (an empty window holds 0xFFFFFFFF / 0)
    for (uint32_t r = r_first + tid; r < r_last; r += kBlock) {
        const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
        if (!scan_read_counts(a, rr, a.end[r], anchor, anchor + 1u)) continue;   // (anchor < contig_len <= 2^32 - 1)
        if constexpr (FILTERED) {
            if (ax.f.flag[r] & ax.f.exclude_flags) continue;
        }
        uint32_t k1; unsigned long long slen;
        scan_read_extent(a.rec, r, rr, k1, slen);
        const unsigned long long base = a.seq_base[r / kBlock];
        const LinkSource<FILTERED> src{ax, base + (uint32_t)(rr.z - (uint32_t)base)};
        const uint64_t obs = dut::link_observe_read((uint32_t)rr.x, a.cigar + rr.y, k1 - rr.y, (uint32_t)slen, s_sites, n_part + 1u, src);
        const uint32_t ca = dut::link_obs(obs, 0);
        link_add(s_tab, ca != LINK_NONE ? ca : kLinkNoCell, lane);
        if (ca == LINK_NONE) continue;
        for (uint32_t j = 1; j <= n_part; ++j) {
            const uint32_t cb = dut::link_obs(obs, j);
            link_add(s_tab, cb != LINK_NONE ? CL_LINK_CLASSES + kLinkCells * (j - 1u) + CL_LINK_CLASSES * ca + cb : kLinkNoCell, lane);
        }
    }
    __syncthreads();
    if (tid < CL_LINK_CLASSES) ax.site_counts[(size_t)i * CL_LINK_CLASSES + tid] = s_tab[tid];
    uint32_t *out = ax.tables + (size_t)pair0 * kLinkCells;
    for (uint32_t k = tid; k < kLinkCells * n_part; k += kBlock) out[k] = s_tab[CL_LINK_CLASSES + k];
}

} // namespace clk

// The host side: the checks, the pair set, the index when this is the first call on a fresh tile, sites and offsets in,
// one launch, the slices back into the context's own storage.
template <bool FILTERED>
static cl_status site_link_counts_run(SiteCtx *c, uint8_t min_quality, typename ScanHost<FILTERED>::Filter filter, const uint32_t *sites, size_t n_sites,
                                      uint32_t max_dist, uint32_t max_partners, cl_link_result *out)
{
    static constexpr const char *kWho = "cl_site_link_counts";
    const std::string who = kWho;
    if (!c) return CL_ERR_INVALID;
    if (!out) return fail(c, CL_ERR_INVALID, who + ": null result");
    cl_status s = site_scan_check(c, kWho, 0, 0);
    if (s != CL_OK) return s;
    SiteResident &S = c->site;
    if constexpr (FILTERED) {
        if (!S.attached) return fail(c, CL_ERR_INVALID, who + " without cl_site_attach_quals on the resident tile");
    }
    if (n_sites > CL_LINK_MAX_SITES) return fail(c, CL_ERR_INVALID, who + ": more than CL_LINK_MAX_SITES sites");
    if (n_sites && !sites) return fail(c, CL_ERR_INVALID, who + ": null sites");
    if (max_dist == 0) return fail(c, CL_ERR_INVALID, who + ": max_dist must be at least 1");
    if (max_partners < 1 || max_partners > CL_LINK_MAX_PARTNERS) return fail(c, CL_ERR_INVALID, who + ": max_partners must lie in 1.." + std::to_string(CL_LINK_MAX_PARTNERS));
    const uint64_t limit = std::min<uint64_t>(S.contig_len, S.ref_len);
    for (size_t i = 0; i < n_sites; ++i) {
        if (i && sites[i] <= sites[i - 1]) return fail(c, CL_ERR_INVALID, who + ": sites must be strictly ascending: site " + std::to_string(i) + " (" + std::to_string(sites[i]) + ") is not above site " + std::to_string(i - 1) + " (" + std::to_string(sites[i - 1]) + ")");
        if (sites[i] >= limit) return fail(c, CL_ERR_INVALID, who + ": site " + std::to_string(i) + " (" + std::to_string(sites[i]) + ") lies beyond the contig or its reference (" + std::to_string(limit) + " positions)");
    }
    std::vector<uint32_t> first(n_sites + 1, 0);
    uint64_t n_pairs = 0;
    for (size_t i = 0; i < n_sites; ++i) {
        first[i] = (uint32_t)std::min<uint64_t>(n_pairs, 0xFFFFFFFFull);
        n_pairs += dut::link_partner_count(sites, n_sites, i, max_dist, max_partners);
    }
    if (n_pairs > CL_LINK_MAX_PAIRS) return fail(c, CL_ERR_INVALID, who + ": " + std::to_string(n_pairs) + " pairs, more than CL_LINK_MAX_PAIRS (" + std::to_string(CL_LINK_MAX_PAIRS) + ")");
    first[n_sites] = (uint32_t)n_pairs;
    S.link_first.swap(first);                                                     // (a refused call leaves the last result's arrays alone)
    const size_t n_tab = (size_t)n_pairs * kLinkCells, n_cnt = n_sites * CL_LINK_CLASSES;
    S.link_tables.resize(n_tab); S.link_counts.resize(n_cnt);
    out->n_sites = n_sites; out->n_pairs = (size_t)n_pairs;
    out->first = S.link_first.data(); out->tables = S.link_tables.data(); out->site_counts = S.link_counts.data();
    S.t_scan.ms = 0.0; S.t_scan.bytes = 0;
    if (n_sites == 0) return CL_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    StageTimer tmr;
    if ((s = site_scan_index(c)) != CL_OK) return s;
    HIP_TRY(c, S.lk_sites.reserve(n_sites)); HIP_TRY(c, S.lk_first.reserve(n_sites + 1));
    HIP_TRY(c, S.lk_tables.reserve(n_tab + 1)); HIP_TRY(c, S.lk_counts.reserve(n_cnt));
    HIP_TRY(c, hipMemcpyAsync(S.lk_sites.p, sites, n_sites * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.lk_first.p, S.link_first.data(), (n_sites + 1) * 4, hipMemcpyHostToDevice, c->stream));
    LinkArgs<FILTERED> A;
    site_scan_fill<FILTERED>(c, A, filter, min_quality, 1, 0, S.contig_len);
    A.sites = S.lk_sites.p; A.first = S.lk_first.p; A.tables = S.lk_tables.p; A.site_counts = S.lk_counts.p;
    HIP_TRY(c, S.t_scan.start(c->stream));
    hipLaunchKernelGGL((k_site_links<FILTERED>), dim3((uint32_t)n_sites), dim3(kBlock), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, S.t_scan.stop(c->stream));
    if (n_tab) { HIP_TRY(c, hipMemcpyAsync(S.link_tables.data(), S.lk_tables.p, n_tab * 4, hipMemcpyDeviceToHost, c->stream)); }
    HIP_TRY(c, hipMemcpyAsync(S.link_counts.data(), S.lk_counts.p, n_cnt * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, S.t_scan.read());
    // the sites and offsets read, the tables and site counts written (of the tile an anchor reads its window's records,
    // ends, CIGAR words, flags, bases and pass bits: not counted, as for cl_site_str_lengths)
    S.t_scan.bytes = (uint64_t)n_sites * 8 + 4 + (uint64_t)(n_tab + n_cnt) * 4;
    tmr.lap("linked sites: sites in, kernel, tables back");
    return CL_OK;
}

extern "C" cl_status cl_site_link_counts(cl_ctx *h, uint8_t min_quality, const cl_scan_filter *filter, const uint32_t *sites, size_t n_sites,
                                         uint32_t max_dist, uint32_t max_partners, cl_link_result *out)
{
    return site_entry(h, [&](SiteCtx *c) {
        if (filter) return site_link_counts_run<true>(c, min_quality, filter, sites, n_sites, max_dist, max_partners, out);
        return site_link_counts_run<false>(c, min_quality, ScanNoFilter{}, sites, n_sites, max_dist, max_partners, out);
    });
}
