// site_engine.hip.h -- the site engine (config 5; a textual part of callable_loci.hip's translation unit): the sparse
// site pileup k_site_pileup with its host side (cl_site_upload / cl_site_run / cl_site_pileup), the host side of the
// dense scans of site_scan.hip.h (cl_site_scan*, cl_site_attach_quals) and their entry points, the repeat lengths of
// site_str.hip.h (cl_site_str_lengths), the error profile of site_errors.hip.h (cl_site_error_profile) and the linked
// sites of site_links.hip.h (cl_site_link_counts), which it includes.  Of a context it uses what EngineBase holds and its own SiteResident.
#pragma once

#include "kernels.hip.h"
#include "engine_base.hip.h"
#include "site_pass_bits.h"

namespace clk {

// ---------------------------------------------------------------------------------------------
// config 5: site-list pileup (src/haplogroup/caller.rs:62-152): for every M/=/X base of a read with
// mapq >= min_quality whose 1-based position is a listed site, hist[site][4-bit base code] += 1.
//
// sorted_pos0 / sorted_idx: the sites sorted by 0-based position and their original indices; bucket[b]: index of
// the first sorted site with position >= 256*b.  One packed record per read (built on the host per call, like
// ReadRec): pos, CIGAR offset, low half of the base offset (the full offset = the block's 64-bit base + the 32-bit
// difference), mapq | n_cigar << 8 | n_bases << 16 with 255 / 0xFFFF meaning "the next record's offsets".
//
// A workgroup takes 256 consecutive reads.  A thread walks its read's first four CIGAR words (one 16-byte load) for
// the reference span and leaves at once when no site lies inside it (three reads in five at one site per ~300
// bases: no per-operation walk, no base is touched); hits go to a histogram of the workgroup's own sites in LDS
// (the reads are sorted, so they share a handful of sites) which is added to the global one once at the end --
// hits outside that range (unsorted input, a very long read) add to the global histogram directly.
// ---------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) SiteRec {
    int32_t  pos;
    uint32_t cigar_off;
    uint32_t seq_lo;
    uint32_t meta;
};
constexpr int kSiteLds = 64;            // sites a workgroup privatises

struct SiteArgs {
    const SiteRec *rec;                 // n + 1
    const unsigned long long *seq_base; // per workgroup of kBlock reads: base offset (in bases) of its first read
    const uint32_t *cigar;              // padded by 8 words
    const uint8_t  *seq4;
    uint32_t n;
    uint32_t min_quality, contig_len;
    unsigned long long ref_len;
    const uint32_t *sorted_pos0, *sorted_idx, *bucket;
    uint32_t n_buckets, n_sites;
    uint32_t *hist;
};

__global__ __launch_bounds__(kBlock) void k_site_pileup(SiteArgs a)
{
    __shared__ uint32_t s_hist[kSiteLds * 16];
    __shared__ uint32_t s_first;
    const uint32_t tid = threadIdx.x;
    const uint32_t r0 = blockIdx.x * kBlock;
    for (uint32_t i = tid; i < (uint32_t)kSiteLds * 16u; i += kBlock) s_hist[i] = 0;
    auto first_site_at = [&](unsigned long long x) {             // first sorted site with position >= x
        const unsigned long long bx = x >> 8;
        uint32_t lo = bx < a.n_buckets ? a.bucket[bx] : a.n_sites;
        while (lo < a.n_sites && a.sorted_pos0[lo] < x) ++lo;
        return lo;
    };
    if (tid == 0) {
        const int32_t p0 = a.rec[r0].pos;
        s_first = first_site_at(p0 < 0 ? 0ull : (unsigned long long)p0);
    }
    __syncthreads();
    const uint32_t first = s_first;
    const uint32_t r = r0 + tid;
    if (r < a.n) {
        const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
        const uint32_t mq = rr.w & 255u;
        // fetch("chr:1-len"), caller.rs:33-36; the mapping-quality gate, caller.rs:80
        if ((uint32_t)rr.x < a.contig_len && mq >= a.min_quality) {
            uint32_t k = rr.y, k1 = k + ((rr.w >> 8) & 255u);
            unsigned long long slen = rr.w >> 16;
            if (((rr.w >> 8) & 255u) == 255u || slen == 0xFFFFull) {
                const uint4 nx = *reinterpret_cast<const uint4 *>(a.rec + r + 1);
                k1 = nx.y; slen = (uint32_t)(nx.z - rr.z);
            }
            const unsigned long long base = a.seq_base[blockIdx.x];
            const unsigned long long s0 = base + (uint32_t)(rr.z - (uint32_t)base);
            Q16 c4;
            __builtin_memcpy(&c4, a.cigar + k, 16);
            const uint32_t n = k1 - k;
            unsigned long long x = (uint32_t)rr.x, reflen = 0;
#pragma unroll
            for (uint32_t d = 0; d < 4u; ++d) {
                const uint32_t c = d < n ? c4.w[d] : 5u;
                reflen += ((0x18Du >> (c & 15u)) & 1u) ? (c >> 4) : 0u;
            }
            for (uint32_t kk = k + 4u; kk < k1; ++kk) {
                const uint32_t c = a.cigar[kk];
                reflen += ((0x18Du >> (c & 15u)) & 1u) ? (c >> 4) : 0u;
            }
            uint32_t lo = first_site_at(x);
            if (lo < a.n_sites && a.sorted_pos0[lo] < x + reflen) {      // some site inside the read's span: walk it
                unsigned long long y = 0;
                for (uint32_t kk = k; kk < k1; ++kk) {
                    const uint32_t d = kk - k;
                    const uint32_t c = d == 0 ? c4.w[0] : d == 1 ? c4.w[1] : d == 2 ? c4.w[2] : d == 3 ? c4.w[3] : a.cigar[kk];
                    const uint32_t op = c & 15u, l = c >> 4;
                    if (op_match(op)) {
                        while (lo < a.n_sites && a.sorted_pos0[lo] < x) ++lo;
                        for (; lo < a.n_sites && a.sorted_pos0[lo] < x + l; ++lo) {
                            const unsigned long long p = a.sorted_pos0[lo];
                            const unsigned long long qi = y + (p - x);
                            if (qi < slen && p < a.ref_len) {           // caller.rs:105,110-113
                                const unsigned long long bi = s0 + qi;
                                const uint32_t byte = a.seq4[bi >> 1];
                                const uint32_t code = (bi & 1ull) ? (byte & 15u) : (byte >> 4);
                                const uint32_t slot = lo - first;       // below `first`: wraps, goes to the global one
                                if (slot < (uint32_t)kSiteLds) atomicAdd(&s_hist[slot * 16u + code], 1u);
                                else atomicAdd(&a.hist[(unsigned long long)a.sorted_idx[lo] * 16ull + code], 1u);
                            }
                        }
                        x += l; y += l;
                    } else if (op_del(op)) {
                        x += l;
                    } else if (op_ins(op)) {
                        y += l;
                    }
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < (uint32_t)kSiteLds * 16u; i += kBlock) {
        const uint32_t v = s_hist[i], si = first + (i >> 4);
        if (v && si < a.n_sites) atomicAdd(&a.hist[(unsigned long long)a.sorted_idx[si] * 16ull + (i & 15u)], v);
    }
}

} // namespace clk

#include "site_scan.hip.h"

using namespace clk;

// config 5: the resident tile of the site pileup (cl_site_upload) and the buffers of a run
struct SiteResident {
    DevBuf<SiteRec> rec; DevBuf<uint8_t> seq; DevBuf<uint32_t> cig, p0, ix, hist, bk; DevBuf<unsigned long long> base;
    uint64_t n = 0, ncig = 0, nbase = 0, ref_len = 0;
    uint32_t contig_len = 0;
    bool resident = false;
    bool filtered = false;           // the resident tile holds only the reads that overlap a site of the list it was uploaded for (cl_site_pileup)
    // cl_site_scan: the per-read ends and per-window read ranges of the resident tile (built by the first scan), the
    // reference bytes of the range, class counts + candidate count, candidates, dense counters (of either form)
    DevBuf<uint32_t> sc_end, sc_wfirst, sc_wlast, sc_dense;
    DevBuf<uint8_t> sc_ref;
    DevBuf<unsigned long long> sc_cls;
    DevBuf<ScanCand> sc_cand;
    bool scan_indexed = false;
    // cl_site_attach_quals: one pass bit per base of seq, one flag per read; the filtered scan's candidates, ambiguous
    // positions and their 16-code histograms
    DevBuf<unsigned long long> q_pass;
    DevBuf<uint16_t> q_flag;
    DevBuf<ScanCandEx> sx_cand;
    DevBuf<uint32_t> sx_amb, sx_hist;
    bool attached = false;
    DevBuf<ScanMinorCand> sm_cand;   // cl_site_scan_minor's candidates, of either form
    DevBuf<ScanCountCand> sd_cand;   // cl_site_scan_dels' candidates, of either form
    // cl_site_scan_ins: its candidates, of either form; the called positions as its allele launch takes them, the
    // observations and the insertions found per position
    DevBuf<ScanCountCand> si_cand;
    DevBuf<ScanInsSite> si_site;
    DevBuf<ScanInsObs> si_obs;
    DevBuf<uint32_t> si_found;
    // cl_site_scan_consensus: the packed bytes of the launched windows, four positions per word, and the range's bytes
    DevBuf<uint32_t> sk_cons;
    std::vector<uint8_t> cons_bytes;
    // cl_site_str_lengths (site_str.hip.h): the loci as sent, their histograms and partial counts, on the device and back
    DevBuf<cl_str_locus> st_loci;
    DevBuf<uint32_t> st_hist, st_partial;
    std::vector<uint32_t> str_hist, str_partial;
    // cl_site_error_profile (site_errors.hip.h): the workgroups' slices and their sum on the device, the sum as it came
    // back, the tables in the result's layout; the sum launch's own events and duration
    DevBuf<unsigned long long> ep_part, ep_sum;
    std::vector<uint64_t> ep_host, ep_tab;
    KernelTimer t_ep_sum;
    double ep_sum_ms = 0.0;
    // cl_site_link_counts (site_links.hip.h): the sites and pair offsets as sent, the tables and site counts, on the device
    // and back
    DevBuf<uint32_t> lk_sites, lk_first, lk_tables, lk_counts;
    std::vector<uint32_t> link_first, link_tables, link_counts;
    // the last cl_site_pileup / cl_site_run and the last cl_site_scan* of either form: the kernels' duration and their
    // algorithmic bytes; the candidates of the last cl_site_scan, cl_site_scan_ex, cl_site_scan_minor and cl_site_scan_dels
    KernelTimer t_pileup, t_scan;
    std::vector<cl_scan_candidate> scan_cand;
    std::vector<cl_scan_candidate_ex> scan_cand_ex;
    std::vector<cl_minor_candidate> minor_cand;
    std::vector<cl_del_candidate> del_cand;
    std::vector<cl_ins_candidate> ins_cand;
    std::vector<cl_ins_obs> ins_obs;
    double ins_scan_ms = 0.0, ins_alleles_ms = 0.0;      // the last cl_site_scan_ins: its two launches
    void release()
    {
        t_pileup.destroy(); t_scan.destroy(); t_ep_sum.destroy();
        q_pass.release(); q_flag.release(); sx_cand.release(); sx_amb.release(); sx_hist.release(); sm_cand.release(); sd_cand.release();
        si_cand.release(); si_site.release(); si_obs.release(); si_found.release(); sk_cons.release();
        st_loci.release(); st_hist.release(); st_partial.release(); ep_part.release(); ep_sum.release();
        lk_sites.release(); lk_first.release(); lk_tables.release(); lk_counts.release();
        rec.release(); seq.release(); cig.release(); p0.release(); ix.release(); hist.release(); bk.release(); base.release();
        sc_end.release(); sc_wfirst.release(); sc_wlast.release(); sc_dense.release(); sc_ref.release(); sc_cls.release(); sc_cand.release();
        resident = false; scan_indexed = false;
    }
};

// A context as the site engine sees it; cl_ctx (callable_loci.hip) derives from it and defines site_ctx.
struct SiteCtx : EngineBase { SiteResident site; };
static SiteCtx *site_ctx(cl_ctx *c);

// the site list as the kernel wants it: sorted by 0-based position (vcf_pos - 1, caller.rs:94) with the original
// indices, vcf_pos 0 left out (it can never match), and the first sorted site at or after every 256th position
struct SitePrep { std::vector<uint32_t> pos0, idx, bucket; uint32_t n_buckets = 0; };
static void site_prepare(const uint32_t *sites, size_t n_sites, SitePrep &P)
{
    // (position, original index) sorted by position, ties by index: a stable radix sort on the 32-bit positions, three
    // passes of 11 bits (std::sort took 10 of the 11 ms of a run on a resident tile with 200 000 sites)
    std::vector<unsigned long long> key(n_sites), tmp(n_sites);
    for (size_t i = 0; i < n_sites; ++i) key[i] = ((unsigned long long)sites[i] << 32) | (unsigned long long)i;
    for (int pass = 0; pass < 3; ++pass) {
        const int sh = 32 + 11 * pass;
        size_t cnt[2049] = {0};
        for (size_t i = 0; i < n_sites; ++i) cnt[((key[i] >> sh) & 2047u) + 1] += 1;
        for (int b = 0; b < 2048; ++b) cnt[b + 1] += cnt[b];
        for (size_t i = 0; i < n_sites; ++i) tmp[cnt[(key[i] >> sh) & 2047u]++] = key[i];
        key.swap(tmp);
    }
    P.pos0.reserve(n_sites); P.idx.reserve(n_sites);
    for (size_t i = 0; i < n_sites; ++i) {
        const uint32_t s = (uint32_t)(key[i] >> 32);
        if (s == 0) continue;
        P.pos0.push_back(s - 1); P.idx.push_back((uint32_t)key[i]);
    }
    if (P.pos0.empty()) return;
    P.n_buckets = (uint32_t)(((uint64_t)P.pos0.back() >> 8) + 2);
    P.bucket.resize(P.n_buckets);
    size_t j = 0;
    for (uint32_t bk = 0; bk < P.n_buckets; ++bk) {
        while (j < P.pos0.size() && P.pos0[j] < ((uint64_t)bk << 8)) ++j;
        P.bucket[bk] = (uint32_t)j;
    }
}

// cl_site_pileup knows the site list when the tile is uploaded: only the reads that can add to the histogram travel --
// those the kernel itself would walk (k_site_pileup: position inside the contig, mapq >= min_quality, a site inside
// [pos, pos + reference span)); at one site per ~300 bases that is two short reads in five, and the bases are what the
// call spends its time sending (1.1 GB at the link's rate for BASELINE configs[4]).  The kept reads' records, CIGAR words
// and base BYTES are gathered straight into the pinned buffers; a read keeps its nibble parity (its bytes are copied
// whole), so read lengths can no longer be taken from offset differences: tiles with a read of 65 535 bases or 255
// operations and more (the records' escape values) are sent whole instead.
struct SiteGather {
    dut::Scratch<uint32_t> kidx;               // kept read k = read kidx[k] of the tile
    dut::Scratch<unsigned long long> B;        // K + 1: first byte of kept read k in the gathered base array
    dut::Scratch<uint32_t> coff;               // K + 1: first CIGAR word of kept read k in the gathered CIGAR array
    uint64_t K = 0;
    bool on = false;
};
static void site_filter(const cl_site_tile *t, const SitePrep &P, uint8_t min_quality, uint32_t contig_len, SiteGather &G)
{
    const uint64_t n = t->n_reads;
    G.on = false;
    if (n == 0 || P.pos0.empty()) return;
    const size_t grain = 1u << 16, nchunk = (n + grain - 1) / grain;
    dut::Scratch<uint8_t> keep(n);
    std::vector<uint64_t> c_k(nchunk + 1, 0), c_b(nchunk + 1, 0), c_c(nchunk + 1, 0);
    std::atomic<bool> escape{false};
    const uint32_t *pos0 = P.pos0.data(); const uint32_t *bucket = P.bucket.data();
    const uint32_t n_sites = (uint32_t)P.pos0.size(), n_buckets = P.n_buckets;
    uint8_t *kp = keep.get();
    dut::parallel_for(nchunk, 1, [&](size_t ch) {
        const size_t a = ch * grain, b = std::min<size_t>(n, a + grain);
        uint64_t k = 0, nb = 0, nc = 0;
        for (size_t i = a; i < b; ++i) {
            kp[i] = 0;
            const uint32_t c0 = t->cigar_off[i], c1 = t->cigar_off[i + 1];
            const uint64_t s0 = t->seq_off[i], s1 = t->seq_off[i + 1];
            if (c1 < c0 || s1 < s0) { escape.store(true); continue; }          // (refused by the upload's own check)
            if (c1 - c0 >= 255u || s1 - s0 >= 0xFFFFull) escape.store(true);
            if ((uint32_t)t->pos[i] >= contig_len || t->mapq[i] < min_quality) continue;
            unsigned long long reflen = 0;
            for (uint32_t q = c0; q < c1; ++q) { const uint32_t cw = t->cigar[q]; reflen += ((0x18Du >> (cw & 15u)) & 1u) ? (cw >> 4) : 0u; }
            const unsigned long long x = (uint32_t)t->pos[i];
            const unsigned long long bx = x >> 8;
            uint32_t lo = bx < n_buckets ? bucket[bx] : n_sites;
            while (lo < n_sites && pos0[lo] < x) ++lo;
            if (lo < n_sites && pos0[lo] < x + reflen) { kp[i] = 1; ++k; nb += ((s1 + 1) >> 1) - (s0 >> 1); nc += c1 - c0; }
        }
        c_k[ch + 1] = k; c_b[ch + 1] = nb; c_c[ch + 1] = nc;
    });
    if (escape.load()) return;
    for (size_t ch = 0; ch < nchunk; ++ch) { c_k[ch + 1] += c_k[ch]; c_b[ch + 1] += c_b[ch]; c_c[ch + 1] += c_c[ch]; }
    const uint64_t K = c_k[nchunk];
    if (c_c[nchunk] > 0xFFFFFFF0ull) return;
    G.kidx = dut::Scratch<uint32_t>(K + 1); G.B = dut::Scratch<unsigned long long>(K + 1); G.coff = dut::Scratch<uint32_t>(K + 1);
    uint32_t *kidx = G.kidx.get(); unsigned long long *B = G.B.get(); uint32_t *coff = G.coff.get();
    dut::parallel_for(nchunk, 1, [&](size_t ch) {
        const size_t a = ch * grain, b = std::min<size_t>(n, a + grain);
        uint64_t k = c_k[ch], nb = c_b[ch], nc = c_c[ch];
        for (size_t i = a; i < b; ++i) {
            if (!kp[i]) continue;
            kidx[k] = (uint32_t)i; B[k] = nb; coff[k] = (uint32_t)nc;
            nb += ((t->seq_off[i + 1] + 1) >> 1) - (t->seq_off[i] >> 1); nc += t->cigar_off[i + 1] - t->cigar_off[i];
            ++k;
        }
    });
    kidx[K] = 0; B[K] = c_b[nchunk]; coff[K] = (uint32_t)c_c[nchunk];
    G.K = K; G.on = true;
}

// ---- config 5: the tile goes to HBM once (cl_site_upload: packed records built straight into the pinned buffers, the
//      4-bit bases and the CIGAR words through the staging ring) and stays resident; any number of site lists can then be
//      run over it (cl_site_run).  cl_site_pileup is the two in one call. ----
static cl_status cl_site_upload_impl(SiteCtx *c, uint32_t contig_len, uint64_t ref_len, const cl_site_tile *t, const SiteGather *G = nullptr)
{
    if (!c || !t) return CL_ERR_INVALID;
    if (c->host_only) return fail(c, CL_ERR_DEVICE, "a host-only context has no device");
    HIP_TRY(c, hipSetDevice(c->device));
    drop_prefetch(c);                                        // the ring is needed below
    SiteResident &S = c->site;
    S.resident = false; S.filtered = false; S.scan_indexed = false; S.attached = false;
    const uint64_t n_all = t->n_reads;
    if (n_all > 0xFFFFFFF0ull) return fail(c, CL_ERR_RANGE, "too many reads");
    if (n_all && (!t->pos || !t->mapq || !t->cigar_off || !t->seq_off)) return fail(c, CL_ERR_INVALID, "null tile array");
    StageTimer tmr;
    // what travels: the whole tile, or (cl_site_pileup, site_filter above) the reads that overlap a site of its list
    const bool g = G && G->on;
    if (!g) {                                                // (site_filter has looked at every offset pair already)
        std::atomic<int> bad{0};
        dut::parallel_for(n_all, 262144, [&](size_t i) { if (t->cigar_off[i + 1] < t->cigar_off[i] || t->seq_off[i + 1] < t->seq_off[i]) bad = 1; });
        if (bad) return fail(c, CL_ERR_INVALID, "offset arrays must be non-decreasing");
    }
    const uint64_t n = g ? G->K : n_all;
    const uint32_t *kidx = g ? G->kidx.get() : nullptr;
    const unsigned long long *GB = g ? G->B.get() : nullptr;
    const uint32_t *gco = g ? G->coff.get() : nullptr;
    const uint64_t ncig = g ? gco[n] : (n_all ? t->cigar_off[n_all] : 0);
    const uint64_t nbytes = g ? GB[n] : ((n_all ? t->seq_off[n_all] : 0) + 1) / 2;
    const uint64_t nbase = g ? 2 * GB[n] : (n_all ? t->seq_off[n_all] : 0);
    const uint64_t *hs_all = t->seq_off;
    // base offset of (kept) read k in the array that travels; k = n: its end
    auto seq_at = [=](uint64_t k) -> uint64_t { return !g ? hs_all[k] : (k < n ? 2 * GB[k] + (hs_all[kidx[k]] & 1ull) : nbase); };
    const uint64_t n_blocks = (n + kBlock - 1) / kBlock;
    // a workgroup's reads must lie within 2^32 bases of its first one (256 reads: always, short of 16 M-base reads)
    for (uint64_t b = 0; b < n_blocks; ++b)
        if (seq_at(std::min<uint64_t>(n, (b + 1) * kBlock)) - seq_at(b * kBlock) > 0xFFFF0000ull)
            return fail(c, CL_ERR_RANGE, "reads too long for the site pileup");
    HIP_TRY(c, S.rec.reserve(n + 1)); HIP_TRY(c, S.base.reserve(n_blocks + 1));
    HIP_TRY(c, S.cig.reserve(ncig + 8)); HIP_TRY(c, S.seq.reserve(nbytes + 16));
    tmr.lap("site upload: checks + device buffers");
    cl_status rs = CL_OK;
    // the bases: the bulk of the tile (0.5 byte per aligned base)
    if (nbytes && !g && (rs = ring_copy(c, S.seq.p, t->seq4, nbytes)) != CL_OK) return rs;
    if (nbytes && g) {
        const uint8_t *seq4 = t->seq4;
        rs = ring_start(c, S.seq.p, nbytes, [seq4, hs_all, kidx, GB, n](uint64_t off, uint64_t len, uint8_t *out) {
            // the kept reads whose bytes fall into [off, off + len): whole bytes of the tile's array, read by read
            uint64_t k = (uint64_t)(std::upper_bound(GB, GB + n + 1, (unsigned long long)off) - GB) - 1;
            uint64_t at = off;
            const uint64_t end = off + len;
            while (at < end && k < n) {
                const uint64_t src0 = hs_all[kidx[k]] >> 1, take = std::min<uint64_t>(GB[k + 1], end) - at;
                memcpy(out + (at - off), seq4 + src0 + (at - GB[k]), take);
                at += take;
                if (at == GB[k + 1]) ++k;
            }
        }, PinRing::kPinBytes, PinRing::kCopyThreads);
        if (rs == CL_OK) rs = ring_finish(c); else (void)ring_finish(c);
        if (rs != CL_OK) return rs;
    }
    tmr.lap("site upload: bases");
    // one packed record per read (+ the sentinel with the totals), built in the pinned buffers
    {
        const int32_t *hp = t->pos; const uint8_t *hm = t->mapq; const uint32_t *hc = t->cigar_off;
        const uint64_t ncig_all = ncig;
        rs = ring_start(c, reinterpret_cast<uint8_t *>(S.rec.p), (n + 1) * sizeof(SiteRec), [=](uint64_t off, uint64_t len, uint8_t *out) {
            SiteRec *o = reinterpret_cast<SiteRec *>(out);
            const size_t i0 = off / sizeof(SiteRec), i1 = (off + len) / sizeof(SiteRec);
            for (size_t k = i0; k < i1; ++k) {
                SiteRec r;
                if (k < n) {
                    const size_t i = g ? kidx[k] : k;
                    const uint32_t nc = hc[i + 1] - hc[i];
                    const uint64_t sl = hs_all[i + 1] - hs_all[i];
                    r.pos = hp[i]; r.cigar_off = g ? gco[k] : hc[i]; r.seq_lo = (uint32_t)seq_at(k);
                    r.meta = (uint32_t)hm[i] | (std::min<uint32_t>(nc, 255u) << 8) | ((uint32_t)std::min<uint64_t>(sl, 0xFFFFull) << 16);
                } else { r.pos = 0; r.cigar_off = (uint32_t)ncig_all; r.seq_lo = (uint32_t)nbase; r.meta = 0; }
                o[k - i0] = r;
            }
        }, PinRing::kPinBytes, g ? PinRing::kCopyThreads : 0);
        // ... beside it, the 64-bit base offset of every workgroup's first read
        std::vector<unsigned long long> h_base(n_blocks + 1);
        for (uint64_t b = 0; b < n_blocks; ++b) h_base[b] = seq_at(b * kBlock);
        h_base[n_blocks] = nbase;
        if (rs == CL_OK) rs = ring_finish(c); else (void)ring_finish(c);
        if (rs != CL_OK) return rs;
        HIP_TRY(c, hipMemcpyAsync(S.base.p, h_base.data(), (n_blocks + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (ncig && !g && (rs = ring_copy(c, S.cig.p, t->cigar, ncig * 4)) != CL_OK) return rs;
    if (ncig && g) {
        const uint32_t *cig = t->cigar; const uint32_t *hc = t->cigar_off;
        rs = ring_start(c, reinterpret_cast<uint8_t *>(S.cig.p), ncig * 4, [cig, hc, kidx, gco, n](uint64_t off, uint64_t len, uint8_t *out) {
            const uint64_t w0 = off / 4, w1 = (off + len) / 4;                  // (a buffer is a whole number of words)
            uint64_t k = (uint64_t)(std::upper_bound(gco, gco + n + 1, (uint32_t)w0) - gco) - 1;
            uint64_t at = w0;
            uint32_t *o = reinterpret_cast<uint32_t *>(out);
            while (at < w1 && k < n) {
                const uint64_t take = std::min<uint64_t>(gco[k + 1], w1) - at;
                const uint32_t *src = cig + hc[kidx[k]] + (at - gco[k]);
                uint32_t *dstw = o + (at - w0);
                for (uint64_t q = 0; q < take; ++q) dstw[q] = src[q];          // (a read has a word or three)
                at += take;
                if (at == gco[k + 1]) ++k;
            }
        }, PinRing::kPinBytes, PinRing::kCopyThreads);
        if (rs == CL_OK) rs = ring_finish(c); else (void)ring_finish(c);
        if (rs != CL_OK) return rs;
    }
    tmr.lap("site upload: records + cigar");
    S.n = n; S.ncig = ncig; S.nbase = nbase; S.contig_len = contig_len; S.ref_len = ref_len;
    S.resident = true; S.filtered = g;
    return CL_OK;
}

static cl_status cl_site_run_impl(SiteCtx *c, uint8_t min_quality, const uint32_t *sites, size_t n_sites, uint32_t *hist, const SitePrep *ready)
{
    if (!c || (!sites && n_sites) || (!hist && n_sites)) return CL_ERR_INVALID;
    if (c->host_only) return fail(c, CL_ERR_DEVICE, "a host-only context has no device");
    SiteResident &S = c->site;
    if (!S.resident) return fail(c, CL_ERR_INVALID, "cl_site_run without cl_site_upload");
    // (a tile that cl_site_pileup filtered for its own list serves that call only: ready != nullptr is that call)
    if (S.filtered && !ready) return fail(c, CL_ERR_INVALID, "cl_site_run: the resident tile was uploaded by cl_site_pileup for its own site list; cl_site_upload gives a tile that serves any list");
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_sites == 0) return CL_OK;
    if (n_sites > 0x0FFFFFFFu) return fail(c, CL_ERR_RANGE, "too many sites");
    StageTimer tmr;
    SitePrep mine;
    if (!ready) { site_prepare(sites, n_sites, mine); ready = &mine; }
    const std::vector<uint32_t> &pos0 = ready->pos0, &idx = ready->idx, &bucket = ready->bucket;
    const uint32_t n_buckets = ready->n_buckets;
    memset(hist, 0, n_sites * 16 * sizeof(uint32_t));
    if (S.n == 0 || pos0.empty()) return CL_OK;
    tmr.lap("site run: sort + buckets");
    HIP_TRY(c, S.p0.reserve(pos0.size())); HIP_TRY(c, S.ix.reserve(pos0.size())); HIP_TRY(c, S.hist.reserve(n_sites * 16));
    HIP_TRY(c, S.bk.reserve(n_buckets));
    HIP_TRY(c, hipMemsetAsync(S.hist.p, 0, n_sites * 16 * 4, c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.p0.p, pos0.data(), pos0.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.ix.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.bk.p, bucket.data(), (size_t)n_buckets * 4, hipMemcpyHostToDevice, c->stream));
    SiteArgs A;
    A.rec = S.rec.p; A.seq_base = S.base.p; A.cigar = S.cig.p; A.seq4 = S.seq.p; A.n = (uint32_t)S.n;
    A.min_quality = min_quality; A.contig_len = S.contig_len; A.ref_len = S.ref_len;
    A.sorted_pos0 = S.p0.p; A.sorted_idx = S.ix.p; A.bucket = S.bk.p; A.n_buckets = n_buckets; A.n_sites = (uint32_t)pos0.size();
    A.hist = S.hist.p;
    HIP_TRY(c, S.t_pileup.start(c->stream));
    hipLaunchKernelGGL(k_site_pileup, dim3((uint32_t)((S.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, S.t_pileup.stop(c->stream));
    HIP_TRY(c, hipMemcpyAsync(hist, S.hist.p, n_sites * 16 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, S.t_pileup.read());
    // 4-bit bases + per-read pos/mapq/offsets + CIGAR words read, the sites' positions /
    // indices read and their 16 counters written
    S.t_pileup.bytes = (S.nbase + 1) / 2 + S.n * sizeof(SiteRec) + S.ncig * 4 + (uint64_t)pos0.size() * 8 + (uint64_t)n_sites * 64;
    tmr.lap("site run: kernel + histogram back");
    return CL_OK;
}

// ---- config 5, dense form: base counts and calls at every position of a range of the resident tile (site_scan.hip.h),
// ---- unfiltered (cl_site_scan) and filtered, strand-aware (cl_site_scan_ex, behind cl_site_attach_quals) ----
// The device writes the public records field by field and the host copies them out as bytes: the same size, and every
// field of the device's struct D at the offset and of the width of its field of the public struct H.
#define SCAN_AT(D, H, df, hf) (offsetof(D, df) == offsetof(H, hf) && sizeof(D::df) == sizeof(H::hf))
#define SCAN_AT4(D, H, a, b, c, d) (SCAN_AT(D, H, a, a) && SCAN_AT(D, H, b, b) && SCAN_AT(D, H, c, c) && SCAN_AT(D, H, d, d))
#define SCAN_COUNT_AS(H, x) (sizeof(ScanCountCand) == sizeof(H) && sizeof(H) == 32 && SCAN_AT4(ScanCountCand, H, pos, ref, pad, depth) && SCAN_AT(ScanCountCand, H, n, x) && \
                             SCAN_AT(ScanCountCand, H, n_fwd, x##_fwd) && SCAN_AT(ScanCountCand, H, n_rev, x##_rev) && SCAN_AT(ScanCountCand, H, depth_fwd, depth_fwd) && \
                             SCAN_AT(ScanCountCand, H, depth_rev, depth_rev))
static_assert(sizeof(ScanCand) == sizeof(cl_scan_candidate) && sizeof(cl_scan_candidate) == 28 && SCAN_AT4(ScanCand, cl_scan_candidate, pos, ref, alt, pad) &&
              SCAN_AT4(ScanCand, cl_scan_candidate, a, c, g, t) && SCAN_AT(ScanCand, cl_scan_candidate, depth, depth), "the device writes cl_scan_candidate");
static_assert(sizeof(ScanCandEx) == sizeof(cl_scan_candidate_ex) && sizeof(cl_scan_candidate_ex) == 44 && SCAN_AT4(ScanCandEx, cl_scan_candidate_ex, pos, ref, alt, pad) &&
              SCAN_AT4(ScanCandEx, cl_scan_candidate_ex, a, c, g, t) && SCAN_AT(ScanCandEx, cl_scan_candidate_ex, depth, depth) &&
              SCAN_AT4(ScanCandEx, cl_scan_candidate_ex, alt_fwd, alt_rev, ref_fwd, ref_rev), "the device writes cl_scan_candidate_ex");
static_assert(sizeof(ScanMinorCand) == sizeof(cl_minor_candidate) && sizeof(cl_minor_candidate) == 44 && SCAN_AT4(ScanMinorCand, cl_minor_candidate, pos, ref, major, minor) &&
              SCAN_AT4(ScanMinorCand, cl_minor_candidate, a, c, g, t) && SCAN_AT(ScanMinorCand, cl_minor_candidate, pad, pad) && SCAN_AT(ScanMinorCand, cl_minor_candidate, depth, depth) &&
              SCAN_AT4(ScanMinorCand, cl_minor_candidate, major_fwd, major_rev, minor_fwd, minor_rev), "the device writes cl_minor_candidate");
static_assert(SCAN_COUNT_AS(cl_del_candidate, del), "the device writes cl_del_candidate");
static_assert(SCAN_COUNT_AS(cl_ins_candidate, ins), "the device writes cl_ins_candidate");
static_assert(sizeof(ScanInsObs) == sizeof(cl_ins_obs) && sizeof(cl_ins_obs) == 32 && SCAN_AT4(ScanInsObs, cl_ins_obs, pos, len, key, strand) && SCAN_AT(ScanInsObs, cl_ins_obs, pad, pad),
              "the device writes cl_ins_obs");
#undef SCAN_COUNT_AS
#undef SCAN_AT4
#undef SCAN_AT
static_assert(sizeof(ScanInsSite) == 16, "one called position of the allele launch");
static_assert(CONS_LOW_DEPTH == 0 && CONS_DELETED == 1 && CONS_NO_CALL == 2 && CONS_REF == 3 && CONS_ALT == 4, "the classes of cl_cons_result, in its order");

// the argument checks every scan shares, in front of any device work
static cl_status site_scan_check(SiteCtx *c, const char *who, uint32_t start, uint32_t end)
{
    if (c->host_only) return fail(c, CL_ERR_DEVICE, "a host-only context has no device");
    const SiteResident &S = c->site;
    if (!S.resident) return fail(c, CL_ERR_INVALID, std::string(who) + " without cl_site_upload");
    if (S.filtered) return fail(c, CL_ERR_INVALID, std::string(who) + ": the resident tile was uploaded by cl_site_pileup for its own site list; cl_site_upload gives a tile that serves a scan");
    if (start > end) return fail(c, CL_ERR_INVALID, std::string(who) + ": start > end");
    if (end > S.contig_len) return fail(c, CL_ERR_INVALID, std::string(who) + ": the range ends beyond the contig");
    return CL_OK;
}

// the per-read ends and per-window read ranges of the resident tile: one kernel, the first time a scan asks
static cl_status site_scan_index(SiteCtx *c)
{
    SiteResident &S = c->site;
    if (S.scan_indexed) return CL_OK;
    const size_t n_win = ((size_t)S.contig_len + kScanWin - 1) / kScanWin;
    HIP_TRY(c, S.sc_end.reserve(S.n + 1)); HIP_TRY(c, S.sc_wfirst.reserve(n_win + 1)); HIP_TRY(c, S.sc_wlast.reserve(n_win + 1));
    HIP_TRY(c, hipMemsetAsync(S.sc_wfirst.p, 0xFF, (n_win + 1) * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(S.sc_wlast.p, 0, (n_win + 1) * 4, c->stream));
    if (S.n) {
        ScanIndexArgs A;
        A.rec = S.rec.p; A.cigar = S.cig.p; A.n = (uint32_t)S.n; A.contig_len = S.contig_len;
        A.end = S.sc_end.p; A.wfirst = S.sc_wfirst.p; A.wlast = S.sc_wlast.p;
        hipLaunchKernelGGL(k_site_scan_index, dim3((uint32_t)((S.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, A);
        HIP_TRY(c, hipGetLastError());
    }
    S.scan_indexed = true;
    return CL_OK;
}

// what the host path of the two forms differs in: the filter argument (none, or the caller's cl_scan_filter), the tile
// bytes a scan reads, and the names and laps of the entry points that exist once per form
template <bool FILTERED> struct ScanHost;
template <> struct ScanHost<false> {
    using Filter = ScanNoFilter;
    static constexpr const char *kScan = "cl_site_scan", *kCounts = "cl_site_scan_counts";
    static constexpr const char *kLap = "site scan: reference in, kernel, candidates back";
    static constexpr const char *kLapSettle = "site scan: ambiguous positions settled by the site pileup";
    static uint64_t tile_bytes(const SiteResident &S) { return (S.nbase + 1) / 2 + S.n * (sizeof(SiteRec) + 4) + S.ncig * 4; }
};
template <> struct ScanHost<true> {
    using Filter = const cl_scan_filter *;
    static constexpr const char *kScan = "cl_site_scan_ex", *kCounts = "cl_site_scan_counts_ex";
    static constexpr const char *kLap = "filtered site scan: reference in, kernel, candidates back";
    static constexpr const char *kLapSettle = "filtered site scan: ambiguous positions settled";
    // those of cl_site_scan, the pass bits and the flags
    static uint64_t tile_bytes(const SiteResident &S) { return ScanHost<false>::tile_bytes(S) + (S.nbase + 7) / 8 + S.n * 2; }
};

// site_scan_check and, for the filtered form, its filter and the attachment
template <bool FILTERED>
static cl_status site_scan_check_form(SiteCtx *c, const char *who, typename ScanHost<FILTERED>::Filter f, uint32_t start, uint32_t end)
{
    cl_status s = site_scan_check(c, who, start, end);
    if (s != CL_OK) return s;
    if constexpr (FILTERED) {
        if (!f) return fail(c, CL_ERR_INVALID, std::string(who) + ": null filter");
        if (!c->site.attached) return fail(c, CL_ERR_INVALID, std::string(who) + " without cl_site_attach_quals on the resident tile");
    }
    return CL_OK;
}

template <bool FILTERED, class Args>
static void site_scan_fill(SiteCtx *c, Args &A, typename ScanHost<FILTERED>::Filter f, uint8_t min_quality, uint32_t min_depth,
                           uint32_t start, uint32_t end)
{
    SiteResident &S = c->site;
    A.s.rec = S.rec.p; A.s.seq_base = S.base.p; A.s.cigar = S.cig.p; A.s.seq4 = S.seq.p;
    A.s.end = S.sc_end.p; A.s.wfirst = S.sc_wfirst.p; A.s.wlast = S.sc_wlast.p;
    A.s.min_quality = min_quality; A.s.contig_len = S.contig_len; A.s.min_depth = min_depth; A.s.ref_len = S.ref_len;
    A.s.start = start; A.s.end_pos = end; A.s.win0 = start / kScanWin;
    A.s.refb = nullptr; A.s.cls = nullptr; A.s.n_cand = nullptr; A.s.cand_cap = 0; A.s.dense = nullptr;
    A.cand = nullptr;
    if constexpr (FILTERED) {
        A.f.flag = S.q_flag.p; A.f.pass = S.q_pass.p; A.f.exclude_flags = f->exclude_flags; A.f.use_bq = f->use_base_quality ? 1u : 0u;
    }
}

// The 16-code histograms of the positions the counter planes cannot classify (site_scan.hip.h).  Unfiltered: those of
// cl_site_run.  Filtered: k_site_scan_settle under the filter of A (cl_site_run's histogram is unfiltered).
template <bool FILTERED>
static cl_status site_scan_hist16(SiteCtx *c, const ScanModeArgs<FILTERED, SCAN_CALLS> &A, const std::vector<uint32_t> &pos1, std::vector<uint32_t> &hist)
{
    hist.resize(pos1.size() * 16);
    if constexpr (FILTERED) {
        SiteResident &S = c->site;
        HIP_TRY(c, S.sx_amb.reserve(pos1.size())); HIP_TRY(c, S.sx_hist.reserve(hist.size()));
        HIP_TRY(c, hipMemcpyAsync(S.sx_amb.p, pos1.data(), pos1.size() * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_site_scan_settle, dim3((uint32_t)pos1.size()), dim3(kBlock), 0, c->stream, A, S.sx_amb.p, S.sx_hist.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(hist.data(), S.sx_hist.p, hist.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return CL_OK;
    } else {
        KernelTimer &T = c->site.t_pileup;
        const double ms = T.ms; const uint64_t by = T.bytes;                  // (cl_site_pileup_stats keeps speaking of the caller's own runs)
        const cl_status s = cl_site_run_impl(c, (uint8_t)A.s.min_quality, pos1.data(), pos1.size(), hist.data(), nullptr);
        T.ms = ms; T.bytes = by;
        return s;
    }
}

// settles ambiguous positions from their 16-code histograms: one code with 7/10 of the depth is a call of a code that
// is not A/C/G/T -> uncomparable; otherwise mixed
static void site_scan_settle(const std::vector<uint32_t> &hist, uint64_t &n_unc, uint64_t &n_mixed)
{
    for (size_t i = 0; i < hist.size(); i += 16) {
        uint64_t depth = 0, m = 0;
        for (int k = 0; k < 16; ++k) { depth += hist[i + k]; m = std::max<uint64_t>(m, hist[i + k]); }
        if (10 * m >= 7 * depth) ++n_unc; else ++n_mixed;
    }
}

// What the host path of a compacting mode differs in, beside the kernel's own ScanModeTraits: the C types of its
// result, candidates and parameters; the name in its messages and its lap; where the candidates live -- one host vector
// and one device buffer per result type: those of a scan stay valid until the next call of the same scan; fault(), the
// first of its parameters it refuses, in the order null, min_depth, count, per-10k range; min_depth() and fill(), what it
// sets in the kernel's record behind site_scan_fill; classes(), its class counts out of h_cls; the tile bytes it reads;
// post(), what is left to do behind the sorted candidates (nothing, unless the mode says so).
struct ScanModeHostBase {
    static constexpr const char *kNoDepth = "min_depth must be at least 1";
    template <class... T> static cl_status post(T &&...) { return CL_OK; }
};
template <bool FILTERED, ScanMode MODE> struct ScanModeHost;

template <bool FILTERED> struct ScanModeHost<FILTERED, SCAN_CALLS> : ScanModeHostBase {
    using H = ScanHost<FILTERED>;
    using Result = std::conditional_t<FILTERED, cl_scan_result_ex, cl_scan_result>;
    using Cand = std::conditional_t<FILTERED, cl_scan_candidate_ex, cl_scan_candidate>;
    using Params = uint32_t;                                     // min_depth itself
    static constexpr const char *kWho = H::kScan, *kLap = H::kLap;
    static auto &host_cand(SiteResident &S) { if constexpr (FILTERED) return S.scan_cand_ex; else return S.scan_cand; }
    static auto &dev_cand(SiteResident &S) { if constexpr (FILTERED) return S.sx_cand; else return S.sc_cand; }
    static const char *fault(Params min_depth) { return min_depth == 0 ? kNoDepth : nullptr; }
    static uint32_t min_depth(Params min_depth) { return min_depth; }
    static void fill(ScanModeArgs<FILTERED, SCAN_CALLS> &, Params) {}
    static void classes(Result &out, const unsigned long long (&h)[8])
    {
        out.n_low_depth = h[SCAN_LOW_DEPTH]; out.n_mixed = h[SCAN_MIXED]; out.n_uncomparable = h[SCAN_UNCOMPARABLE];
        out.n_match = h[SCAN_MATCH]; out.n_variant = h[SCAN_VARIANT];
    }
    static uint64_t tile_bytes(const SiteResident &S) { return H::tile_bytes(S); }
    // ambiguous positions leave the list and are settled from their 16-code histograms
    static cl_status post(SiteCtx *c, const ScanModeArgs<FILTERED, SCAN_CALLS> &A, std::vector<Cand> &cand, const unsigned long long (&h)[8],
                          Result &out, StageTimer &tmr)
    {
        if (!h[SCAN_AMBIGUOUS]) return CL_OK;
        std::vector<uint32_t> amb, hist;
        size_t k = 0;
        for (const Cand &cd : cand) { if (cd.alt == 0) amb.push_back(cd.pos); else cand[k++] = cd; }
        cand.resize(k);
        const cl_status s = site_scan_hist16<FILTERED>(c, A, amb, hist);
        if (s != CL_OK) return s;
        site_scan_settle(hist, out.n_uncomparable, out.n_mixed);
        tmr.lap(H::kLapSettle);
        return CL_OK;
    }
};

// the minor mode: a second allele beside the most frequent one (site_scan.hip.h), over either form
template <bool FILTERED> struct ScanModeHost<FILTERED, SCAN_MINOR> : ScanModeHostBase {
    using Result = cl_minor_result;
    using Cand = cl_minor_candidate;
    using Params = const cl_minor_params *;
    static constexpr const char *kWho = "cl_site_scan_minor", *kLap = "minor-allele scan: reference in, kernel, candidates back";
    static std::vector<Cand> &host_cand(SiteResident &S) { return S.minor_cand; }
    static DevBuf<ScanMinorCand> &dev_cand(SiteResident &S) { return S.sm_cand; }
    static const char *fault(Params p)
    {
        return !p ? "null params" : p->min_depth == 0 ? kNoDepth : p->min_minor_count == 0 ? "min_minor_count must be at least 1"
             : (p->min_minor_per_10k < 1 || p->min_minor_per_10k > 5000) ? "min_minor_per_10k must lie in 1..5000" : nullptr;
    }
    static uint32_t min_depth(Params p) { return p->min_depth; }
    static void fill(ScanModeArgs<FILTERED, SCAN_MINOR> &A, Params p) { A.t.min_count = p->min_minor_count; A.t.min_per_10k = p->min_minor_per_10k; }
    static void classes(Result &out, const unsigned long long (&h)[8]) { out.n_low_depth = h[MINOR_LOW_DEPTH]; out.n_single = h[MINOR_SINGLE]; out.n_minor = h[MINOR_MINOR]; }
    static uint64_t tile_bytes(const SiteResident &S) { return ScanHost<FILTERED>::tile_bytes(S); }
};

// The deletion and the insertion mode -- reads whose D operation covers a position, reads with a counting I operation
// anchored at it, each beside the scan's depth under one count rule (site_scan.hip.h) -- have one host definition.  What
// they differ in: their C types, the names of the rule's fields in them, where their candidates live, their messages.
template <ScanMode MODE> struct ScanCountNames;
template <> struct ScanCountNames<SCAN_DELS> {
    using Result = cl_del_result; using Cand = cl_del_candidate; using Rule = cl_del_params;
    static constexpr auto kMinCount = &Rule::min_del_count, kMinPer10k = &Rule::min_del_per_10k;
    static constexpr auto kCalled = &Result::n_deleted;
    static constexpr auto kHostCand = &SiteResident::del_cand;
    static constexpr auto kDevCand = &SiteResident::sd_cand;
    static constexpr const char *kWho = "cl_site_scan_dels", *kLap = "deletion scan: reference in, kernel, candidates back";
    static constexpr const char *kNoCount = "min_del_count must be at least 1", *kPer10kRange = "min_del_per_10k must lie in 1..10000";
};
template <> struct ScanCountNames<SCAN_INS> {
    using Result = cl_ins_result; using Cand = cl_ins_candidate; using Rule = cl_ins_params;
    static constexpr auto kMinCount = &Rule::min_ins_count, kMinPer10k = &Rule::min_ins_per_10k;
    static constexpr auto kCalled = &Result::n_inserted;
    static constexpr auto kHostCand = &SiteResident::ins_cand;
    static constexpr auto kDevCand = &SiteResident::si_cand;
    static constexpr const char *kWho = "cl_site_scan_ins", *kLap = "insertion scan: reference in, kernel, candidates back";
    static constexpr const char *kNoCount = "min_ins_count must be at least 1", *kPer10kRange = "min_ins_per_10k must lie in 1..10000";
};

// the first parameter of a count rule that is refused, under the names N: p is any of the records that hold one
// (cl_del_params, cl_ins_params; cl_cons_params, whose rule is the deletion mode's)
template <class N, class P>
static const char *scan_count_fault(const P *p, uint32_t P::*min_count, uint32_t P::*min_per_10k)
{
    return !p ? "null params" : p->min_depth == 0 ? ScanModeHostBase::kNoDepth : p->*min_count == 0 ? N::kNoCount
         : (p->*min_per_10k < 1 || p->*min_per_10k > 10000) ? N::kPer10kRange : nullptr;
}

template <bool FILTERED, ScanMode MODE> struct ScanCountHost : ScanModeHostBase, ScanCountNames<MODE> {
    using N = ScanCountNames<MODE>;
    using Params = const typename N::Rule *;
    static auto &host_cand(SiteResident &S) { return S.*N::kHostCand; }
    static auto &dev_cand(SiteResident &S) { return S.*N::kDevCand; }
    static const char *fault(Params p) { return scan_count_fault<N>(p, N::kMinCount, N::kMinPer10k); }
    static uint32_t min_depth(Params p) { return p->min_depth; }
    static void fill(ScanModeArgs<FILTERED, MODE> &A, Params p) { A.t.min_count = p->*N::kMinCount; A.t.min_per_10k = p->*N::kMinPer10k; }
    static void classes(typename N::Result &out, const unsigned long long (&h)[8]) { out.n_low_depth = h[COUNT_LOW_DEPTH]; out.n_kept = h[COUNT_KEPT]; out.*N::kCalled = h[COUNT_CALLED]; }
    // the tile without its bases: records, ends, CIGAR words; under a filter the flags and the pass bits
    static uint64_t tile_bytes(const SiteResident &S) { return S.n * (sizeof(SiteRec) + 4) + S.ncig * 4 + (FILTERED ? (S.nbase + 7) / 8 + S.n * 2 : 0); }
};
template <bool FILTERED> struct ScanModeHost<FILTERED, SCAN_DELS> : ScanCountHost<FILTERED, SCAN_DELS> {};

// behind the insertion mode's candidates a second launch over them alone fetches what was inserted (site_scan.hip.h)
template <bool FILTERED> struct ScanModeHost<FILTERED, SCAN_INS> : ScanCountHost<FILTERED, SCAN_INS> {
    using Result = cl_ins_result;
    using Cand = cl_ins_candidate;
    // The observations: the candidates' positions with the exclusive prefix sum of their ins go to the device, one
    // workgroup per candidate stores its insertions into its own slots of a buffer of exactly sum(ins) entries and says
    // how many it found.  t_scan and its bytes become those of both launches.
    static cl_status post(SiteCtx *c, const ScanModeArgs<FILTERED, SCAN_INS> &A, std::vector<Cand> &cand, const unsigned long long (&)[8],
                          Result &out, StageTimer &tmr)
    {
        SiteResident &S = c->site;
        std::vector<cl_ins_obs> &obs = S.ins_obs;
        obs.clear();
        S.ins_scan_ms = S.t_scan.ms; S.ins_alleles_ms = 0.0;
        out.n_obs = 0; out.obs = obs.data();
        if (cand.empty()) return CL_OK;
        std::vector<ScanInsSite> site(cand.size());
        uint64_t n_obs = 0;
        for (size_t i = 0; i < cand.size(); ++i) { site[i] = {cand[i].pos, cand[i].ins, n_obs}; n_obs += cand[i].ins; }
        std::vector<uint32_t> found(cand.size());
        HIP_TRY(c, S.si_site.reserve(site.size())); HIP_TRY(c, S.si_found.reserve(site.size())); HIP_TRY(c, S.si_obs.reserve(n_obs));
        HIP_TRY(c, hipMemcpyAsync(S.si_site.p, site.data(), site.size() * sizeof(ScanInsSite), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, S.t_scan.start(c->stream));
        for (size_t at = 0; at < site.size(); at += (size_t)1 << 30) {          // (a grid holds fewer than 2^31 workgroups)
            const uint32_t n = (uint32_t)std::min<size_t>(site.size() - at, (size_t)1 << 30);
            hipLaunchKernelGGL((k_site_scan_ins_alleles<FILTERED>), dim3(n), dim3(kBlock), 0, c->stream, A, S.si_site.p + at, S.si_obs.p, S.si_found.p + at);
            HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, S.t_scan.stop(c->stream));
        HIP_TRY(c, hipMemcpyAsync(found.data(), S.si_found.p, found.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, S.t_scan.read(true));
        S.ins_alleles_ms = S.t_scan.ms - S.ins_scan_ms;
        for (size_t i = 0; i < cand.size(); ++i)
            if (found[i] != cand[i].ins)
                return fail(c, CL_ERR_INTERNAL, "cl_site_scan_ins: the allele launch found " + std::to_string(found[i]) + " insertions at position " +
                                                    std::to_string(cand[i].pos) + " where the scan counted " + std::to_string(cand[i].ins));
        obs.resize(n_obs);
        if (n_obs) HIP_TRY(c, hipMemcpy(obs.data(), S.si_obs.p, n_obs * sizeof(cl_ins_obs), hipMemcpyDeviceToHost));
        // (of the tile the allele launch reads a window's records per candidate and the inserted bases: not counted)
        S.t_scan.bytes += site.size() * (sizeof(ScanInsSite) + 4) + n_obs * sizeof(cl_ins_obs);
        tmr.lap("insertion scan: observations of the called positions back");
        // the slots of a position fill in the order its reads arrive: the order of the result is restored here
        std::sort(obs.begin(), obs.end(), [](const cl_ins_obs &a, const cl_ins_obs &b) {
            if (a.pos != b.pos) return a.pos < b.pos;
            if (a.len != b.len) return a.len < b.len;
            if (a.key[0] != b.key[0]) return a.key[0] < b.key[0];
            if (a.key[1] != b.key[1]) return a.key[1] < b.key[1];
            return a.strand < b.strand;
        });
        out.n_obs = n_obs; out.obs = obs.data();
        return CL_OK;
    }
};

// What every scan with a reference checks behind its own null result, in this order: site_scan_check_form, the mode's
// parameters (fault: the first one it refuses, or null), the reference's length and pointer
template <bool FILTERED>
static cl_status site_scan_enter(SiteCtx *c, const char *who_c, typename ScanHost<FILTERED>::Filter filter, const char *fault, const uint8_t *ref_bases,
                                 uint64_t ref_len, uint32_t start, uint32_t end)
{
    const std::string who = who_c;
    const cl_status s = site_scan_check_form<FILTERED>(c, who_c, filter, start, end);
    if (s != CL_OK) return s;
    if (fault) return fail(c, CL_ERR_INVALID, who + ": " + fault);
    if (ref_len != c->site.ref_len) return fail(c, CL_ERR_INVALID, who + ": ref_len differs from the one given to cl_site_upload");
    if (!ref_bases && ref_len) return fail(c, CL_ERR_INVALID, who + ": null reference");
    return CL_OK;
}

// the reference bytes of the range to the device (those that exist: positions at and beyond ref_len read as "other") and
// the class counters' buffer; n_ref: the bytes sent
static cl_status site_scan_reference(SiteCtx *c, const uint8_t *ref_bases, uint64_t ref_len, uint32_t start, uint32_t end, uint64_t &n_ref)
{
    SiteResident &S = c->site;
    const uint64_t ref_hi = std::min<uint64_t>(end, ref_len);
    n_ref = ref_hi > start ? ref_hi - start : 0;
    HIP_TRY(c, S.sc_ref.reserve(n_ref + 16)); HIP_TRY(c, S.sc_cls.reserve(8));
    if (n_ref) HIP_TRY(c, hipMemcpyAsync(S.sc_ref.p, ref_bases + start, n_ref, hipMemcpyHostToDevice, c->stream));
    return CL_OK;
}

// one launch of k_site_scan over n_blocks windows between the events of t_scan, behind cleared class counters (if it has any)
template <bool FILTERED, ScanMode MODE>
static cl_status site_scan_launch(SiteCtx *c, const ScanModeArgs<FILTERED, MODE> &A, uint32_t n_blocks)
{
    KernelTimer &T = c->site.t_scan;
    if (A.s.cls) HIP_TRY(c, hipMemsetAsync(A.s.cls, 0, 8 * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, T.start(c->stream));
    hipLaunchKernelGGL((k_site_scan<FILTERED, MODE>), dim3(n_blocks), dim3(kBlock), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, T.stop(c->stream));
    return CL_OK;
}

// A scan that compacts candidates, of any mode and form: the checks, the index, the reference bytes of the range, the
// kernel until the candidates fit, the candidates back and in ascending position, the mode's post step.
template <bool FILTERED, ScanMode MODE>
static cl_status site_scan_run(SiteCtx *c, uint8_t min_quality, typename ScanHost<FILTERED>::Filter filter, typename ScanModeHost<FILTERED, MODE>::Params prm,
                               const uint8_t *ref_bases, uint64_t ref_len, uint32_t start, uint32_t end, typename ScanModeHost<FILTERED, MODE>::Result *out)
{
    using M = ScanModeHost<FILTERED, MODE>;
    using Cand = typename M::Cand;
    if (!c) return CL_ERR_INVALID;
    const std::string who = M::kWho;
    if (!out) return fail(c, CL_ERR_INVALID, who + ": null result");
    cl_status s = site_scan_enter<FILTERED>(c, M::kWho, filter, M::fault(prm), ref_bases, ref_len, start, end);
    if (s != CL_OK) return s;
    SiteResident &S = c->site;
    std::vector<Cand> &cand = M::host_cand(S);
    auto &d_cand = M::dev_cand(S);
    memset(out, 0, sizeof(*out));
    out->start = start; out->end = end;
    cand.clear();
    out->candidates = cand.data();
    S.t_scan.ms = 0.0; S.t_scan.bytes = 0;
    if (start == end) return CL_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    StageTimer tmr;
    if ((s = site_scan_index(c)) != CL_OK) return s;
    uint64_t n_ref = 0;
    if ((s = site_scan_reference(c, ref_bases, ref_len, start, end, n_ref)) != CL_OK) return s;
    const uint32_t n_blocks = (end - 1) / kScanWin - start / kScanWin + 1;
    // candidates are few where the sample follows the reference: a buffer of a position in 64 (at least 64 K entries);
    // when more are wanted the kernel says how many, the buffer grows and the scan runs again -- nothing is cut short
    uint64_t cap = std::max<uint64_t>(65536, (uint64_t)(end - start) / 64);
    unsigned long long h_cls[8];                                 // the class counts, then the candidates wanted
    ScanModeArgs<FILTERED, MODE> A;
    for (;;) {
        HIP_TRY(c, d_cand.reserve(cap));
        // (the record is filled once the index and every buffer stand)
        site_scan_fill<FILTERED>(c, A, filter, min_quality, M::min_depth(prm), start, end);
        M::fill(A, prm);
        A.s.refb = S.sc_ref.p; A.s.cls = S.sc_cls.p; A.s.n_cand = reinterpret_cast<uint32_t *>(S.sc_cls.p + SCAN_CLASSES);
        A.cand = d_cand.p; A.s.cand_cap = (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull);
        if ((s = site_scan_launch(c, A, n_blocks)) != CL_OK) return s;
        HIP_TRY(c, hipMemcpyAsync(h_cls, S.sc_cls.p, sizeof(h_cls), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, S.t_scan.read(true));                         // (a scan that ran again: the launches' sum)
        const uint64_t want = (uint32_t)h_cls[SCAN_CLASSES];
        if (want <= cap) break;
        cap = want;
    }
    const uint64_t n_cand = (uint32_t)h_cls[SCAN_CLASSES];
    cand.resize(n_cand);
    if (n_cand) HIP_TRY(c, hipMemcpy(cand.data(), d_cand.p, n_cand * sizeof(Cand), hipMemcpyDeviceToHost));
    S.t_scan.bytes = M::tile_bytes(S) + n_ref + n_cand * sizeof(Cand);
    tmr.lap(M::kLap);
    // the compaction runs wave by wave: ascending position is restored here
    std::sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) { return a.pos < b.pos; });
    M::classes(*out, h_cls);
    if ((s = M::post(c, A, cand, h_cls, *out, tmr)) != CL_OK) return s;
    out->candidates = cand.data();
    return CL_OK;
}

// a mode whose filter may be null: that is its unfiltered form
template <ScanMode MODE, class... Rest>
static cl_status site_scan_either(SiteCtx *c, uint8_t min_quality, const cl_scan_filter *filter, Rest... rest)
{
    if (filter) return site_scan_run<true, MODE>(c, min_quality, filter, rest...);
    return site_scan_run<false, MODE>(c, min_quality, ScanNoFilter{}, rest...);
}

// The consensus scan, of either form: one launch, one byte per position, five class counts.  It compacts nothing, so
// there is no candidate buffer and nothing to grow: the checks, the index, the reference and the record's fill are those
// of site_scan_run; the device buffer holds whole windows from the first one's start and the range is copied out of it.
template <bool FILTERED>
static cl_status site_scan_consensus_run(SiteCtx *c, uint8_t min_quality, typename ScanHost<FILTERED>::Filter filter, const cl_cons_params *prm,
                                         const uint8_t *ref_bases, uint64_t ref_len, uint32_t start, uint32_t end, cl_cons_result *out)
{
    static constexpr const char *kWho = "cl_site_scan_consensus";
    if (!c) return CL_ERR_INVALID;
    if (!out) return fail(c, CL_ERR_INVALID, std::string(kWho) + ": null result");
    // (the deletion rule's parameters, refused as cl_site_scan_dels refuses them)
    const char *fault = scan_count_fault<ScanCountNames<SCAN_DELS>>(prm, &cl_cons_params::min_del_count, &cl_cons_params::min_del_per_10k);
    cl_status s = site_scan_enter<FILTERED>(c, kWho, filter, fault, ref_bases, ref_len, start, end);
    if (s != CL_OK) return s;
    SiteResident &S = c->site;
    memset(out, 0, sizeof(*out));
    out->start = start; out->end = end;
    S.cons_bytes.resize((size_t)(end - start));                 // (a second call over as many positions fills nothing in)
    out->cons = S.cons_bytes.data();
    S.t_scan.ms = 0.0; S.t_scan.bytes = 0;
    if (start == end) return CL_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    StageTimer tmr;
    if ((s = site_scan_index(c)) != CL_OK) return s;
    uint64_t n_ref = 0;
    if ((s = site_scan_reference(c, ref_bases, ref_len, start, end, n_ref)) != CL_OK) return s;
    const uint32_t win0 = start / kScanWin, n_blocks = (end - 1) / kScanWin - win0 + 1;
    HIP_TRY(c, S.sk_cons.reserve((size_t)n_blocks * kBlock));
    ScanModeArgs<FILTERED, SCAN_CONS> A;
    site_scan_fill<FILTERED>(c, A, filter, min_quality, prm->min_depth, start, end);
    A.t.min_count = prm->min_del_count; A.t.min_per_10k = prm->min_del_per_10k;
    A.s.refb = S.sc_ref.p; A.s.cls = S.sc_cls.p; A.cand = S.sk_cons.p;
    if ((s = site_scan_launch(c, A, n_blocks)) != CL_OK) return s;
    unsigned long long h_cls[8];
    HIP_TRY(c, hipMemcpyAsync(h_cls, S.sc_cls.p, sizeof(h_cls), hipMemcpyDeviceToHost, c->stream));
    // the range's bytes: the buffer's byte 0 is position win0 * kScanWin
    HIP_TRY(c, hipMemcpyAsync(S.cons_bytes.data(), reinterpret_cast<const uint8_t *>(S.sk_cons.p) + (start - win0 * kScanWin), (size_t)(end - start),
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, S.t_scan.read());
    S.t_scan.bytes = ScanHost<FILTERED>::tile_bytes(S) + n_ref + (uint64_t)(end - start);
    tmr.lap("consensus scan: reference in, kernel, bytes back");
    out->n_low_depth = h_cls[CONS_LOW_DEPTH]; out->n_deleted = h_cls[CONS_DELETED]; out->n_no_call = h_cls[CONS_NO_CALL];
    out->n_ref = h_cls[CONS_REF]; out->n_alt = h_cls[CONS_ALT];
    out->cons = S.cons_bytes.data();
    return CL_OK;
}

template <bool FILTERED>
static cl_status site_scan_counts_impl(SiteCtx *c, uint8_t min_quality, typename ScanHost<FILTERED>::Filter filter, uint32_t start, uint32_t end,
                                       uint32_t *counts)
{
    using H = ScanHost<FILTERED>;
    if (!c) return CL_ERR_INVALID;
    cl_status s = site_scan_check_form<FILTERED>(c, H::kCounts, filter, start, end);
    if (s != CL_OK) return s;
    if (end - start > CL_SCAN_MAX_DENSE) return fail(c, CL_ERR_INVALID, std::string(H::kCounts) + ": more than CL_SCAN_MAX_DENSE positions");
    c->site.t_scan.ms = 0.0; c->site.t_scan.bytes = 0;
    if (start == end) return CL_OK;
    if (!counts) return fail(c, CL_ERR_INVALID, std::string(H::kCounts) + ": null array");
    SiteResident &S = c->site;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((s = site_scan_index(c)) != CL_OK) return s;
    const size_t n_dense = (size_t)(end - start) * ScanForm<FILTERED>::kDense;
    HIP_TRY(c, S.sc_dense.reserve(n_dense));
    ScanModeArgs<FILTERED, SCAN_DENSE> A;
    site_scan_fill<FILTERED>(c, A, filter, min_quality, 1, start, end);
    A.s.dense = S.sc_dense.p;
    if ((s = site_scan_launch(c, A, (end - 1) / kScanWin - start / kScanWin + 1)) != CL_OK) return s;
    HIP_TRY(c, hipMemcpyAsync(counts, S.sc_dense.p, n_dense * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, S.t_scan.read());
    S.t_scan.bytes = H::tile_bytes(S) + n_dense * 4;
    return CL_OK;
}

// ---- the attachment of the filtered form ----
static cl_status site_quals_check(const cl_site_quals *q, std::string &why)
{
    if (!q) { why = "null attachment"; return CL_ERR_INVALID; }
    if (!q->qual_off || !q->seq_off || (q->n_reads && !q->flag)) { why = "null attachment array"; return CL_ERR_INVALID; }
    std::atomic<int> bad{0};
    dut::parallel_for(q->n_reads, 262144, [&](size_t i) { if (q->qual_off[i + 1] < q->qual_off[i] || q->seq_off[i + 1] < q->seq_off[i]) bad = 1; });
    if (bad) { why = "offset arrays must be non-decreasing"; return CL_ERR_INVALID; }
    if (q->qual_off[q->n_reads] > q->qual_off[0] && !q->qual) { why = "null quality array"; return CL_ERR_INVALID; }
    return CL_OK;
}

// an entry point's body over the site engine's view of the handle, behind the guard of the C ABI
template <class F> static cl_status site_entry(cl_ctx *h, F &&f)
{
    SiteCtx *c = site_ctx(h);
    return guarded(c, [&] { return f(c); });
}

#include "site_str.hip.h"
#include "site_errors.hip.h"
#include "site_links.hip.h"

extern "C" {

cl_status cl_site_scan(cl_ctx *h, uint8_t min_quality, uint32_t min_depth, const uint8_t *ref_bases, uint64_t ref_len,
                       uint32_t start, uint32_t end, cl_scan_result *out)
{
    return site_entry(h, [&](SiteCtx *c) { return site_scan_run<false, SCAN_CALLS>(c, min_quality, ScanNoFilter{}, min_depth, ref_bases, ref_len, start, end, out); });
}

cl_status cl_site_scan_counts(cl_ctx *h, uint8_t min_quality, uint32_t start, uint32_t end, uint32_t *counts)
{
    return site_entry(h, [&](SiteCtx *c) { return site_scan_counts_impl<false>(c, min_quality, ScanNoFilter{}, start, end, counts); });
}

cl_status cl_site_attach_quals(cl_ctx *h, const cl_site_quals *q, uint8_t min_base_quality)
{
    return site_entry(h, [&](SiteCtx *c) -> cl_status {
        if (!c) return CL_ERR_INVALID;
        if (c->host_only) return fail(c, CL_ERR_DEVICE, "a host-only context has no device");
        SiteResident &S = c->site;
        if (!S.resident) return fail(c, CL_ERR_INVALID, "cl_site_attach_quals without cl_site_upload");
        if (S.filtered) return fail(c, CL_ERR_INVALID, "cl_site_attach_quals: the resident tile was uploaded by cl_site_pileup for its own site list; cl_site_upload gives a tile that serves a scan");
        std::string why;
        if (site_quals_check(q, why) != CL_OK) return fail(c, CL_ERR_INVALID, "cl_site_attach_quals: " + why);
        if (q->n_reads != S.n) return fail(c, CL_ERR_INVALID, "cl_site_attach_quals: n_reads differs from the resident tile's");
        if (q->seq_off[q->n_reads] != S.nbase) return fail(c, CL_ERR_INVALID, "cl_site_attach_quals: seq_off is not the one of the resident tile");
        HIP_TRY(c, hipSetDevice(c->device));
        drop_prefetch(c);                                        // the ring is needed below
        S.attached = false;
        StageTimer tmr;
        const uint64_t n = S.n, n_words = (S.nbase + 63) / 64;
        HIP_TRY(c, S.q_pass.reserve(n_words + 2)); HIP_TRY(c, S.q_flag.reserve(n + 1));
        if (n_words) {
            const cl_site_quals Q = *q;
            cl_status rs = ring_start(c, reinterpret_cast<uint8_t *>(S.q_pass.p), n_words * 8, [Q, min_base_quality](uint64_t off, uint64_t len, uint8_t *out) {
                // (a buffer is a whole number of words)
                dut::site_pass_words(Q.n_reads, Q.seq_off, Q.qual_off, Q.qual, min_base_quality, off / 8, (off + len) / 8, reinterpret_cast<uint64_t *>(out));
            }, PinRing::kPinBytes, PinRing::kCopyThreads);
            if (rs == CL_OK) rs = ring_finish(c); else (void)ring_finish(c);
            if (rs != CL_OK) return rs;
        }
        cl_status rs = CL_OK;
        if (n && (rs = ring_copy(c, S.q_flag.p, q->flag, n * 2)) != CL_OK) return rs;
        tmr.lap("site attach: pass bits + flags");
        S.attached = true;
        return CL_OK;
    });
}

cl_status cl_site_scan_ex(cl_ctx *h, uint8_t min_quality, uint32_t min_depth, const cl_scan_filter *filter, const uint8_t *ref_bases,
                          uint64_t ref_len, uint32_t start, uint32_t end, cl_scan_result_ex *out)
{
    return site_entry(h, [&](SiteCtx *c) { return site_scan_run<true, SCAN_CALLS>(c, min_quality, filter, min_depth, ref_bases, ref_len, start, end, out); });
}

cl_status cl_site_scan_minor(cl_ctx *h, uint8_t min_quality, const cl_scan_filter *filter, const cl_minor_params *params, const uint8_t *ref_bases,
                             uint64_t ref_len, uint32_t start, uint32_t end, cl_minor_result *out)
{
    return site_entry(h, [&](SiteCtx *c) { return site_scan_either<SCAN_MINOR>(c, min_quality, filter, params, ref_bases, ref_len, start, end, out); });
}

cl_status cl_site_scan_dels(cl_ctx *h, uint8_t min_quality, const cl_scan_filter *filter, const cl_del_params *params, const uint8_t *ref_bases,
                            uint64_t ref_len, uint32_t start, uint32_t end, cl_del_result *out)
{
    return site_entry(h, [&](SiteCtx *c) { return site_scan_either<SCAN_DELS>(c, min_quality, filter, params, ref_bases, ref_len, start, end, out); });
}

cl_status cl_site_scan_ins(cl_ctx *h, uint8_t min_quality, const cl_scan_filter *filter, const cl_ins_params *params, const uint8_t *ref_bases,
                           uint64_t ref_len, uint32_t start, uint32_t end, cl_ins_result *out)
{
    return site_entry(h, [&](SiteCtx *c) {
        if (c) c->site.ins_scan_ms = c->site.ins_alleles_ms = 0.0;
        return site_scan_either<SCAN_INS>(c, min_quality, filter, params, ref_bases, ref_len, start, end, out);
    });
}

cl_status cl_site_scan_consensus(cl_ctx *h, uint8_t min_quality, const cl_scan_filter *filter, const cl_cons_params *params, const uint8_t *ref_bases,
                                 uint64_t ref_len, uint32_t start, uint32_t end, cl_cons_result *out)
{
    return site_entry(h, [&](SiteCtx *c) {
        if (filter) return site_scan_consensus_run<true>(c, min_quality, filter, params, ref_bases, ref_len, start, end, out);
        return site_scan_consensus_run<false>(c, min_quality, ScanNoFilter{}, params, ref_bases, ref_len, start, end, out);
    });
}

cl_status cl_site_scan_ins_stats(cl_ctx *h, double *scan_ms, double *alleles_ms)
{
    if (!h) return CL_ERR_INVALID;
    if (scan_ms) *scan_ms = site_ctx(h)->site.ins_scan_ms;
    if (alleles_ms) *alleles_ms = site_ctx(h)->site.ins_alleles_ms;
    return CL_OK;
}

cl_status cl_site_scan_counts_ex(cl_ctx *h, uint8_t min_quality, const cl_scan_filter *filter, uint32_t start, uint32_t end, uint32_t *counts)
{
    return site_entry(h, [&](SiteCtx *c) { return site_scan_counts_impl<true>(c, min_quality, filter, start, end, counts); });
}

cl_status cl_debug_site_pass_bits(const cl_site_quals *quals, uint8_t min_base_quality, uint64_t *words_out, uint64_t n_words)
{
    try {
        std::string why;
        if (site_quals_check(quals, why) != CL_OK || (n_words && !words_out)) return CL_ERR_INVALID;
        dut::site_pass_words(quals->n_reads, quals->seq_off, quals->qual_off, quals->qual, min_base_quality, 0, n_words, words_out);
        return CL_OK;
    }
    catch (...) { return CL_ERR_NOMEM; }
}

cl_status cl_site_scan_stats(cl_ctx *h, double *kernel_ms, uint64_t *bytes)
{
    if (!h) return CL_ERR_INVALID;
    if (kernel_ms) *kernel_ms = site_ctx(h)->site.t_scan.ms;
    if (bytes) *bytes = site_ctx(h)->site.t_scan.bytes;
    return CL_OK;
}

cl_status cl_site_pileup_stats(cl_ctx *h, double *kernel_ms, uint64_t *bytes)
{
    if (!h) return CL_ERR_INVALID;
    if (kernel_ms) *kernel_ms = site_ctx(h)->site.t_pileup.ms;
    if (bytes) *bytes = site_ctx(h)->site.t_pileup.bytes;
    return CL_OK;
}

cl_status cl_site_upload(cl_ctx *h, uint32_t contig_len, uint64_t ref_len, const cl_site_tile *t)
{
    return site_entry(h, [&](SiteCtx *c) { return cl_site_upload_impl(c, contig_len, ref_len, t); });
}

cl_status cl_site_run(cl_ctx *h, uint8_t min_quality, const uint32_t *sites, size_t n_sites, uint32_t *hist)
{
    return site_entry(h, [&](SiteCtx *c) { return cl_site_run_impl(c, min_quality, sites, n_sites, hist, nullptr); });
}

cl_status cl_site_pileup(cl_ctx *h, uint8_t min_quality, uint32_t contig_len, uint64_t ref_len,
                         const cl_site_tile *t, const uint32_t *sites, size_t n_sites, uint32_t *hist)
{
    if (!h || !t || (!sites && n_sites) || (!hist && n_sites)) return CL_ERR_INVALID;
    if (n_sites == 0) return CL_OK;
    return site_entry(h, [&](SiteCtx *c) {
        if (n_sites > 0x0FFFFFFFu) return fail(c, CL_ERR_RANGE, "too many sites");
        // the sorted site list first (a millisecond): it says which reads need to travel at all
        SitePrep prep;
        site_prepare(sites, n_sites, prep);
        SiteGather G;
        static const bool no_filter = [] { const char *e = getenv("DUT_SITE_FILTER"); return e && *e == '0'; }();   // =0: the whole tile travels (A/B, tests)
        if (!no_filter && t->n_reads && t->pos && t->mapq && t->cigar_off && t->seq_off) {
            StageTimer tf;
            site_filter(t, prep, min_quality, contig_len, G);
            tf.lap("site pileup: reads that overlap a site");
        }
        cl_status s = cl_site_upload_impl(c, contig_len, ref_len, t, &G);
        if (s != CL_OK) return s;
        return cl_site_run_impl(c, min_quality, sites, n_sites, hist, &prep);
    });
}

} // extern "C"
