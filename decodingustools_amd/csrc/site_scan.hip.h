// site_scan.hip.h -- the dense form of the site pileup (config 5): base counts and SNV calls at EVERY position of a
// range of the resident site tile (cl_site_upload), instead of at the sites of a list.
//
// k_site_pileup (kernels.hip.h) is built for a sparse list: one thread per read, a read leaves at once when no site
// lies in its span, 64 sites per workgroup in LDS.  With a site at every base none of that helps, and the histogram
// (64 bytes per position) has to cross HBM and the link.  Here a workgroup owns a window of kScanWin reference positions:
// it counts the bases of every read over the window in LDS, applies the calling rule of caller.rs:132-149 there and
// writes back only the positions that differ from the reference (or, in the dense mode, five counters per position).
//
// Per position the semantics are those of k_site_pileup, condition by condition (hist[p][c] of cl_site_run for the
// 1-based site p + 1): read start < contig_len, mapq >= min_quality, bases of M/=/X operations, query index < l_seq,
// p < ref_len; no flag or base-quality filter.
//
// Two kernels:
//   k_site_scan_index   once per resident tile: the reference end of every read and, per window, the index range
//                       [first, last) of the reads that overlap it (atomicMin / atomicMax of the read's index over
//                       the windows of its span).  The range holds every overlapping read whatever the order of the
//                       tile, so an unsorted tile gives exact counts too -- its ranges are merely wider.
//   k_site_scan<DENSE>  one workgroup per window: reads of the window's range are dealt to the threads, a thread walks
//                       its read's CIGAR over the window and adds into six LDS counter planes (A, C, G, T, N, any other
//                       code; one ds_add without return per base, consecutive positions in consecutive banks); then
//                       every thread classifies positions and the candidates are compacted with one ballot and one
//                       atomic per wave.
//
// Six planes and not sixteen: depth = their sum, and the call needs the largest single code.  That is one of the five
// named planes unless the codes of the sixth plane (=, IUPAC ambiguity codes) together reach 7/10 of the depth; such a
// position cannot be classified from six counters (one code with 7/10 is "uncomparable", several that share it are
// "mixed").  It is reported as ambiguous and the host settles it with the 16-code histogram of cl_site_run.
#pragma once

#include "kernels.hip.h"

namespace clk {

constexpr uint32_t kScanWin = 1024;          // positions per workgroup: 6 planes x 1024 x 4 B = 24 KB of LDS, 6 workgroups per CU
constexpr uint32_t kScanPlanes = 6;          // A C G T N other
enum { SCAN_LOW_DEPTH = 0, SCAN_MIXED = 1, SCAN_UNCOMPARABLE = 2, SCAN_MATCH = 3, SCAN_VARIANT = 4, SCAN_AMBIGUOUS = 5, SCAN_CLASSES = 6 };

// one compacted position: a variant (alt = 'A' 'C' 'G' 'T') or an ambiguous one (alt = 0, settled by the host)
struct ScanCand {
    uint32_t pos;                            // 1-based
    uint8_t  ref, alt, pad[2];
    uint32_t a, c, g, t, depth;
};

struct ScanIndexArgs {
    const SiteRec *rec;                      // n + 1
    const uint32_t *cigar;                   // padded by 8 words
    uint32_t n, contig_len;
    uint32_t *end;                           // n: pos + reference span, clamped to 2^32 - 1; 0 for a read that never counts
    uint32_t *wfirst, *wlast;                // per window of kScanWin positions of the contig: preset to 0xFFFFFFFF / 0
};

struct ScanArgs {
    const SiteRec *rec;
    const unsigned long long *seq_base;      // per kBlock reads: base offset of the first one
    const uint32_t *cigar;
    const uint8_t  *seq4;
    const uint32_t *end, *wfirst, *wlast;
    uint32_t min_quality, contig_len, min_depth;
    unsigned long long ref_len;
    uint32_t start, end_pos;                 // the range, 0-based half open, end_pos <= contig_len
    uint32_t win0;                           // window of blockIdx.x == 0
    const uint8_t *refb;                     // reference bytes of [start, min(end_pos, ref_len)), refb[0] <-> start
    unsigned long long *cls;                 // SCAN_CLASSES counts
    uint32_t *n_cand;                        // candidates wanted (also beyond cand_cap)
    ScanCand *cand;
    uint32_t cand_cap;
    uint32_t *dense;                         // DENSE: (end_pos - start) * 5: A C G T depth
};

// number of CIGAR operations and bases of a read, with SiteRec's escape to the next record's offsets
__device__ __forceinline__ void scan_read_extent(const SiteRec *rec, uint32_t r, const uint4 &rr, uint32_t &k1, unsigned long long &slen)
{
    k1 = rr.y + ((rr.w >> 8) & 255u);
    slen = rr.w >> 16;
    if (((rr.w >> 8) & 255u) == 255u || slen == 0xFFFFull) {
        const uint4 nx = *reinterpret_cast<const uint4 *>(rec + r + 1);
        k1 = nx.y; slen = (uint32_t)(nx.z - rr.z);
    }
}

__global__ __launch_bounds__(kBlock) void k_site_scan_index(ScanIndexArgs a)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= a.n) return;
    const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
    uint32_t e = 0;
    if ((uint32_t)rr.x < a.contig_len) {                                    // fetch("chr:1-len"), caller.rs:33-36
        uint32_t k1; unsigned long long slen;
        scan_read_extent(a.rec, r, rr, k1, slen);
        unsigned long long reflen = 0;
        for (uint32_t kk = rr.y; kk < k1; ++kk) {
            const uint32_t c = a.cigar[kk];
            reflen += ((0x18Du >> (c & 15u)) & 1u) ? (c >> 4) : 0u;
        }
        if (reflen) {
            const unsigned long long x = (uint32_t)rr.x, xe = x + reflen;
            e = xe > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)xe;
            const uint32_t last_p = (e > a.contig_len ? a.contig_len : e) - 1u;   // x < contig_len and e > x: >= x
            for (uint32_t w = (uint32_t)x / kScanWin; w <= last_p / kScanWin; ++w) {
                atomicMin(&a.wfirst[w], r);
                atomicMax(&a.wlast[w], r + 1u);
            }
        }
    }
    a.end[r] = e;
}

__device__ __forceinline__ uint32_t scan_plane(uint32_t code)
{
    return code == 1u ? 0u : code == 2u ? 1u : code == 4u ? 2u : code == 8u ? 3u : code == 15u ? 4u : 5u;
}

template <bool DENSE>
__global__ __launch_bounds__(kBlock) void k_site_scan(ScanArgs a)
{
    __shared__ uint32_t s_cnt[kScanPlanes * kScanWin];
    __shared__ unsigned long long s_cls[SCAN_CLASSES];
    const uint32_t tid = threadIdx.x;
    const uint32_t w = a.win0 + blockIdx.x;
    const unsigned long long ws64 = (unsigned long long)w * kScanWin;
    // the part of the window that is asked for and that can hold a count (p < ref_len, caller.rs:110-113)
    const uint32_t ws = (uint32_t)ws64;
    const uint32_t lo = ws > a.start ? ws : a.start;
    const uint32_t we = (ws64 + kScanWin < (unsigned long long)a.end_pos) ? ws + kScanWin : a.end_pos;   // lo <= we: the host launches overlapping windows only
    const uint32_t hi = (unsigned long long)we < a.ref_len ? we : (uint32_t)a.ref_len;
    for (uint32_t i = tid; i < kScanPlanes * kScanWin; i += kBlock) s_cnt[i] = 0;
    if (tid < (uint32_t)SCAN_CLASSES) s_cls[tid] = 0;
    __syncthreads();
    const uint32_t r_first = a.wfirst[w], r_last = a.wlast[w];
    if (r_first < r_last && lo < hi) {
        for (uint32_t r = r_first + tid; r < r_last; r += kBlock) {
            const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
            const uint32_t e = a.end[r];
            // read start < contig_len (end = 0 otherwise), the mapping-quality gate (caller.rs:80), overlap with [lo, hi)
            if ((rr.w & 255u) < a.min_quality || e <= lo || (uint32_t)rr.x >= hi) continue;
            uint32_t k1; unsigned long long slen;
            scan_read_extent(a.rec, r, rr, k1, slen);
            const unsigned long long base = a.seq_base[r / kBlock];
            const unsigned long long s0 = base + (uint32_t)(rr.z - (uint32_t)base);
            unsigned long long x = (uint32_t)rr.x, y = 0;
            for (uint32_t kk = rr.y; kk < k1 && x < hi; ++kk) {
                const uint32_t c = a.cigar[kk];
                const uint32_t op = c & 15u, l = c >> 4;
                if (op_match(op)) {
                    // [x, x + l) cut to [lo, hi) and to the bases the read has (query index < l_seq, caller.rs:105)
                    unsigned long long p0 = x > lo ? x : lo, p1 = x + l < hi ? x + l : hi;
                    if (y < slen) { if (p1 - x > slen - y && p1 > x) p1 = x + (slen - y); } else p1 = p0;
                    for (unsigned long long p = p0; p < p1; ++p) {
                        const unsigned long long bi = s0 + y + (p - x);
                        const uint32_t byte = a.seq4[bi >> 1];
                        const uint32_t code = (bi & 1ull) ? (byte & 15u) : (byte >> 4);
                        atomicAdd(&s_cnt[scan_plane(code) * kScanWin + ((uint32_t)p - ws)], 1u);
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
    __syncthreads();
    if (DENSE) {
        // five counters per position of the range, in the order of the output array: consecutive threads, consecutive words
        const uint32_t n5 = (we - lo) * 5u;
        uint32_t *out = a.dense + (unsigned long long)(lo - a.start) * 5ull;
        for (uint32_t i = tid; i < n5; i += kBlock) {
            const uint32_t q = i / 5u, cc = i - q * 5u, o = lo - ws + q;
            uint32_t v = s_cnt[(cc < 4u ? cc : 4u) * kScanWin + o];
            if (cc == 4u) v += s_cnt[o] + s_cnt[kScanWin + o] + s_cnt[2u * kScanWin + o] + s_cnt[3u * kScanWin + o] + s_cnt[5u * kScanWin + o];
            out[i] = v;
        }
        return;
    }
    uint32_t mine[SCAN_CLASSES] = {0, 0, 0, 0, 0, 0};
    const uint32_t lane = tid & 63u;
    for (uint32_t o0 = 0; o0 < kScanWin; o0 += kBlock) {                       // (uniform trip count: the ballot below needs whole waves)
        const uint32_t o = o0 + tid, p = ws + o;
        const bool in = p >= lo && p < we;
        int cls = -1;
        ScanCand cd;
        if (in) {
            const uint32_t A = s_cnt[o], Cc = s_cnt[kScanWin + o], G = s_cnt[2u * kScanWin + o], T = s_cnt[3u * kScanWin + o];
            const uint32_t N = s_cnt[4u * kScanWin + o], O = s_cnt[5u * kScanWin + o];
            const unsigned long long depth = (unsigned long long)A + Cc + G + T + N + O;      // below 2^32: one count per read
            uint32_t m = A; uint32_t alt = 'A';
            if (Cc > m) { m = Cc; alt = 'C'; }
            if (G > m) { m = G; alt = 'G'; }
            if (T > m) { m = T; alt = 'T'; }
            if (N > m) { m = N; alt = 'N'; }
            uint32_t rb = p < hi ? a.refb[p - a.start] : (uint32_t)'N';
            rb &= ~32u;                                                          // upper case; anything but ACGT is "other"
            const bool ref_ok = rb == 'A' || rb == 'C' || rb == 'G' || rb == 'T';
            // called <=> m / depth >= 0.7 in f64 <=> 10 m >= 7 depth (a ratio off 7/10 is off by more than an f64 divide rounds)
            if (depth < a.min_depth) cls = SCAN_LOW_DEPTH;
            else if (10ull * m >= 7ull * depth) cls = (alt == 'N' || !ref_ok) ? SCAN_UNCOMPARABLE : (alt == rb ? SCAN_MATCH : SCAN_VARIANT);
            else if (10ull * O >= 7ull * depth) cls = SCAN_AMBIGUOUS;
            else cls = SCAN_MIXED;
            mine[cls] += 1u;
            cd.pos = p + 1u; cd.ref = (uint8_t)rb; cd.alt = cls == SCAN_VARIANT ? (uint8_t)alt : (uint8_t)0; cd.pad[0] = cd.pad[1] = 0;
            cd.a = A; cd.c = Cc; cd.g = G; cd.t = T; cd.depth = (uint32_t)depth;
        }
        const bool emit = cls == SCAN_VARIANT || cls == SCAN_AMBIGUOUS;
        const unsigned long long bal = __ballot(emit);
        if (bal) {
            uint32_t base_i = 0;
            if (lane == 0) base_i = atomicAdd(a.n_cand, (uint32_t)__popcll(bal));
            base_i = __shfl(base_i, 0);
            if (emit) {
                const uint32_t i = base_i + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                if (i < a.cand_cap) a.cand[i] = cd;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < SCAN_CLASSES; ++k) {
        uint32_t v = mine[k];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
        if (lane == 0 && v) atomicAdd(&s_cls[k], (unsigned long long)v);
    }
    __syncthreads();
    if (tid < (uint32_t)SCAN_CLASSES && s_cls[tid]) atomicAdd(&a.cls[tid], s_cls[tid]);
}

} // namespace clk
