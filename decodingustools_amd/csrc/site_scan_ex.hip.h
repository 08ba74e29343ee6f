// site_scan_ex.hip.h -- the filtered, strand-aware form of the dense site scan (site_scan.hip.h), for a resident site
// tile that carries an attachment (cl_site_attach_quals): per read its BAM flag, per base one pass bit
// (qual >= min_base_quality, taken on the host; bit i of word w <-> base 64 w + i in the numbering of seq4).
//
// k_site_scan<DENSE> stays what it is; this is a kernel of its own over the same index (k_site_scan_index) and the same
// window of kScanWin positions per workgroup.  Relative to it:
//   per read   one 2-byte load of the flag and one early exit on (flag & exclude_flags); flag & 0x10 picks the strand;
//   per base   one bit of a 64-bit word of pass bits that is loaded once per CIGAR operation and once more whenever
//              the base index crosses a multiple of 64 -- never the quality bytes;
//   counters   ten LDS planes instead of six: A C G T by strand (forward, reverse), N, any other code.  Exactly 40 KB of
//              LDS per workgroup: 4 workgroups (16 waves) per CU of 160 KiB where the unfiltered kernel has 6.
// The call sums the strands and is the rule of k_site_scan, word for word; a candidate also carries the per-strand counts
// of its alternative and reference bases.  A position whose "other" plane holds 7/10 of the depth is reported as
// ambiguous exactly as there, and settled with k_site_scan_settle: the 16-code histogram of just those positions under
// the same filter (cl_site_run's histogram is unfiltered and cannot serve).
#pragma once

#include "site_scan.hip.h"

namespace clk {

constexpr uint32_t kScanExPlanes = 10;       // A+ A- C+ C- G+ G- T+ T- N other  (+ forward, - reverse: flag & 0x10)

struct ScanCandEx {
    uint32_t pos;                            // 1-based
    uint8_t  ref, alt, pad[2];
    uint32_t a, c, g, t, depth;              // both strands
    uint32_t alt_fwd, alt_rev, ref_fwd, ref_rev;
};

struct ScanExArgs {
    ScanArgs s;                              // cand and dense of it are not used
    const uint16_t *flag;                    // per read
    const unsigned long long *pass;          // one bit per base of seq4
    uint32_t exclude_flags, use_bq;
    ScanCandEx *cand;
    uint32_t *dense;                         // DENSE: (end_pos - start) * 9: A+ A- C+ C- G+ G- T+ T- depth
};

__device__ __forceinline__ uint32_t scan_ex_plane(uint32_t code, uint32_t rev)
{
    return code == 1u ? rev : code == 2u ? 2u + rev : code == 4u ? 4u + rev : code == 8u ? 6u + rev : code == 15u ? 8u : 9u;
}

template <bool DENSE>
__global__ __launch_bounds__(kBlock) void k_site_scan_ex(ScanExArgs ax)
{
    // exactly 40 KB: four workgroups fit a CU's 160 KiB (a byte more and only three do), so the class counts of the
    // end take over the first words of the planes once every thread has read its counters
    __shared__ alignas(8) uint32_t s_cnt[kScanExPlanes * kScanWin];
    const ScanArgs &a = ax.s;
    const uint32_t tid = threadIdx.x;
    const uint32_t w = a.win0 + blockIdx.x;
    const unsigned long long ws64 = (unsigned long long)w * kScanWin;
    const uint32_t ws = (uint32_t)ws64;
    const uint32_t lo = ws > a.start ? ws : a.start;
    const uint32_t we = (ws64 + kScanWin < (unsigned long long)a.end_pos) ? ws + kScanWin : a.end_pos;
    const uint32_t hi = (unsigned long long)we < a.ref_len ? we : (uint32_t)a.ref_len;
    for (uint32_t i = tid; i < kScanExPlanes * kScanWin; i += kBlock) s_cnt[i] = 0;
    __syncthreads();
    const uint32_t r_first = a.wfirst[w], r_last = a.wlast[w];
    if (r_first < r_last && lo < hi) {
        for (uint32_t r = r_first + tid; r < r_last; r += kBlock) {
            const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
            const uint32_t e = a.end[r];
            if ((rr.w & 255u) < a.min_quality || e <= lo || (uint32_t)rr.x >= hi) continue;
            const uint32_t fl = ax.flag[r];
            if (fl & ax.exclude_flags) continue;
            const uint32_t rev = (fl >> 4) & 1u;
            uint32_t k1; unsigned long long slen;
            scan_read_extent(a.rec, r, rr, k1, slen);
            const unsigned long long base = a.seq_base[r / kBlock];
            const unsigned long long s0 = base + (uint32_t)(rr.z - (uint32_t)base);
            unsigned long long x = (uint32_t)rr.x, y = 0;
            for (uint32_t kk = rr.y; kk < k1 && x < hi; ++kk) {
                const uint32_t c = a.cigar[kk];
                const uint32_t op = c & 15u, l = c >> 4;
                if (op_match(op)) {
                    unsigned long long p0 = x > lo ? x : lo, p1 = x + l < hi ? x + l : hi;
                    if (y < slen) { if (p1 - x > slen - y && p1 > x) p1 = x + (slen - y); } else p1 = p0;
                    unsigned long long bi = s0 + y + (p0 - x);
                    unsigned long long pw = ~0ull;
                    if (ax.use_bq && p0 < p1) pw = ax.pass[bi >> 6];
                    for (unsigned long long p = p0; p < p1; ++p, ++bi) {
                        if (ax.use_bq) {
                            if ((bi & 63ull) == 0ull) pw = ax.pass[bi >> 6];
                            if (!((pw >> (bi & 63ull)) & 1ull)) continue;
                        }
                        const uint32_t byte = a.seq4[bi >> 1];
                        const uint32_t code = (bi & 1ull) ? (byte & 15u) : (byte >> 4);
                        atomicAdd(&s_cnt[scan_ex_plane(code, rev) * kScanWin + ((uint32_t)p - ws)], 1u);
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
        // nine counters per position of the range, in the order of the output array
        const uint32_t n9 = (we - lo) * 9u;
        uint32_t *out = ax.dense + (unsigned long long)(lo - a.start) * 9ull;
        for (uint32_t i = tid; i < n9; i += kBlock) {
            const uint32_t q = i / 9u, cc = i - q * 9u, o = lo - ws + q;
            uint32_t v;
            if (cc < 8u) v = s_cnt[cc * kScanWin + o];
            else { v = 0; for (uint32_t k = 0; k < kScanExPlanes; ++k) v += s_cnt[k * kScanWin + o]; }
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
        ScanCandEx cd;
        if (in) {
            uint32_t f[4], v[4];
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) { f[b] = s_cnt[(2u * b) * kScanWin + o]; v[b] = s_cnt[(2u * b + 1u) * kScanWin + o]; }
            const uint32_t A = f[0] + v[0], Cc = f[1] + v[1], G = f[2] + v[2], T = f[3] + v[3];
            const uint32_t N = s_cnt[8u * kScanWin + o], O = s_cnt[9u * kScanWin + o];
            const unsigned long long depth = (unsigned long long)A + Cc + G + T + N + O;      // below 2^32: one count per read
            uint32_t m = A; uint32_t alt = 'A'; uint32_t ai = 0;
            if (Cc > m) { m = Cc; alt = 'C'; ai = 1; }
            if (G > m) { m = G; alt = 'G'; ai = 2; }
            if (T > m) { m = T; alt = 'T'; ai = 3; }
            if (N > m) { m = N; alt = 'N'; }
            uint32_t rb = p < hi ? a.refb[p - a.start] : (uint32_t)'N';
            rb &= ~32u;
            const bool ref_ok = rb == 'A' || rb == 'C' || rb == 'G' || rb == 'T';
            if (depth < a.min_depth) cls = SCAN_LOW_DEPTH;
            else if (10ull * m >= 7ull * depth) cls = (alt == 'N' || !ref_ok) ? SCAN_UNCOMPARABLE : (alt == rb ? SCAN_MATCH : SCAN_VARIANT);
            else if (10ull * O >= 7ull * depth) cls = SCAN_AMBIGUOUS;
            else cls = SCAN_MIXED;
            mine[cls] += 1u;
            cd.pos = p + 1u; cd.ref = (uint8_t)rb; cd.alt = cls == SCAN_VARIANT ? (uint8_t)alt : (uint8_t)0; cd.pad[0] = cd.pad[1] = 0;
            cd.a = A; cd.c = Cc; cd.g = G; cd.t = T; cd.depth = (uint32_t)depth;
            cd.alt_fwd = cd.alt_rev = cd.ref_fwd = cd.ref_rev = 0;
            if (cls == SCAN_VARIANT) {
                const uint32_t ri = rb == 'A' ? 0u : rb == 'C' ? 1u : rb == 'G' ? 2u : 3u;
#pragma unroll
                for (uint32_t b = 0; b < 4u; ++b) {                               // (selects, not indexed registers)
                    if (b == ai) { cd.alt_fwd = f[b]; cd.alt_rev = v[b]; }
                    if (b == ri) { cd.ref_fwd = f[b]; cd.ref_rev = v[b]; }
                }
            }
        }
        const bool emit = cls == SCAN_VARIANT || cls == SCAN_AMBIGUOUS;
        const unsigned long long bal = __ballot(emit);
        if (bal) {
            uint32_t base_i = 0;
            if (lane == 0) base_i = atomicAdd(a.n_cand, (uint32_t)__popcll(bal));
            base_i = __shfl(base_i, 0);
            if (emit) {
                const uint32_t i = base_i + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                if (i < a.cand_cap) ax.cand[i] = cd;
            }
        }
    }
    __syncthreads();
    unsigned long long *s_cls = reinterpret_cast<unsigned long long *>(s_cnt);
    if (tid < (uint32_t)SCAN_CLASSES) s_cls[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SCAN_CLASSES; ++k) {
        uint32_t v = mine[k];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
        if (lane == 0 && v) atomicAdd(&s_cls[k], (unsigned long long)v);
    }
    __syncthreads();
    if (tid < (uint32_t)SCAN_CLASSES && s_cls[tid]) atomicAdd(&a.cls[tid], s_cls[tid]);
}

// The 16-code histogram of single positions under the filter of ax: one workgroup per position of pos1 (1-based, inside
// the contig), over the reads of the position's window range.  For the few positions the ten planes cannot classify.
__global__ __launch_bounds__(kBlock) void k_site_scan_settle(ScanExArgs ax, const uint32_t *pos1, uint32_t *hist16)
{
    __shared__ uint32_t s_h[16];
    const ScanArgs &a = ax.s;
    const uint32_t tid = threadIdx.x;
    if (tid < 16u) s_h[tid] = 0;
    __syncthreads();
    const uint32_t p = pos1[blockIdx.x] - 1u;
    const uint32_t w = p / kScanWin;
    const uint32_t r_first = a.wfirst[w], r_last = a.wlast[w];
    if (r_first < r_last && (unsigned long long)p < a.ref_len) {
        for (uint32_t r = r_first + tid; r < r_last; r += kBlock) {
            const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
            const uint32_t e = a.end[r];
            if ((rr.w & 255u) < a.min_quality || e <= p || (uint32_t)rr.x > p) continue;
            if ((uint32_t)ax.flag[r] & ax.exclude_flags) continue;
            uint32_t k1; unsigned long long slen;
            scan_read_extent(a.rec, r, rr, k1, slen);
            const unsigned long long base = a.seq_base[r / kBlock];
            const unsigned long long s0 = base + (uint32_t)(rr.z - (uint32_t)base);
            unsigned long long x = (uint32_t)rr.x, y = 0;
            for (uint32_t kk = rr.y; kk < k1 && x <= p; ++kk) {
                const uint32_t c = a.cigar[kk];
                const uint32_t op = c & 15u, l = c >> 4;
                if (op_match(op)) {
                    if (p < x + l) {
                        const unsigned long long q = y + (p - x);
                        if (q < slen) {
                            const unsigned long long bi = s0 + q;
                            if (!ax.use_bq || ((ax.pass[bi >> 6] >> (bi & 63ull)) & 1ull)) {
                                const uint32_t byte = a.seq4[bi >> 1];
                                atomicAdd(&s_h[(bi & 1ull) ? (byte & 15u) : (byte >> 4)], 1u);
                            }
                        }
                        break;
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
    if (tid < 16u) hist16[(size_t)blockIdx.x * 16u + tid] = s_h[tid];
}

} // namespace clk
