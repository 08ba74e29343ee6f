// depth_targets.hip.h -- k_target_depth, k_target_scan, k_target_finish: depth and callable-base summaries of the resident
// contig over a caller's list of targets (cl_contig_targets, include/callable_loci.h).  Included by callable_loci.hip behind
// depth_runs.hip.h.
//
// Every target [s, e) is two queries of a cumulative sum: with f(p) = (raw[p], qc[p], [raw[p] >= t_k]..., [qc[p] >= t_k]...),
// V = 2 + 2 K fields, and C(q) = the sum of f over p < q, the target's figures are C(e) - C(s).  Targets may therefore
// overlap, nest and repeat at no cost, and nothing is added across workgroups by an atomic: two calls give the same bytes.
// The host sorts the distinct query points that lie inside a window (a point on a window's first position needs none of
// this: C there is the scan's offset) and uploads them with, per window, the range of points inside it.
//
//   k_target_depth   a sibling of k_depth_profile and k_depth_runs, a kernel of its own: the same residents, the same
//                    rebuild of both depths per position (window_depths.hip.h: bit-sliced counter planes for qc, the scanned
//                    +-1 difference array for raw; 128 threads, a window of 2048, 16 positions per thread).  Per window the totals of f
//                    (64 bits each, one record per window, stored by one lane); in a window that holds query points (a workgroup-uniform branch) also the in-window
//                    prefix of f at each of them: the points are marked in a 2048-bit mask in LDS, a point's slot is the
//                    window's first slot plus the marks before it, and the thread that owns the position stores its
//                    exclusive prefix among the threads plus its own partial up to the point.  A window without points --
//                    for an exome nearly every one -- does the reduction only.  No global atomic, no per-position store.
//   k_target_scan    exclusive scan of the windows' totals into 64-bit offsets, one workgroup per field, n_win + 1 entries:
//                    entry n_win is the grand total (a point at n_win * 2048)
//   k_target_finish  one wave per target: lane f < V takes field f as offset + in-window prefix at e less the same at s;
//                    the states come from the interval array the tail kernel left (sorted, covering [0, extent)): a
//                    binary search for s, then the lanes stride over the intervals up to e, each clipped to the target
// Every index that comes from uploaded data is checked against its array before use; a failed check raises *err (the host
// answers CL_ERR_INTERNAL) instead of reading or storing out of range.
#pragma once

namespace clk {

constexpr int kTargetMaxThr = 8;                           // CL_TARGET_MAX_THRESHOLDS
constexpr int kTargetScanBlock = 1024;
constexpr int kTargetFinishBlock = 256;                    // four targets per workgroup
constexpr int kTargetWords = 30;                           // sizeof(cl_target_stats) / 4
constexpr uint32_t kTargetNoSlot = 0xFFFFFFFFu;            // a query point on a window's first position

// The planes the in-window scan runs over: the two 64-bit sums in pieces of 24, 24 and 16 bits (a thread's sum of 16 depths
// is below 2^36; 64 pieces of 24 bits add up below 2^30), then per threshold one word, raw count | qc count << 16 (a
// window's count is at most 2048).  The stored prefix of a point: raw lo, raw hi, qc lo, qc hi, then those eight words
// (all eight whatever K is: three 16-byte stores; the thresholds beyond K are 0xFFFFFFFF and count nothing).
constexpr int kTargetScanPlanes = 6 + kTargetMaxThr;
constexpr int kTargetPreWords = 4 + kTargetMaxThr;
// A window's totals, 64 bits each: raw, qc, the eight raw counts, the eight qc counts (all of them whatever K is).
constexpr int kTargetTotSlots = 2 + 2 * kTargetMaxThr;
static_assert(kTargetPreWords == 12, "three uint4 per point");

struct TargetArgs {
    DepthResidents res;
    uint32_t n_pt, pad;
    const uint32_t *pt;               // [n_pt]: the query points with q % 2048 != 0, ascending, distinct; behind them
                                      // pt_first[n_win + 1]: window w holds points [pt_first[w], pt_first[w + 1])
    ulonglong2 *wtot;                 // [n_win][kTargetTotSlots / 2]: the windows' totals of f
    uint4 *pre;                       // [n_pt][kTargetPreWords / 4]: the in-window prefix at every point
    uint32_t *err;
    uint32_t thr[kTargetMaxThr];      // the K thresholds, then 0xFFFFFFFF: no depth reaches it, the unused counts stay 0 unasked
};

template <int NP, bool HEAD4>
__global__ __launch_bounds__(kDepthBlock) void k_target_depth(TargetArgs a)
{
    constexpr int T = kDepthT, BS = kDepthBlock, PER = kDepthPer, MT = kTargetMaxThr;
    __shared__ __attribute__((aligned(16))) uint32_t s_diff[T];
    __shared__ uint32_t s_pl[NP][64];                      // wave 1's planes, then the window's (written by wave 0)
    __shared__ uint32_t s_mark[64];                        // bit p - W: p is a query point
    __shared__ uint32_t s_rank[64];                        // the marks below word i
    __shared__ uint32_t s_w[kTargetScanPlanes];            // wave 0's totals per plane
    __shared__ uint32_t s_tot;                             // wave 0's total of the differences

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    // the thresholds in eight vector registers: as scalar operands of 2 x 256 unrolled compares the compiler loads them
    // several times over in overlapping pairs, 27 SGPRs, and spills the loop's lane masks for them
    uint32_t thr[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) { uint32_t t = a.thr[k]; asm volatile("" : "+v"(t)); thr[k] = t; }

    for (uint32_t w = blockIdx.x; w < a.res.n_win; w += gridDim.x) {
        const uint32_t W = w * (uint32_t)T;
        const WinMeta wm = a.res.win[w];
        const RowLane rl = row_lane(a.res.rows, wm, lane, wv);
        // the window's points: a range of the uploaded list, held against the list before anything is read through it
        const uint32_t *pt_first = a.pt + a.n_pt;
        uint32_t pf = pt_first[w], pe = pt_first[w + 1u];
        if (pf > pe || pe > a.n_pt) { if (tid == 0u) atomicOr(a.err, 1u); pf = 0u; pe = 0u; }
        const uint32_t np = pe - pf;                       // (workgroup-uniform)

        wd_clear(s_diff, tid);
        if (wv == 0) s_mark[lane] = 0u;
        __syncthreads();

        uint32_t c[NP];
        wd_rows<NP>(c, rl, wm.rn, wv);
        wd_scatter<HEAD4>(a.res, wm, W, s_diff, tid);
        // ---- the window's points: marks ----
        for (uint32_t j = tid; j < np; j += BS) {
            const uint32_t x = a.pt[pf + j] - W;           // (a point below W wraps beyond T)
            if (x < (uint32_t)T) atomicOr(&s_mark[x >> 5], 1u << (x & 31u));
            else atomicOr(a.err, 1u);
        }
        if (wv != 0) wd_planes_put<NP>(c, s_pl, lane);
        __syncthreads();
        if (wv == 0) {
            wd_planes_add<NP>(c, s_pl, lane);
            if (np) {
                const uint32_t m = (uint32_t)__popc(s_mark[lane]);
                s_rank[lane] = dpp_incl_scan_u32(m) - m;
            }
        }
        uint32_t vr[PER], vq[PER];
        const uint32_t excl = wd_diff_scan(vr, s_diff, &s_tot, tid);
        __syncthreads();
        wd_diff_finish(vr, excl, &s_tot, wv);
        wd_extract<NP>(vq, s_pl, tid);
        const uint32_t n_ok = wd_span(W, tid, a.res.extent).n_ok;
        // ---- the thread's totals of f (positions at and beyond the extent count nowhere) ----
        unsigned long long t_raw = 0ull, t_qc = 0ull;
        uint32_t t_ge[MT];
#pragma unroll
        for (int k = 0; k < MT; ++k) t_ge[k] = 0u;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if ((uint32_t)i >= n_ok) { vr[i] = 0u; vq[i] = 0u; }
            t_raw += vr[i]; t_qc += vq[i];
#pragma unroll
            for (int k = 0; k < MT; ++k) t_ge[k] += (vr[i] >= thr[k] ? 1u : 0u) + (vq[i] >= thr[k] ? 0x10000u : 0u);
        }
        // ---- one inclusive scan per plane over the wave; lane 63 holds the wave's total ----
        uint32_t sc[kTargetScanPlanes];
        sc[0] = dpp_incl_scan_u32((uint32_t)t_raw & 0xFFFFFFu);
        sc[1] = dpp_incl_scan_u32((uint32_t)(t_raw >> 24) & 0xFFFFFFu);
        sc[2] = dpp_incl_scan_u32((uint32_t)(t_raw >> 48));
        sc[3] = dpp_incl_scan_u32((uint32_t)t_qc & 0xFFFFFFu);
        sc[4] = dpp_incl_scan_u32((uint32_t)(t_qc >> 24) & 0xFFFFFFu);
        sc[5] = dpp_incl_scan_u32((uint32_t)(t_qc >> 48));
#pragma unroll
        for (int k = 0; k < MT; ++k) sc[6 + k] = dpp_incl_scan_u32(t_ge[k]);
        if (wv == 0 && lane == 63u) {
#pragma unroll
            for (int j = 0; j < kTargetScanPlanes; ++j) s_w[j] = sc[j];
        }
        __syncthreads();
        // ---- the window's totals: the last lane of wave 1 holds its wave's in sc, wave 0's are in LDS; it stores the record ----
        if (wv != 0 && lane == 63u) {
            ulonglong2 *q = a.wtot + (size_t)w * (kTargetTotSlots / 2);
            q[0] = make_ulonglong2((unsigned long long)(sc[0] + s_w[0]) + ((unsigned long long)(sc[1] + s_w[1]) << 24) + ((unsigned long long)(sc[2] + s_w[2]) << 48),
                                   (unsigned long long)(sc[3] + s_w[3]) + ((unsigned long long)(sc[4] + s_w[4]) << 24) + ((unsigned long long)(sc[5] + s_w[5]) << 48));
#pragma unroll
            for (int k = 0; k < MT; k += 2) {
                const uint32_t w0 = sc[6 + k] + s_w[6 + k], w1 = sc[7 + k] + s_w[7 + k];
                q[1 + k / 2] = make_ulonglong2(w0 & 0xFFFFu, w1 & 0xFFFFu);
                q[1 + MT / 2 + k / 2] = make_ulonglong2(w0 >> 16, w1 >> 16);
            }
        }
        // ---- a window with points: the in-window prefix of f at each of them, stored by the thread that owns it ----
        if (np) {
            const uint32_t mword = s_mark[tid >> 1];
            const uint32_t m16 = (mword >> ((tid & 1u) * 16u)) & 0xFFFFu;
            if (m16) {
                uint32_t slot = pf + s_rank[tid >> 1] + ((tid & 1u) ? (uint32_t)__popc(mword & 0xFFFFu) : 0u);
                // the thread's slots, held against the window's range once (pe <= n_pt: inside pre)
                const bool fits = slot + (uint32_t)__popc(m16) <= pe;
                if (!fits) atomicOr(a.err, 1u);
                // the exclusive prefix among the window's threads: the wave's scan less the thread's own, wave 0's total before wave 1
                unsigned long long x_raw = (unsigned long long)sc[0] + ((unsigned long long)sc[1] << 24) + ((unsigned long long)sc[2] << 48) - t_raw;
                unsigned long long x_qc = (unsigned long long)sc[3] + ((unsigned long long)sc[4] << 24) + ((unsigned long long)sc[5] << 48) - t_qc;
                uint32_t x_ge[MT];
#pragma unroll
                for (int k = 0; k < MT; ++k) x_ge[k] = sc[6 + k] - t_ge[k];
                if (wv) {
                    x_raw += (unsigned long long)s_w[0] + ((unsigned long long)s_w[1] << 24) + ((unsigned long long)s_w[2] << 48);
                    x_qc += (unsigned long long)s_w[3] + ((unsigned long long)s_w[4] << 24) + ((unsigned long long)s_w[5] << 48);
#pragma unroll
                    for (int k = 0; k < MT; ++k) x_ge[k] += s_w[6 + k];
                }
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    if (fits && (m16 & (1u << i))) {
                        uint4 *q = a.pre + (size_t)slot * (kTargetPreWords / 4);
                        q[0] = make_uint4((uint32_t)x_raw, (uint32_t)(x_raw >> 32), (uint32_t)x_qc, (uint32_t)(x_qc >> 32));
                        q[1] = make_uint4(x_ge[0], x_ge[1], x_ge[2], x_ge[3]);
                        q[2] = make_uint4(x_ge[4], x_ge[5], x_ge[6], x_ge[7]);
                        ++slot;
                    }
                    x_raw += vr[i]; x_qc += vq[i];
#pragma unroll
                    for (int k = 0; k < MT; ++k) x_ge[k] += (vr[i] >= thr[k] ? 1u : 0u) + (vq[i] >= thr[k] ? 0x10000u : 0u);
                }
            }
        }
        __syncthreads();                                   // the next window overwrites what this one read
    }
}

// Inclusive prefix sum of 64-bit values over the wave (six steps of a lane shift: the scan runs once per 1024 windows).
__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// The exclusive scan of the windows' totals into 64-bit offsets: workgroup f scans field f of V = 2 + 2 K (raw, qc, K raw
// counts, K qc counts), kTargetScanBlock windows per step, and stores n_win + 1 entries (the last: the field's total over
// the contig).
__global__ __launch_bounds__(kTargetScanBlock) void k_target_scan(const unsigned long long *__restrict__ wtot, uint32_t n_win, uint32_t n_thr,
                                                                   unsigned long long *__restrict__ off)
{
    __shared__ unsigned long long s_w[kTargetScanBlock / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t K = n_thr < (uint32_t)kTargetMaxThr ? n_thr : (uint32_t)kTargetMaxThr, f = blockIdx.x;
    // field f's slot among a window's totals (f < 2 + 2 K by the launch; a larger one scans slot 0 into its own row)
    const uint32_t slot = f < 2u ? f : f < 2u + K ? f : f < 2u + 2u * K ? 2u + (uint32_t)kTargetMaxThr + (f - 2u - K) : 0u;
    const unsigned long long *src = wtot + slot;
    unsigned long long *dst = off + (size_t)blockIdx.x * ((size_t)n_win + 1u);
    unsigned long long run = 0ull;
    for (uint32_t base = 0; base < n_win; base += (uint32_t)kTargetScanBlock) {
        const uint32_t w = base + tid;
        const unsigned long long c = w < n_win ? src[(size_t)w * kTargetTotSlots] : 0ull;
        const unsigned long long inc = wave_incl_scan_u64(c, lane);
        if (lane == 63u) s_w[wv] = inc;
        __syncthreads();
        unsigned long long o = inc - c, tot = 0ull;
        for (uint32_t i = 0; i < (uint32_t)(kTargetScanBlock / 64); ++i) { const unsigned long long v = s_w[i]; if (i < wv) o += v; tot += v; }
        if (w < n_win) dst[w] = run + o;
        run += tot;
        __syncthreads();
    }
    if (tid == 0u) dst[n_win] = run;
}

struct TargetFinishArgs {
    const uint32_t *tg;               // [n][4]: s, e (clipped to the extent), the slots of s and e among the points
    uint32_t n, n_pt;
    uint32_t n_thr, n_win;
    const unsigned long long *off;    // [V][n_win + 1]
    const uint32_t *pre;              // [n_pt][kTargetPreWords]
    const Interval *iv;
    uint32_t n_iv, extent;
    uint32_t *out;                    // [n][kTargetWords]: cl_target_stats, zeroed before the launch
    uint32_t *err;
};

__global__ __launch_bounds__(kTargetFinishBlock) void k_target_finish(TargetFinishArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * (uint32_t)(kTargetFinishBlock / 64) + (threadIdx.x >> 6);   // (wave-uniform)
    if (i >= a.n) return;
    const uint32_t K = a.n_thr < (uint32_t)kTargetMaxThr ? a.n_thr : (uint32_t)kTargetMaxThr;
    const uint32_t s = a.tg[4u * (size_t)i], e = a.tg[4u * (size_t)i + 1u];
    const uint32_t ss = a.tg[4u * (size_t)i + 2u], es = a.tg[4u * (size_t)i + 3u];
    uint32_t *o = a.out + (size_t)i * kTargetWords;
    if (!(s <= e && e <= a.extent && (e >> 11) <= a.n_win)) { if (lane == 0u) atomicOr(a.err, 1u); return; }
    if (lane == 0u) { o[0] = s; o[1] = e; o[2] = e - s; }
    if (s == e) return;                                    // (the rest of the record is zeros)
    // (a point inside a window has a slot among the points; one on a window's first position needs none)
    if (((s & 2047u) && ss >= a.n_pt) || ((e & 2047u) && es >= a.n_pt)) { if (lane == 0u) atomicOr(a.err, 1u); return; }

    // ---- the depth fields: lane f < V ----
    if (lane < 2u + 2u * K) {
        const unsigned long long *of = a.off + (size_t)lane * ((size_t)a.n_win + 1u);
        auto prefix_at = [&](uint32_t q, uint32_t slot) -> unsigned long long {
            unsigned long long v = of[q >> 11];
            if (q & 2047u) {
                const uint32_t *q = a.pre + (size_t)slot * kTargetPreWords;   // (slot < n_pt: checked above)
                if (lane < 2u) v += (unsigned long long)q[2u * lane] | ((unsigned long long)q[2u * lane + 1u] << 32);
                else {
                    const uint32_t g = lane - 2u, qc = g >= K ? 1u : 0u, k = g - qc * K;
                    const uint32_t word = q[4u + k];
                    v += qc ? word >> 16 : word & 0xFFFFu;
                }
            }
            return v;
        };
        const unsigned long long v = prefix_at(e, es) - prefix_at(s, ss);
        if (lane < 2u) { o[4u + 2u * lane] = (uint32_t)v; o[5u + 2u * lane] = (uint32_t)(v >> 32); }
        else {
            const uint32_t g = lane - 2u, qc = g >= K ? 1u : 0u, k = g - qc * K;
            o[14u + 8u * qc + k] = (uint32_t)v;
        }
    }
    // ---- the states: the last interval that starts at or below s, then the lanes stride up to e ----
    uint32_t lo = 0u, hi = a.n_iv;                         // the answer lies in [lo, hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.iv[mid].start <= s) lo = mid; else hi = mid;
    }
    uint32_t cnt[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    bool bad = a.n_iv == 0u;
    // interval j, clipped to the target, into the lane's counts; whether it starts below e
    // (without a branch, the index clamped into the array: the eight loads of a round are independent)
    auto take = [&](uint32_t j) -> bool {
        const Interval v = a.iv[j < a.n_iv ? j : a.n_iv - 1u];
        const bool in = j < a.n_iv && v.start < e;
        const uint32_t b = v.start > s ? v.start : s, d = v.end < e ? v.end : e;
        const uint32_t n = in && d > b ? d - b : 0u;
#pragma unroll
        for (int st = 0; st < 6; ++st) cnt[st] += v.state == (uint32_t)st ? n : 0u;
        bad |= in && v.state >= 6u;
        return in;
    };
    if (a.n_iv == 0u) { if (lane == 0u) atomicOr(a.err, 1u); return; }
    // The first 64 intervals, which is where an exon-sized target ends; a longer one goes on 512 at a time, eight loads
    // in flight per lane (a whole-contig target is bound by the latency of this walk).  The intervals ascend: once the
    // last lane's last interval is at or beyond e, so is everything behind it.
    bool more = take(lo + lane);
    for (uint32_t base = lo + 64u; __builtin_amdgcn_readlane((int)more, 63); base += 512u) {
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) more = take(base + u * 64u + lane);
    }
    uint32_t mine = 0u, all = 0u;
#pragma unroll
    for (int st = 0; st < 6; ++st) { const uint32_t t = dpp_wave_sum_u32(cnt[st]); if (lane == (uint32_t)st) mine = t; all += t; }
    if (lane < 6u) o[8u + lane] = mine;
    // (intervals that do not cover the target exactly once: not the array the tail kernel leaves)
    if (bad || all != e - s) atomicOr(a.err, 1u);
}

} // namespace clk
