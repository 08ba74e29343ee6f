// target_order.hip.h -- k_target_order, k_target_order_step: minimum, quartiles and maximum of both depths of the resident
// contig over a caller's list of targets (cl_contig_target_order, include/callable_loci.h).  Included by callable_loci.hip
// behind depth_targets.hip.h.
//
// Order statistics are no differences of a cumulative sum, so the prefix form of depth_targets.hip.h gives none of them.
// They are selected bit by bit instead, every target at once: a selector (kind in {raw, qc} x quartile j in {1, 2, 3}) of a
// target holds the high bits of its answer that are decided (`val`) and the rank it still looks for among the target's
// positions whose depth agrees with those bits (`rank`, from 0).  A round takes the next bit down: it counts the positions
// that agree with the decided bits and have that bit clear; a rank below the count leaves the bit clear, any other sets
// it and takes the count off the rank.  After the last bit val is the depth of that rank: the smallest v with
// #{d <= v} >= ceil(j len / 4), the quartile rule of dut_depth_stats.  No per-position value leaves the workgroup.
//
// The host cuts the targets at the windows into pieces (target_pieces.h) and uploads them sorted by window.
//
//   k_target_order<NP, HEAD4, FIRST>
//                    a sibling of k_target_depth: the same residents, the same rebuild of both depths per position
//                    (window_depths.hip.h; 128 threads, a window of 2048), both left as 2048-entry arrays in LDS (raw in
//                    the scanned difference array).  The two waves then take the window's pieces in turn, the lanes
//                    striding over a piece's positions.  FIRST: the wave's minimum and maximum of both kinds into the
//                    target's four words by atomicMax (a minimum as the maximum of the complement, so that zeroed words
//                    start both).  Otherwise per selector the count of this round by ballot and popcount, and one
//                    atomicAdd per selector and piece into the target's six counts.  A window without pieces -- for an
//                    exome nearly every one -- skips the rebuild (a workgroup-uniform branch).  Integer atomics only:
//                    the sums do not depend on their order, two calls give the same bytes.
//   k_target_order_step
//                    eight threads per target: thread k < 6 is selector k, thread 6 the rest of the record.  After the
//                    FIRST launch it sets the ranks (j len + 3) / 4 - 1, folds the targets' largest raw depth into one
//                    word (what the host reads to know how many rounds there are) and writes the record as it stands;
//                    after a round it settles the bit, zeroes the count, and after the last one writes the quartiles.
// Every index that comes from uploaded data is checked against its array before use; a failed check raises *err (the host
// answers CL_ERR_INTERNAL) instead of reading or storing out of range.
#pragma once

namespace clk {

constexpr int kOrderSel = 6;                               // raw q1, q2, q3, qc q1, q2, q3
// A target's state, 24 words: ~min raw, max raw, ~min qc, max qc; val[6]; rank[6]; cnt[6]; two spare.
constexpr int kOrderStateWords = 24;
constexpr int kOrderMinMax = 0, kOrderVal = 4, kOrderRank = 10, kOrderCnt = 16;
constexpr int kOrderWords = 13;                            // sizeof(cl_target_order) / 4
constexpr int kOrderStepBlock = 256;                       // 32 targets per workgroup

struct OrderArgs {
    DepthResidents res;
    uint32_t n_pc, n_tg;
    const uint2 *pc;                  // [n_pc]: the pieces {target, a | b << 16}, sorted by window
    const uint32_t *pc_first;         // [n_win + 1]: window w holds pieces [pc_first[w], pc_first[w + 1])
    uint32_t *st;                     // [n_tg][kOrderStateWords], zeroed before the FIRST launch
    uint32_t *err;
    uint32_t bit, pad;                // the bit this round decides (not FIRST)
};

template <int NP, bool HEAD4, bool FIRST>
__global__ __launch_bounds__(kDepthBlock) void k_target_order(OrderArgs a)
{
    constexpr int T = kDepthT, PER = kDepthPer;
    __shared__ __attribute__((aligned(16))) uint32_t s_diff[T];   // the differences, then raw_depth
    __shared__ __attribute__((aligned(16))) uint32_t s_qc[T];     // qc_depth
    __shared__ uint32_t s_pl[NP][64];                      // wave 1's planes, then the window's (written by wave 0)
    __shared__ uint32_t s_tot;                             // wave 0's total of the differences

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));

    for (uint32_t w = blockIdx.x; w < a.res.n_win; w += gridDim.x) {
        // the window's pieces: a range of the uploaded list, held against the list before anything is read through it
        uint32_t pf = a.pc_first[w], pe = a.pc_first[w + 1u];
        if (pf > pe || pe > a.n_pc) { if (tid == 0u) atomicOr(a.err, 1u); pf = 0u; pe = 0u; }
        if (pf == pe) continue;                            // (workgroup-uniform, in front of every barrier of the loop)
        const uint32_t W = w * (uint32_t)T;
        const WinMeta wm = a.res.win[w];
        const RowLane rl = row_lane(a.res.rows, wm, lane, wv);

        wd_clear(s_diff, tid);
        __syncthreads();

        uint32_t c[NP];
        wd_rows<NP>(c, rl, wm.rn, wv);
        wd_scatter<HEAD4>(a.res, wm, W, s_diff, tid);
        if (wv != 0) wd_planes_put<NP>(c, s_pl, lane);
        __syncthreads();
        if (wv == 0) wd_planes_add<NP>(c, s_pl, lane);
        uint32_t vr[PER], vq[PER];
        const uint32_t excl = wd_diff_scan(vr, s_diff, &s_tot, tid);
        __syncthreads();
        wd_diff_finish(vr, excl, &s_tot, wv);
        wd_extract<NP>(vq, s_pl, tid);
        // both depths into LDS: a thread's 16 raw depths over the 16 differences it alone has read
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            reinterpret_cast<uint4 *>(s_diff)[tid * (PER / 4) + q] = make_uint4(vr[4 * q], vr[4 * q + 1], vr[4 * q + 2], vr[4 * q + 3]);
            reinterpret_cast<uint4 *>(s_qc)[tid * (PER / 4) + q] = make_uint4(vq[4 * q], vq[4 * q + 1], vq[4 * q + 2], vq[4 * q + 3]);
        }
        __syncthreads();

        // ---- the window's pieces, wave wv every second one (positions at and beyond the extent are in no piece) ----
        const uint32_t n_ok = W >= a.res.extent ? 0u : (a.res.extent - W < (uint32_t)T ? a.res.extent - W : (uint32_t)T);
        for (uint32_t j = pf + wv; j < pe; j += 2u) {
            const uint2 pc = a.pc[j];                      // (wave-uniform)
            const uint32_t tg = pc.x, pa = pc.y & 0xFFFFu, pb = pc.y >> 16;
            if (!(tg < a.n_tg && pa < pb && pb <= n_ok)) { if (lane == 0u) atomicOr(a.err, 1u); continue; }
            uint32_t *st = a.st + (size_t)tg * kOrderStateWords;
            if (FIRST) {
                uint32_t nr = 0u, xr = 0u, nq = 0u, xq = 0u;   // ~min raw, max raw, ~min qc, max qc
                for (uint32_t x = pa + lane; x < pb; x += 64u) {
                    const uint32_t r = s_diff[x], q = s_qc[x];
                    nr = ~r > nr ? ~r : nr; xr = r > xr ? r : xr;
                    nq = ~q > nq ? ~q : nq; xq = q > xq ? q : xq;
                }
                nr = dpp_wave_max_u32(nr); xr = dpp_wave_max_u32(xr);
                nq = dpp_wave_max_u32(nq); xq = dpp_wave_max_u32(xq);
                const uint32_t mine = lane == 0u ? nr : lane == 1u ? xr : lane == 2u ? nq : xq;
                if (lane < 4u) atomicMax(&st[kOrderMinMax + lane], mine);
            } else {
                // a selector's decided bits (the bits below them are still 0): a depth agrees with them and has this
                // round's bit clear where nothing of depth ^ val is left at or above the bit
                uint32_t val[kOrderSel], cnt[kOrderSel];
#pragma unroll
                for (int k = 0; k < kOrderSel; ++k) { val[k] = st[kOrderVal + k]; cnt[k] = 0u; }
                for (uint32_t base = pa; base < pb; base += 64u) {   // (wave-uniform: every lane is at the ballots)
                    const uint32_t x = base + lane;
                    const bool in = x < pb;
                    const uint32_t r = in ? s_diff[x] : 0u, q = in ? s_qc[x] : 0u;
#pragma unroll
                    for (int k = 0; k < kOrderSel; ++k) {
                        const uint32_t d = k < 3 ? r : q;
                        cnt[k] += (uint32_t)__popcll(__ballot(in && ((d ^ val[k]) >> a.bit) == 0u));
                    }
                }
                uint32_t mine = 0u;
#pragma unroll
                for (int k = 0; k < kOrderSel; ++k) mine = lane == (uint32_t)k ? cnt[k] : mine;
                if (lane < (uint32_t)kOrderSel && mine) atomicAdd(&st[kOrderCnt + lane], mine);
            }
        }
        __syncthreads();                                   // the next window overwrites what this one read
    }
}

struct OrderStepArgs {
    const uint32_t *tg;               // [n][2]: s, e (clipped to the extent)
    uint32_t n, extent;
    uint32_t *st;                     // [n][kOrderStateWords]
    uint32_t *out;                    // [n][kOrderWords]: cl_target_order
    uint32_t *max_raw;                // one word, zeroed before the FIRST launch: the largest raw depth of any target
    uint32_t *err;
    uint32_t first, last;             // behind the FIRST launch; behind the last round
    uint32_t bit, pad;                // the bit the round has counted for (not first)
};

__global__ __launch_bounds__(kOrderStepBlock) void k_target_order_step(OrderStepArgs a)
{
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0u) s_max = 0u;
    __syncthreads();
    const uint64_t g = (uint64_t)blockIdx.x * kOrderStepBlock + threadIdx.x;
    const uint64_t i = g >> 3;
    const uint32_t k = (uint32_t)g & 7u;
    if (i < a.n) {
        const uint32_t s = a.tg[2u * i], e = a.tg[2u * i + 1u];
        uint32_t *st = a.st + i * kOrderStateWords, *o = a.out + i * kOrderWords;
        if (!(s <= e && e <= a.extent)) { if (k == 0u) atomicOr(a.err, 1u); }
        else {
            const uint32_t len = e - s;
            if (k < (uint32_t)kOrderSel) {
                uint32_t val = 0u;
                if (len) {
                    if (a.first) {
                        const uint32_t j = k % 3u + 1u;
                        st[kOrderRank + k] = (uint32_t)(((uint64_t)j * len + 3u) / 4u - 1u);
                    } else {
                        const uint32_t cnt = st[kOrderCnt + k], rank = st[kOrderRank + k];
                        val = st[kOrderVal + k];
                        if (rank >= cnt) { val |= 1u << a.bit; st[kOrderVal + k] = val; st[kOrderRank + k] = rank - cnt; }
                        st[kOrderCnt + k] = 0u;
                    }
                }
                if (a.first || a.last) o[3u + 5u * (k / 3u) + 1u + k % 3u] = val;
            } else if (k == 6u && a.first) {
                o[0] = s; o[1] = e; o[2] = len;
                const uint32_t xr = len ? st[kOrderMinMax + 1] : 0u;
                o[3] = len ? ~st[kOrderMinMax] : 0u; o[7] = xr;
                o[8] = len ? ~st[kOrderMinMax + 2] : 0u; o[12] = len ? st[kOrderMinMax + 3] : 0u;
                if (xr) atomicMax(&s_max, xr);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u && a.first && s_max) atomicMax(a.max_raw, s_max);
}

} // namespace clk
