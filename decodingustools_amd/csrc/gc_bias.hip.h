// gc_bias.hip.h -- k_gc_bias: both depths of the resident contig by the GC content of the reference around each position,
// reduced on the device (cl_contig_gc_bias, include/callable_loci.h).  Included by callable_loci.hip behind
// window_depths.hip.h (the rebuild of both depths, shared with k_depth_profile, k_depth_runs and k_target_depth).
//
// The reference is two bit planes, gc and valid (gc_bits.h), interleaved as pairs of 64-bit words: pair k is {gc, valid}
// of the positions [64 k - kGcPad, 64 k - kGcPad + 64).  kGcPad = 512 invalid positions stand in front of position 0
// and at least as many behind the last window, so a workgroup reads the 48 pairs of [W - 512, W + 2048 + 512) whatever
// the window length n <= 1024 is: the halo is n / 2 positions before the window and n - n / 2 behind it.
//
// Per workgroup (128 threads, a thread owns 16 positions of a window of 2048; windows w = blockIdx.x, + gridDim.x, ...):
//   * wave 0's lanes 0..47 load a pair each and leave the 96 + 1 words of either plane in LDS, with the exclusive
//     prefix of their popcounts (one DPP scan: both counts are below 2^16 and share a word)
//   * both depths as in k_depth_profile (the wd_* phases of window_depths.hip.h)
//   * a thread takes g and the number of valid bases of its first position's window from the prefix and two masked
//     popcounts a plane, then moves on with one bit entering and one leaving (two 16-bit fields a plane); the bin is
//     100 g / (n - v), v the invalid bases, or the skipped slot kGcBins when v > max_invalid
//   * the 4 x 101 bins in LDS: a thread merges the equal bins among its 16 positions and adds a run with one atomic a
//     table.  Widths: a workgroup takes at most 2^21 / 2048 windows of 2048 positions (n_win <= 2^21, the grid is 2048
//     once there are that many), 2^21 positions: the counts fit 32 bits; the depth sums are 64-bit, whatever NP is
//   * at the end: one global atomic per non-empty bin
// Everything is an integer sum: the result does not depend on the order of the atomics.
#pragma once

namespace clk {

constexpr int kGcBins = 101;                               // CL_GC_BINS
constexpr int kGcPad = 512;                                // CL_GC_MAX_WINDOW / 2, a whole number of pairs
constexpr int kGcWords = (kDepthT + 2 * kGcPad) / 32;      // 32-bit words of a plane a workgroup holds
// what the kernel adds to, in 64-bit words: positions[kGcBins] and the skipped positions behind them, then zero_raw,
// sum_raw, sum_qc [kGcBins] each
constexpr int kGcOutWords = 4 * kGcBins + 1;
static_assert(kGcPad % 64 == 0 && kGcWords / 2 <= 64, "a lane of wave 0 loads a pair");

struct GcArgs {
    DepthResidents res;
    const uint4 *bits;                 // (n_win * 2048 + 2 * kGcPad) / 64 pairs {gc lo, gc hi, valid lo, valid hi}
    uint32_t window, max_invalid;      // 1 <= window <= 2 * kGcPad, max_invalid < window
    unsigned long long *out;           // [kGcOutWords]
};

// the set bits of a plane below bit x of the workgroup's stretch (x < 32 kGcWords)
__device__ __forceinline__ uint32_t gc_below(const uint32_t *words, const uint32_t *pre, uint32_t x)
{
    return pre[x >> 5] + (uint32_t)__builtin_popcount(words[x >> 5] & ((1u << (x & 31u)) - 1u));
}
// the 16 bits of a plane from bit x on (x + 16 <= 32 kGcWords; the word behind the stretch is zero)
__device__ __forceinline__ uint32_t gc_field(const uint32_t *words, uint32_t x)
{
    const unsigned long long two = ((unsigned long long)words[(x >> 5) + 1u] << 32) | words[x >> 5];
    return (uint32_t)(two >> (x & 31u)) & 0xFFFFu;
}
// num / den for num <= 100 * 1024 and 1 <= den <= 1024 with num <= 100 den: both are exact in f32, the quotient is at
// most 100 and the product with the reciprocal is off by less than 2^-15, so the estimate is off by at most 1
__device__ __forceinline__ uint32_t gc_quot(uint32_t num, uint32_t den)
{
    uint32_t q = (uint32_t)((float)num * __builtin_amdgcn_rcpf((float)den));
    if (q * den > num) --q;
    if ((q + 1u) * den <= num) ++q;
    return q;
}

template <int NP, bool HEAD4>
__global__ __launch_bounds__(kDepthBlock) void k_gc_bias(GcArgs a)
{
    constexpr int T = kDepthT, BS = kDepthBlock, PER = kDepthPer;
    __shared__ __attribute__((aligned(16))) uint32_t s_diff[T];
    __shared__ uint32_t s_pl[NP][64];                      // wave 1's planes, then the window's (written by wave 0)
    __shared__ uint32_t s_tot;                             // wave 0's total of the differences
    __shared__ uint32_t s_bw[2][kGcWords + 1];             // gc, valid: the stretch's words and a zero word
    __shared__ uint32_t s_bp[2][kGcWords + 1];             // ... the set bits in front of each word
    __shared__ uint32_t s_cnt[2][kGcBins + 1];             // positions (slot kGcBins: skipped), zero_raw
    __shared__ unsigned long long s_sum[2][kGcBins];       // sum_raw, sum_qc

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t Wn = a.window, K = a.max_invalid;
    for (uint32_t i = tid; i < 2u * (kGcBins + 1); i += BS) (&s_cnt[0][0])[i] = 0u;
    for (uint32_t i = tid; i < 2u * kGcBins; i += BS) (&s_sum[0][0])[i] = 0ull;

    for (uint32_t w = blockIdx.x; w < a.res.n_win; w += gridDim.x) {
        const uint32_t W = w * (uint32_t)T;
        const WinMeta wm = a.res.win[w];
        const RowLane rl = row_lane(a.res.rows, wm, lane, wv);

        wd_clear(s_diff, tid);
        if (wv == 0) {
            // ---- the two planes over [W - kGcPad, W + T + kGcPad): pair w * (T / 64) is the first ----
            uint4 b = make_uint4(0u, 0u, 0u, 0u);
            if (lane < (uint32_t)(kGcWords / 2)) b = a.bits[(size_t)w * (T / 64) + lane];
            const uint32_t n_gc = (uint32_t)(__builtin_popcount(b.x) + __builtin_popcount(b.y));
            const uint32_t n_va = (uint32_t)(__builtin_popcount(b.z) + __builtin_popcount(b.w));
            const uint32_t both = n_gc | (n_va << 16);     // (either total is at most 32 kGcWords = 3072)
            const uint32_t excl = dpp_incl_scan_u32(both) - both;
            if (lane <= (uint32_t)(kGcWords / 2)) {        // (lane kGcWords / 2: the zero word and the totals)
                s_bw[0][2u * lane] = b.x; s_bw[1][2u * lane] = b.z;
                s_bp[0][2u * lane] = excl & 0xFFFFu; s_bp[1][2u * lane] = excl >> 16;
            }
            if (lane < (uint32_t)(kGcWords / 2)) {
                s_bw[0][2u * lane + 1u] = b.y; s_bw[1][2u * lane + 1u] = b.w;
                s_bp[0][2u * lane + 1u] = (excl & 0xFFFFu) + (uint32_t)__builtin_popcount(b.x);
                s_bp[1][2u * lane + 1u] = (excl >> 16) + (uint32_t)__builtin_popcount(b.z);
            }
        }
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
        const DepthSpan sp = wd_span(W, tid, a.res.extent);
        const uint32_t n_ok = sp.n_ok;
        // ---- the bins of the thread's positions: position i's window is the bits [lo0 + i, lo0 + i + Wn) ----
        uint32_t vb[PER];
        {
            const uint32_t lo0 = tid * (uint32_t)PER + (uint32_t)kGcPad - (Wn >> 1), hi0 = lo0 + Wn;   // hi0 + 16 <= 32 kGcWords
            uint32_t g = gc_below(s_bw[0], s_bp[0], hi0) - gc_below(s_bw[0], s_bp[0], lo0);
            uint32_t v = Wn - (gc_below(s_bw[1], s_bp[1], hi0) - gc_below(s_bw[1], s_bp[1], lo0));       // the invalid bases
            const uint32_t out_g = gc_field(s_bw[0], lo0), in_g = gc_field(s_bw[0], hi0);
            const uint32_t out_v = gc_field(s_bw[1], lo0), in_v = gc_field(s_bw[1], hi0);
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                vb[i] = v > K ? (uint32_t)kGcBins : gc_quot(100u * g, Wn - (v > K ? 0u : v));
                g += ((in_g >> i) & 1u) - ((out_g >> i) & 1u);
                v += ((out_v >> i) & 1u) - ((in_v >> i) & 1u);
            }
        }
        // ---- a run of equal bins among the thread's positions is one atomic a table ----
        {
            uint32_t run_n = 0u, run_z = 0u;
            unsigned long long run_r = 0ull, run_q = 0ull;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if ((uint32_t)i < n_ok) {
                    // a run ends at the thread's last position below the extent, or where the next bin differs
                    bool end = (uint32_t)i + 1u == n_ok;
                    if (i + 1 < PER) end |= vb[i + 1 < PER ? i + 1 : i] != vb[i];
                    run_n += 1u; run_z += vr[i] == 0u ? 1u : 0u; run_r += vr[i]; run_q += vq[i];
                    if (end) {
                        const uint32_t b = vb[i];          // <= kGcBins
                        atomicAdd(&s_cnt[0][b], run_n);
                        if (b < (uint32_t)kGcBins) {       // (a skipped position's depths are left out)
                            if (run_z) atomicAdd(&s_cnt[1][b], run_z);
                            if (run_r) atomicAdd(&s_sum[0][b], run_r);
                            if (run_q) atomicAdd(&s_sum[1][b], run_q);
                        }
                        run_n = 0u; run_z = 0u; run_r = 0ull; run_q = 0ull;
                    }
                }
            }
        }
        __syncthreads();                                   // the next window's clear, planes and bit words
    }
    __syncthreads();
    // ---- one global atomic per non-empty bin of the workgroup ----
    for (uint32_t i = tid; i < (uint32_t)kGcBins + 1u; i += BS) {
        const uint32_t n = s_cnt[0][i];
        if (n) atomicAdd(&a.out[i], (unsigned long long)n);
    }
    for (uint32_t i = tid; i < (uint32_t)kGcBins; i += BS) {
        const uint32_t z = s_cnt[1][i];
        const unsigned long long r = s_sum[0][i], q = s_sum[1][i];
        if (z) atomicAdd(&a.out[kGcBins + 1 + i], (unsigned long long)z);
        if (r) atomicAdd(&a.out[2 * kGcBins + 1 + i], r);
        if (q) atomicAdd(&a.out[3 * kGcBins + 1 + i], q);
    }
}

} // namespace clk
