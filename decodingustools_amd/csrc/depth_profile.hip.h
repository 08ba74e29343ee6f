// depth_profile.hip.h -- k_depth_profile: the depth distribution of the resident contig, reduced on the device
// (cl_contig_depth_profile, include/callable_loci.h).  Included by callable_loci.hip behind pileup_rows.hip.h (bs_add4, bs_maj, the heads).
//
// A kernel of its own beside k_pileup_rows, not a further template flag of it: it reads the same residents (the
// windows' pass-bit rows, heads and window records) and rebuilds raw_depth and qc_depth per position the same way
// (bit-sliced counter planes for qc, a scanned difference array for raw: mod.rs:17-42), but what it does with them
// wants other resources than the classifier -- up to 32 KB of LDS for the histograms, workgroups that stay for many
// windows so that a histogram is flushed once per workgroup and not once per window -- and none of that may reach
// the production instantiation, whose time follows the number of workgroups a CU holds.
//
// Per workgroup (128 threads, a thread owns 16 positions of a window of 2048; windows w = blockIdx.x, + gridDim.x, ...):
//   * the window's rows into the two waves' counter planes (bs_add4), wave 0 adds wave 1's (ripple adder) and leaves
//     the sum in LDS; the +-1 of every candidate head into a 32-bit difference array, scanned per thread and per wave
//   * hist_raw / hist_qc in LDS, min(depth, n_bins - 1): depth changes at read ends only, so a thread merges the equal
//     neighbours among its 16 positions and adds a run's length with one LDS atomic (DESIGN.md has what else was tried
//     for the hot bins)
//   * window sums (window = S positions, S >= 16: a thread's 16 positions touch two windows at most): a 2048-position
//     window touches at most 2048 / 16 + 1 of them; 64-bit LDS slots, one global atomic per touched slot and window
//   * at the end: one global atomic per non-empty bin, and the two exact sums (wave reduction, one atomic per wave)
// Everything is an integer sum: the result does not depend on the order of the atomics.
#pragma once

namespace clk {

constexpr int kDepthBlock = 128;
constexpr int kDepthWinSlots = 2048 / 16 + 2;

struct DepthArgs {
    const WinMeta  *win;
    const void     *heads;            // 8 bytes each, or 4 with HEAD4 (pileup_rows.hip.h)
    const uint32_t *wide_idx;
    const uint4    *rows;
    uint32_t extent, n_win;
    uint32_t n_bins, window;           // window = 0: no window table
    unsigned long long *hist;          // [2][n_bins]: raw, qc
    unsigned long long *wins;          // [2][n_windows]: raw, qc (window > 0)
    unsigned long long n_windows;
    unsigned long long *sums;          // [2]: raw, qc
};

template <int NP, bool HEAD4>
__global__ __launch_bounds__(kDepthBlock) void k_depth_profile(DepthArgs a)
{
    constexpr int T = 2048, BS = kDepthBlock, PER = T / BS;
    static_assert(PER == 16 && BS == 128, "two waves, a lane of the final phase owns half a block of 32 positions");
    __shared__ __attribute__((aligned(16))) uint32_t s_diff[T];
    __shared__ uint32_t s_pl[NP][64];                      // wave 1's planes, then the window's (written by wave 0)
    __shared__ unsigned long long s_win[2][kDepthWinSlots];
    __shared__ uint32_t s_tot;                             // wave 0's total of the differences
    extern __shared__ uint32_t s_hist[];                   // [2][n_bins]: raw, qc

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t nb = a.n_bins, S = a.window;
    for (uint32_t i = tid; i < 2u * nb; i += BS) s_hist[i] = 0u;
    uint32_t *const h_raw = s_hist, *const h_qc = s_hist + nb;
    unsigned long long tot_raw = 0ull, tot_qc = 0ull;

    for (uint32_t w = blockIdx.x; w < a.n_win; w += gridDim.x) {
        const uint32_t W = w * (uint32_t)T;
        const WinMeta wm = a.win[w];
        const uint32_t lo = wm.lo, wlo = wm.wlo, wn = wm.wn;
        const uint32_t n_cand = wn + (wm.hi - lo);
        const uint32_t ng = wm.rn;
        const RowLane rl = row_lane(a.rows, wm, lane, wv);

        // ---- clear (the previous window's readers are behind the barrier at the end of the loop) ----
        {
            uint4 *d4 = reinterpret_cast<uint4 *>(s_diff);
            for (int i = tid; i < T / 4; i += BS) d4[i] = make_uint4(0, 0, 0, 0);
            if (S) for (int i = tid; i < 2 * kDepthWinSlots; i += BS) (&s_win[0][0])[i] = 0ull;
        }
        __syncthreads();

        // ---- the window's rows: groups wv, wv + 2, ... into this wave's counter planes ----
        uint32_t c[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) c[p] = 0u;
        for (int k = 0; wv + (uint32_t)k < ng; k += 2) bs_add4<NP>(c, row_unit(rl, k));
        // ---- the window's candidates: +-1 at the clipped span ends (as k_pileup_rows) ----
        for (uint32_t v = tid; v < n_cand; v += BS) {
            uint32_t r = lo + (v - wn);
            if (v < wn) r = a.wide_idx[wlo + v];
            const HeadCand hc = head_cand<T>(head_at<HEAD4>(a.heads, r), W);
            if (hc.hit) {
                atomicAdd(&s_diff[hc.cb], 1u);
                if (hc.ce < (uint32_t)T) atomicAdd(&s_diff[hc.ce], 0xFFFFFFFFu);
            }
        }
        if (wv != 0) {
#pragma unroll
            for (int p = 0; p < NP; ++p) s_pl[p][lane] = c[p];
        }
        __syncthreads();
        if (wv == 0) {
            uint32_t carry = 0u;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const uint32_t d = s_pl[p][lane];
                const uint32_t s = c[p] ^ d ^ carry;
                carry = bs_maj(c[p], d, carry);
                s_pl[p][lane] = s;                         // (a lane reads and writes its own slots only)
            }
        }
        // ---- raw_depth: the differences scanned ----
        uint32_t vr[PER];
        uint32_t sr = 0;
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            const uint4 d = reinterpret_cast<const uint4 *>(s_diff)[tid * (PER / 4) + q];
            sr += d.x; vr[4 * q] = sr; sr += d.y; vr[4 * q + 1] = sr;
            sr += d.z; vr[4 * q + 2] = sr; sr += d.w; vr[4 * q + 3] = sr;
        }
        const uint32_t ir = dpp_incl_scan_u32(sr);
        if (tid == 63u) s_tot = ir;
        __syncthreads();
        const uint32_t off = ir - sr + (wv ? s_tot : 0u);
        const uint32_t p0 = W + tid * PER;
        const uint32_t n_ok = p0 >= a.extent ? 0u : (a.extent - p0 < (uint32_t)PER ? a.extent - p0 : (uint32_t)PER);
        // ---- qc_depth: the 16 counts of this thread out of the planes of block tid / 2 ----
        uint32_t vq[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) vq[i] = 0u;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const uint32_t word = s_pl[p][tid >> 1] >> ((tid & 1u) * 16u);
#pragma unroll
            for (int i = 0; i < PER; ++i) vq[i] |= ((word >> i) & 1u) << p;
        }
        // (positions at and beyond the extent: no read reaches them; they count nowhere)
        unsigned long long a_raw = 0ull, a_qc = 0ull, b_raw = 0ull, b_qc = 0ull;
        uint32_t brk = (uint32_t)PER, k0 = 0u;
        if (S) { k0 = p0 / S; const uint32_t left = S - (p0 - k0 * S); brk = left < (uint32_t)PER ? left : (uint32_t)PER; }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            vr[i] += off;
            if ((uint32_t)i >= n_ok) { vr[i] = 0u; vq[i] = 0u; }
            if ((uint32_t)i < brk) { a_raw += vr[i]; a_qc += vq[i]; } else { b_raw += vr[i]; b_qc += vq[i]; }
            vr[i] = vr[i] < nb - 1u ? vr[i] : nb - 1u;
            vq[i] = vq[i] < nb - 1u ? vq[i] : nb - 1u;
        }
        tot_raw += a_raw + b_raw; tot_qc += a_qc + b_qc;
        // ---- histograms: a run of equal depths among the thread's positions is one atomic ----
        {
            uint32_t run_r = 0u, run_q = 0u;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if ((uint32_t)i < n_ok) {
                    // a run ends at the thread's last position below the extent, or where the next depth differs
                    bool end_r = (uint32_t)i + 1u == n_ok, end_q = end_r;
                    if (i + 1 < PER) { end_r |= vr[i + 1 < PER ? i + 1 : i] != vr[i]; end_q |= vq[i + 1 < PER ? i + 1 : i] != vq[i]; }
                    run_r += 1u; run_q += 1u;
                    if (end_r) { atomicAdd(&h_raw[vr[i]], run_r); run_r = 0u; }
                    if (end_q) { atomicAdd(&h_qc[vq[i]], run_q); run_q = 0u; }
                }
            }
        }
        // ---- window sums: positions [0, brk) of the thread lie in window k0, the rest in k0 + 1 ----
        const uint32_t kW = S ? W / S : 0u;                // the first window this workgroup's positions touch
        if (S && n_ok) {
            const uint32_t sl = k0 - kW;                   // <= T / S + 1 <= kDepthWinSlots - 2
            if (a_raw) atomicAdd(&s_win[0][sl], a_raw);
            if (a_qc) atomicAdd(&s_win[1][sl], a_qc);
            if (b_raw) atomicAdd(&s_win[0][sl + 1u], b_raw);
            if (b_qc) atomicAdd(&s_win[1][sl + 1u], b_qc);
        }
        __syncthreads();
        if (S) {
            for (uint32_t i = tid; i < 2u * (uint32_t)kDepthWinSlots; i += BS) {
                const uint32_t kind = i / (uint32_t)kDepthWinSlots, sl = i - kind * (uint32_t)kDepthWinSlots;
                const unsigned long long v = s_win[kind][sl];
                // (a slot that got a sum belongs to a position below the extent: its window exists)
                if (v && (unsigned long long)kW + sl < a.n_windows) atomicAdd(&a.wins[kind * a.n_windows + kW + sl], v);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // ---- one global atomic per non-empty bin of the workgroup ----
    for (uint32_t i = tid; i < 2u * nb; i += BS) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&a.hist[i], (unsigned long long)v);
    }
    tot_raw = wave_sum_u64(tot_raw); tot_qc = wave_sum_u64(tot_qc);
    if (lane == 0) {
        if (tot_raw) atomicAdd(&a.sums[0], tot_raw);
        if (tot_qc) atomicAdd(&a.sums[1], tot_qc);
    }
}

} // namespace clk
