// depth_profile.hip.h -- k_depth_profile: the depth distribution of the resident contig, reduced on the device
// (cl_contig_depth_profile, include/callable_loci.h).  Included by callable_loci.hip behind window_depths.hip.h (the
// rebuild of both depths, shared with k_depth_runs and k_target_depth).
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

constexpr int kDepthWinSlots = 2048 / 16 + 2;

struct DepthArgs {
    DepthResidents res;
    uint32_t n_bins, window;           // window = 0: no window table
    unsigned long long *hist;          // [2][n_bins]: raw, qc
    unsigned long long *wins;          // [2][n_windows]: raw, qc (window > 0)
    unsigned long long n_windows;
    unsigned long long *sums;          // [2]: raw, qc
};

template <int NP, bool HEAD4>
__global__ __launch_bounds__(kDepthBlock) void k_depth_profile(DepthArgs a)
{
    constexpr int T = kDepthT, BS = kDepthBlock, PER = kDepthPer;
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

    for (uint32_t w = blockIdx.x; w < a.res.n_win; w += gridDim.x) {
        const uint32_t W = w * (uint32_t)T;
        const WinMeta wm = a.res.win[w];
        const RowLane rl = row_lane(a.res.rows, wm, lane, wv);

        wd_clear(s_diff, tid);
        if (S) for (int i = tid; i < 2 * kDepthWinSlots; i += BS) (&s_win[0][0])[i] = 0ull;
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
        // ---- qc_depth: wd_extract's loop in the kernel's own text.  Through the function this kernel takes 11 to 14
        // registers more (a wave less per SIMD at 8 and 16 planes) or, with the function's asm, 8 more at 8 planes ----
#pragma unroll
        for (int i = 0; i < PER; ++i) vq[i] = 0u;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const uint32_t word = s_pl[p][tid >> 1] >> ((tid & 1u) * 16u);
#pragma unroll
            for (int i = 0; i < PER; ++i) vq[i] |= ((word >> i) & 1u) << p;
        }
        const DepthSpan sp = wd_span(W, tid, a.res.extent);
        const uint32_t p0 = sp.p0, n_ok = sp.n_ok;
        // (positions at and beyond the extent: no read reaches them; they count nowhere)
        unsigned long long a_raw = 0ull, a_qc = 0ull, b_raw = 0ull, b_qc = 0ull;
        uint32_t brk = (uint32_t)PER, k0 = 0u;
        if (S) { k0 = p0 / S; const uint32_t left = S - (p0 - k0 * S); brk = left < (uint32_t)PER ? left : (uint32_t)PER; }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
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
