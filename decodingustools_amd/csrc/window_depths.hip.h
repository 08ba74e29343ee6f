// window_depths.hip.h -- the rebuild of raw_depth and qc_depth per position of a window out of the residents of a run,
// written once for the three kernels that start from it: k_depth_profile (depth_profile.hip.h), k_depth_runs
// (depth_runs.hip.h) and k_target_depth (depth_targets.hip.h).  Included by callable_loci.hip behind pileup_rows.hip.h
// (the heads, the rows' lanes, bs_add4, bs_maj) and in front of those three.
//
// A workgroup of kDepthBlock = 128 threads takes a window of 2048 positions, a thread 16 of them (mod.rs:17-42):
//   raw   the +-1 of every candidate head at its clipped span ends into a 32-bit difference array in LDS (wd_clear,
//         wd_scatter), scanned per thread and over the wave, wave 0's total in front of wave 1 (wd_diff_scan in front of
//         a barrier, wd_diff_finish behind it)
//   qc    the window's rows into the two waves' bit-sliced counter planes (wd_rows), wave 1's through LDS to wave 0
//         (wd_planes_put, a barrier, wd_planes_add: a ripple adder that leaves the window's planes in LDS), and behind
//         a further barrier a thread's 16 counts out of the planes of block tid / 2 (wd_extract; k_depth_profile has
//         that one loop in its own text, see there)
// and wd_span says which of the thread's positions lie below the extent.  Phases and not one body: k_depth_runs builds
// one kind per call, k_target_depth marks its query points between two of them, and every barrier stays in the kernel,
// where what it separates can be seen.  Every function is inlined, but the compiler optimises a function on its own
// first and does not treat it as text in place: DESIGN.md has the kernels' registers, instructions and times.
#pragma once

namespace clk {

constexpr int kDepthBlock = 128;
constexpr int kDepthT = 2048, kDepthPer = kDepthT / kDepthBlock;
static_assert(kDepthPer == 16 && kDepthBlock == 128, "two waves, a thread's 16 positions are half a block of 32");

// What the three kernels read of a run: the first member of their argument records (callable_loci.hip: depth_residents).
struct DepthResidents {
    const WinMeta  *win;
    const void     *heads;            // 8 bytes each, or 4 with HEAD4 (pileup_rows.hip.h)
    const uint32_t *wide_idx;
    const uint4    *rows;
    uint32_t extent, n_win;
};

// ---- clear (the previous window's readers are behind the barrier at the end of the kernel's loop) ----
__device__ __forceinline__ void wd_clear(uint32_t *s_diff, uint32_t tid)
{
    uint4 *d4 = reinterpret_cast<uint4 *>(s_diff);
    for (int i = tid; i < kDepthT / 4; i += kDepthBlock) d4[i] = make_uint4(0, 0, 0, 0);
}

// ---- the window's rows: groups wv, wv + 2, ... into this wave's counter planes ----
template <int NP>
__device__ __forceinline__ void wd_rows(uint32_t (&c)[NP], const RowLane &rl, uint32_t ng, uint32_t wv)
{
#pragma unroll
    for (int p = 0; p < NP; ++p) c[p] = 0u;
    for (int k = 0; wv + (uint32_t)k < ng; k += 2) bs_add4<NP>(c, row_unit(rl, k));
}

// ---- the window's candidates: +-1 at the clipped span ends (as k_pileup_rows) ----
template <bool HEAD4>
__device__ __forceinline__ void wd_scatter(const DepthResidents &r, const WinMeta &wm, uint32_t W, uint32_t *s_diff, uint32_t tid)
{
    const uint32_t lo = wm.lo, wlo = wm.wlo, wn = wm.wn;
    const uint32_t n_cand = wn + (wm.hi - lo);
    for (uint32_t v = tid; v < n_cand; v += kDepthBlock) {
        uint32_t h = lo + (v - wn);
        if (v < wn) h = r.wide_idx[wlo + v];
        const HeadCand hc = head_cand<kDepthT>(head_at<HEAD4>(r.heads, h), W);
        if (hc.hit) {
            atomicAdd(&s_diff[hc.cb], 1u);
            if (hc.ce < (uint32_t)kDepthT) atomicAdd(&s_diff[hc.ce], 0xFFFFFFFFu);
        }
    }
}

// ---- the plane hand-over: wave 1 puts its planes into LDS; behind a barrier wave 0 adds them to its own and leaves
// ---- the window's there (a lane reads and writes its own slots only) ----
template <int NP>
__device__ __forceinline__ void wd_planes_put(const uint32_t (&c)[NP], uint32_t (*s_pl)[64], uint32_t lane)
{
#pragma unroll
    for (int p = 0; p < NP; ++p) s_pl[p][lane] = c[p];
}
template <int NP>
__device__ __forceinline__ void wd_planes_add(const uint32_t (&c)[NP], uint32_t (*s_pl)[64], uint32_t lane)
{
    uint32_t carry = 0u;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const uint32_t d = s_pl[p][lane];
        const uint32_t s = c[p] ^ d ^ carry;
        carry = bs_maj(c[p], d, carry);
        s_pl[p][lane] = s;
    }
}

// ---- raw_depth: the differences scanned.  In front of a barrier the thread's 16 running sums and its exclusive
// ---- prefix within its wave (returned; wave 0's total goes to s_tot), behind it the offset onto the sums ----
__device__ __forceinline__ uint32_t wd_diff_scan(uint32_t (&vr)[kDepthPer], const uint32_t *s_diff, uint32_t *s_tot, uint32_t tid)
{
    uint32_t sr = 0;
#pragma unroll
    for (int q = 0; q < kDepthPer / 4; ++q) {
        const uint4 d = reinterpret_cast<const uint4 *>(s_diff)[tid * (kDepthPer / 4) + q];
        sr += d.x; vr[4 * q] = sr; sr += d.y; vr[4 * q + 1] = sr;
        sr += d.z; vr[4 * q + 2] = sr; sr += d.w; vr[4 * q + 3] = sr;
    }
    const uint32_t ir = dpp_incl_scan_u32(sr);
    if (tid == 63u) *s_tot = ir;
    return ir - sr;
}
__device__ __forceinline__ void wd_diff_finish(uint32_t (&vr)[kDepthPer], uint32_t excl, const uint32_t *s_tot, uint32_t wv)
{
    const uint32_t off = excl + (wv ? *s_tot : 0u);
#pragma unroll
    for (int i = 0; i < kDepthPer; ++i) vr[i] += off;
}

// ---- qc_depth: the 16 counts of this thread out of the planes of block tid / 2 ----
// (The empty asm keeps a count's chain as it is written, one v_and_or per plane behind the shift: in a function the
// compiler pairs the terms of a count into v_or3, half an instruction more per plane and position, 1 to 2 % of a
// kernel's time.  k_depth_profile keeps this loop in its own text, without the asm: DESIGN.md has why.)
template <int NP>
__device__ __forceinline__ void wd_extract(uint32_t (&vq)[kDepthPer], const uint32_t (*s_pl)[64], uint32_t tid)
{
#pragma unroll
    for (int i = 0; i < kDepthPer; ++i) vq[i] = 0u;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const uint32_t word = s_pl[p][tid >> 1] >> ((tid & 1u) * 16u);
#pragma unroll
        for (int i = 0; i < kDepthPer; ++i) { vq[i] |= ((word >> i) & 1u) << p; asm("" : "+v"(vq[i])); }
    }
}

// The thread's first position and how many of its 16 lie below the extent (no read reaches the others: they count nowhere).
struct DepthSpan { uint32_t p0, n_ok; };
__device__ __forceinline__ DepthSpan wd_span(uint32_t W, uint32_t tid, uint32_t extent)
{
    const uint32_t p0 = W + tid * kDepthPer;
    return DepthSpan{p0, p0 >= extent ? 0u : (extent - p0 < (uint32_t)kDepthPer ? extent - p0 : (uint32_t)kDepthPer)};
}

} // namespace clk
