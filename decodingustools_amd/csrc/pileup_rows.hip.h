// pileup_rows.hip.h -- k_pileup_rows, the pass-bit form of the pileup (the product), and everything only it and the
// depth profile beside it (depth_profile.hip.h: the same rows and heads, the same adders) use.  It shares with the byte
// forms (pileup_bytes.hip.h) what kernels.hip.h holds and nothing else.
#pragma once
#include "kernels.hip.h"

namespace clk {

// k_pileup_rows reads HEADS, in their general form 8 bytes each: {pos, span | low << 31} -- the read as the pileup holds
// it, [pos, pos + span) (span = bam_cigar2rlen: D and N included; mod.rs:22-28), and whether its mapq is at or below
// max_low_mapq (mod.rs:26-28).  Nothing else of a read is needed there: its M/=/X bases are in the rows, and its shares of
// summed_coverage and summed_mapq (contig_profiler.rs:74, 79-82: per-read separable) are added up by
// cl_push_reads' walk on the host.  A span of more than kHeadSpanMax positions (engine_limits.h: 2^31 - 1) is cut into
// several heads (the +-1 scatter of [a, b) and [b, c) is that of [a, c)); a read without a reference span has none.
//
// HEAD4, the 4-byte form of the same: pos & 0xFFFF | span << 16 | low << 31 -- for a contig in which every span fits 15
// bits and none was cut (callable_loci.hip: no wide read, that is no span beyond kWideSpan = 16 384, and no head span
// below a read's).  A window W reads only its ordinary candidates, W - 16 384 < pos < W + T, so 16 bits of the position
// say where it lies: pos - W = (int16)(pos16 - W16), in (-16 384, 2 048).  The same head serves every window that reads
// it.  One wide read anywhere keeps the whole contig on 8-byte heads.
template <bool HEAD4> struct HeadOf { typedef uint2 type; };
template <> struct HeadOf<true> { typedef uint32_t type; };
template <bool HEAD4> __device__ __forceinline__ typename HeadOf<HEAD4>::type head_at(const void *heads, uint32_t r)
{
    return reinterpret_cast<const typename HeadOf<HEAD4>::type *>(heads)[r];
}
// What the kernels that scatter a window's candidates need of a head (k_pileup_rows, k_depth_profile, k_depth_runs): the
// span clipped to the window [W, W + T) as [cb, ce) -- ce may be T or beyond: nothing ends inside the window then --,
// whether the read's mapq counts as low, and whether the head touches the window at all (a zeroed head, a head of a cut
// span that lies elsewhere, a read that ends in front of the window: hit = false and nothing else is to be used).
struct HeadCand { uint32_t cb, ce, low; bool hit; };
template <int T> __device__ __forceinline__ HeadCand head_cand(const uint2 h, uint32_t W)
{
    const uint32_t x = h.x, span = h.y & kHeadSpanMax, e = x + span;
    return HeadCand{x > W ? x - W : 0u, e - W, h.y >> 31, span && e > W && x < W + (uint32_t)T};
}
template <int T> __device__ __forceinline__ HeadCand head_cand(const uint32_t h, uint32_t W)
{
    const int32_t span = (int32_t)((h >> 16) & 0x7FFFu), dx = (int32_t)(int16_t)(uint16_t)(h - W), e = dx + span;
    return HeadCand{(uint32_t)(dx > 0 ? dx : 0), (uint32_t)e, h >> 31, span && e > 0 && dx < T};
}

// What the kernels that read a window's rows need of its record (k_pileup_rows, k_depth_profile, k_depth_runs).  The
// rows lie in UNITS of 128 bytes (pass_rows.h): 4 rows of one SEGMENT of 256 positions, the 8 blocks of lanes 8 s ..
// 8 s + 7, 16 bytes per lane.  Segment s has a stack of h_s units of its own; a window's units are contiguous, segment
// after segment, from unit wm.rlo.  The eight heights are the bytes of wm.q0 (segment 0 lowest); q0 == 0 is the
// equal-heights form, every segment wm.rn units (a window with a segment beyond 255 units, and DUT_ROWS_UNIFORM=1).
// wm.rn is the largest height: the wave's loop bound.
//
// The units are read through a buffer descriptor of the WINDOW's own bytes, and a lane whose segment has no unit k asks
// for an offset beyond the descriptor: the load returns zeros without touching memory.  That is straight code -- no
// branch around a load, every add waits for its own load only -- and a segment lower than the window's highest simply
// adds zeros for the units beyond it.  A lane gets the byte offset of its 16 bytes of unit g0 of its segment (g0: the
// first unit its wave takes) and how many units the segment has from there on (n <= 0 for none).  Relative to g0, so
// that the k of an unrolled loop is a constant: the load of unit g0 + k takes its k x 128 from the INSTRUCTION's
// immediate offset (row_unit), and the lane's own part is one compare and one select, k < n ? off : kRowNoUnit, the
// same constant for every k.  What keeps a lane inside its window's units:
//   k < n    the select: off + 128 k is then unit g0 + k of the lane's own segment, which the window has (the heights
//            are the window's own record, and the host has checked rlo + units against the resident rows);
//   else     the descriptor: the immediate offset is part of the offset that the range check looks at (a SCALAR offset
//            would not be), kRowNoUnit + 128 k is beyond every descriptor (num_records < 2^31) and does not wrap.
// (The upload refuses a window whose units take 2^31 bytes or more, so offsets fit 32 bits: callable_loci.hip, size_for_extent.)
typedef unsigned int RowWords __attribute__((ext_vector_type(4)));
constexpr uint32_t kRowNoUnit = 0x80000000u;               // an offset no window's descriptor reaches (and + 128 k neither: 128 k < 2^31)
struct RowLane { __amdgpu_buffer_rsrc_t rs; uint32_t off; int32_t n; };
__device__ __forceinline__ RowLane row_lane(const uint4 *rows, const WinMeta &wm, uint32_t lane, uint32_t g0)
{
    const uint32_t s = lane >> 3;
    uint32_t n = wm.rn, first = s * wm.rn, units = 8u * wm.rn;
    if (wm.q0) {
        n = (uint32_t)(wm.q0 >> (8u * s)) & 0xFFu;
        // the heights below s: the bytes of q0 under byte s, summed four at a time (v_sad_u8 against 0)
        const unsigned long long below = wm.q0 & ((1ull << (8u * s)) - 1ull);
        first = __builtin_amdgcn_sad_u8((uint32_t)below, 0u, __builtin_amdgcn_sad_u8((uint32_t)(below >> 32), 0u, 0u));
        // ... and all eight, in scalar registers: pairs of bytes in 16-bit fields, then the fields
        const uint32_t lo = (uint32_t)wm.q0, hi = (uint32_t)(wm.q0 >> 32);
        const uint32_t f = (lo & 0x00FF00FFu) + ((lo >> 8) & 0x00FF00FFu) + (hi & 0x00FF00FFu) + ((hi >> 8) & 0x00FF00FFu);
        units = (f + (f >> 16)) & 0xFFFFu;
    }
    return RowLane{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(rows + (size_t)wm.rlo * 8u), 0, (int)(units * 128u), 0x00020000),
                   (first + g0) * 128u + (lane & 7u) * 16u, (int32_t)(n - g0)};
}
// the lane's 16 bytes of unit g0 + k of its segment, zeros where the segment has none; g0 on by `by` units
__device__ __forceinline__ uint4 row_unit(const RowLane &rl, int k)
{
    uint32_t o = k < rl.n ? rl.off : kRowNoUnit;
    // (opaque to the optimiser, so that the constant below stays one add behind the select -- which instruction selection
    // folds into the load's immediate offset -- instead of being pushed into both of its arms: a v_add and a v_mov per load)
    asm("" : "+v"(o));
    const RowWords v = __builtin_amdgcn_raw_buffer_load_b128(rl.rs, o + (uint32_t)k * 128u, 0, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void row_advance(RowLane &rl, int by) { rl.off += (uint32_t)by * 128u; rl.n -= by; }
// a head at byte offset `off` of a buffer descriptor of heads, a zeroed one (no candidate) where the offset lies beyond it
typedef unsigned int HeadWords __attribute__((ext_vector_type(2)));
template <bool HEAD4> __device__ __forceinline__ typename HeadOf<HEAD4>::type head_fetch(__amdgpu_buffer_rsrc_t rs, uint32_t off);
template <> __device__ __forceinline__ uint32_t head_fetch<true>(__amdgpu_buffer_rsrc_t rs, uint32_t off)
{
    return __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
}
template <> __device__ __forceinline__ uint2 head_fetch<false>(__amdgpu_buffer_rsrc_t rs, uint32_t off)
{
    const HeadWords v = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
    return make_uint2(v.x, v.y);
}

// ---------------------------------------------------------------------------------------------
// k_pileup_rows: the pass-bit form of the pileup (the default; DUT_QUAL_FORM=bytes selects the byte forms, k_pileup).
//
// "qual >= min_base_quality" (mod.rs:33) is decided once on the host, where the quality bytes are touched anyway
// (cl_push_reads: one bit per base, qual_pack.cpp), and the bits reach the device as ROWS (pass_rows.h): per window a
// stack of T-bit rows, bit p of a row <-> reference position W + p, every read of the window (mapq >= min) alone in its
// stretch of a row.  qc_depth[p] (mod.rs:30-37) is then the column sum of the window's rows -- taken BIT-SLICED: a lane
// owns a block of 32 positions, the window's one wave streams groups of 4 rows (one 16-byte load per lane: a unit of
// 128 bytes per segment of 8 lanes, as many as the segment's own stack is high -- row_lane above --, no masks, no
// shifts), and adds them into NP counter planes (plane k = bit k of the 32 counts) with carry-save adders: three-input
// boolean operations (v_bitop3), 16 or 8 rows through one tree (bs_add16, bs_add8 below), about 2.5 to 3 instructions
// per row for 32 positions.  No LDS atomics, no CIGAR, no offsets.  The planes stay in the lane's registers and are
// compared there -- still bit-sliced -- with min_depth and max_depth (callable_profiler.rs:108-113): two 32-bit masks,
// those of the 32 positions the lane goes on to classify.
// quality_bases is the number of set bits (contig_profiler.rs:71: taken from the planes, sum of 2^p x popcount);
// summed_baseq comes with the bits from the host's walk (contig_profiler.rs:70, per-read separable: SURVEY 8a-7).
//
// The window's candidates are heads (8 or 4 bytes, one per read with a reference span; above): the +-1 scatter of raw_depth
// and low_mapq_count (mod.rs:22-28) into ONE difference array in LDS, nothing else -- the reads' other separable sums
// (summed_coverage, summed_mapq) come from the host's walk too.  Word p of the array is the difference of the PACKED
// count raw_depth + (low_mapq_count << 16) at position W + p: a head adds v = 1 + (low << 16) where it begins and -v
// where it ends, two atomics whatever its mapq.  Sums of such words are linear mod 2^32, so every partial sum (a lane's,
// the scan over the lanes) may wrap and borrow from field to field; the prefix sum AT a position is raw | low << 16
// exactly, because without DEEP a window has at most 32 767 candidates (callable_loci.hip: kNeedDeep): low <= raw <=
// 32 767, bits 15 and 31 clear.  The final phase tests that one word and never splits it (see there).
//
// The final phase works in the BIT DOMAIN: per position only the two tests that need the position's integers (raw_depth
// > 0; the low-MAPQ rule, callable_profiler.rs:100-101) are taken, each leaving one bit; from there a thread's PER
// positions are PER bits of a register -- the reference's N bits (one bit per position in HBM), the two compare masks,
// the priorities of callable_profiler.rs:104-116 as boolean operations on masks, the state as three bit planes, the
// state counts as popcounts, run boundaries as planes ^ (planes << 1 | previous state), the run list by a loop over the
// set bits of the boundary mask.
//
// NP: counter planes -- 8 while no window has more than 255 rows (63 groups), 16 up to 65 535, else 32.
// DEEP: two arrays of 32-bit difference words, raw_depth's and low_mapq_count's (a window with more than 32 767
//       candidates), as in k_pileup.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bs_maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a | b)); }

// 4 rows (one group) into the counter planes: two carry-save adders on plane 0, one on plane 1, a half-adder ripple above
template <int NP>
__device__ __forceinline__ void bs_add4(uint32_t (&c)[NP], const uint4 x)
{
    const uint32_t t0 = c[0] ^ x.x ^ x.y, k0 = bs_maj(c[0], x.x, x.y);
    c[0] = t0 ^ x.z ^ x.w;
    const uint32_t k1 = bs_maj(t0, x.z, x.w);
    uint32_t k = bs_maj(c[1], k0, k1);
    c[1] = c[1] ^ k0 ^ k1;
#pragma unroll
    for (int p = 2; p < NP; ++p) { const uint32_t t = c[p] & k; c[p] ^= k; k = t; }
}

// 8 and 16 rows (2 and 4 groups) at once, as a TREE of carry-save adders: the rows and plane 0 through three-input
// adders (sum = a ^ b ^ c, carry = maj: one v_bitop3 each), their carries and plane 1 through the same, and so on until
// one carry is left -- for plane 3 (8 rows) or 4 (16 rows) --, and only that one ripples through the planes above.  The
// ripple is 12 of bs_add4's 18 operations; here it is paid once per 8 or 16 rows: 24 operations for 8 rows, 38 for 16,
// against 36 and 72.  Exact as bs_add4 is: every adder keeps the weighted sum of what it takes (a + b + c = sum + 2 x
// carry), so the planes hold the old counts + the rows' column sums mod 2^NP, and the one thing dropped is the carry out
// of plane NP - 1.  That carry is zero while the true count is below 2^NP: 8 planes are used up to 63 groups = 252 rows
// (<= 255), 16 up to 65 535 rows, and rows that are zeros (slots a segment does not have: row_unit) add nothing.
__device__ __forceinline__ uint32_t bs_csa(uint32_t &s, uint32_t a, uint32_t b)
{
    const uint32_t k = bs_maj(s, a, b);
    s ^= a ^ b;
    return k;
}
template <int NP>
__device__ __forceinline__ void bs_ripple(uint32_t (&c)[NP], int from, uint32_t k)
{
#pragma unroll
    for (int p = from; p < NP; ++p) { const uint32_t t = c[p] & k; c[p] ^= k; k = t; }
}
template <int NP>
__device__ __forceinline__ void bs_add8(uint32_t (&c)[NP], const uint4 x, const uint4 y)
{
    static_assert(NP >= 4, "the tree of 8 rows ends in plane 2");
    const uint32_t a0 = bs_csa(c[0], x.x, x.y), a1 = bs_csa(c[0], x.z, x.w), a2 = bs_csa(c[0], y.x, y.y), a3 = bs_csa(c[0], y.z, y.w);
    const uint32_t b0 = bs_csa(c[1], a0, a1), b1 = bs_csa(c[1], a2, a3);
    bs_ripple<NP>(c, 3, bs_csa(c[2], b0, b1));
}
template <int NP>
__device__ __forceinline__ void bs_add16(uint32_t (&c)[NP], const uint4 x, const uint4 y, const uint4 z, const uint4 v)
{
    static_assert(NP >= 5, "the tree of 16 rows ends in plane 3");
    const uint32_t a0 = bs_csa(c[0], x.x, x.y), a1 = bs_csa(c[0], x.z, x.w), a2 = bs_csa(c[0], y.x, y.y), a3 = bs_csa(c[0], y.z, y.w);
    const uint32_t a4 = bs_csa(c[0], z.x, z.y), a5 = bs_csa(c[0], z.z, z.w), a6 = bs_csa(c[0], v.x, v.y), a7 = bs_csa(c[0], v.z, v.w);
    const uint32_t b0 = bs_csa(c[1], a0, a1), b1 = bs_csa(c[1], a2, a3), b2 = bs_csa(c[1], a4, a5), b3 = bs_csa(c[1], a6, a7);
    const uint32_t d0 = bs_csa(c[2], b0, b1), d1 = bs_csa(c[2], b2, b3);
    bs_ripple<NP>(c, 4, bs_csa(c[3], d0, d1));
}

// bit i = (the count of position i < K), for the NP planes of a block
template <int NP>
__device__ __forceinline__ uint32_t bs_less_than(const uint32_t (&c)[NP], unsigned long long K)
{
    if (NP < 64 && (K >> NP) != 0ull) return 0xFFFFFFFFu;       // K beyond what NP planes can count to
    uint32_t lt = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int p = NP - 1; p >= 0; --p) {
        if ((K >> p) & 1ull) { lt |= eq & ~c[p]; eq &= c[p]; }
        else eq &= ~c[p];
    }
    return lt;
}

// What k_pileup_rows takes (callable_loci.hip: rows_args fills it, every member, in this order).  Every argument
// that is read takes one or two scalar registers of the wave (they limited the two-wave form's residency; at 5 waves
// per SIMD they no longer do: see the LDS comment in the kernel).
struct RowsArgs {
    const uint4    *rows;         // per window and segment, units of 4 rows x 8 blocks (host, at upload)
    const void     *heads;        // per read with a reference span: 8 bytes, or 4 in an instantiation with HEAD4 (above)
    const uint32_t *wide_idx;     // read indices of the wide reads, ascending
    const WinMeta  *win;
    const uint32_t *refn;         // bit p = the reference base at p is 'N' / 'n' (or beyond the reference)
    const uint32_t *lut8;         // the low-MAPQ thresholds of depths 0..255 as bytes (255 = never): 64 words, built once per
                                  // engine from its options (callable_loci.hip: build_lut8).  Lane l keeps word l; the fast
                                  // path fetches the word of a depth with ds_bpermute, which takes the lane from bits [7:2]
                                  // of its address only, so it is handed the packed word raw | low << 16 as it is
    uint16_t       *runs;
    uint32_t       *win_words;    // per window: n_inner | first state << 16 | last state << 24 (kernels.hip.h: win_word)
    WinRecord      *winpart;      // per window: its totals, 32 bytes (kernels.hip.h)
    unsigned long long *summary;  // the contig summary as 16 words, and the start values of a run (callable_loci.hip: d_sum0):
    const unsigned long long *summary_start;   // the workgroup of window 0 copies them (kernels.hip.h: summary_start)
    uint32_t        extent, n_win, n_win8;
    uint32_t        min_depth, max_depth;
    // the general path (a thread that sees a depth of 255 or more, or DEEP)
    uint32_t        min_depth_for_low_mapq;
    const uint32_t *lut;          // kLutSize entries: smallest low count that is "too many"
    double          max_low_mapq_fraction;
    // DEBUG instantiations only (test dumps; nullptr otherwise)
    uint8_t        *state;
    uint32_t       *dbg_raw, *dbg_qc, *dbg_low;
};

// threads per workgroup: ONE wave per window, 32 positions per thread in the final phase -- the lane that counted a
// block of 32 positions is the thread that classifies them.  (256 -> 128 threads was the measured winner of round 4,
// 128 -> 64 that of round 21, DESIGN.md section 5: what a wave does once per window -- scans, reductions, set-up -- is
// done once, and nothing travels between waves: no barrier waits, no planes or masks through LDS.)
constexpr int kRowsBlock = 64;
// The waves per SIMD the register allocation is to leave room for.  LDS admits 20 workgroups per CU for every form
// without DEEP (8 192 bytes: 5 waves per SIMD, 96 vector registers) and 10 with it (16 384 bytes).  The production
// form (8 planes) takes the 5.  The forms with more planes hold 16 or 32 of them beside the 48 row registers and are
// given the registers instead: 4 waves (128) for 16 planes, 3 (168) for 32 planes and for DEEP, which keeps 10
// workgroups on 4 SIMDs.  The DEBUG forms (test dumps) keep the planes alive through the final phase for the dump of
// qc_depth and get one wave less than their form (at its registers the forms of 8 and of 32 planes spill), the form of
// 8 planes without DEEP two less: its walk holds the lane's 32 packed words beside the dumps' addresses and spills at 128.
constexpr int rows_min_waves(bool DEBUG, bool DEEP, int NP)
{
    return ((DEEP || NP > 16) ? 3 : (NP > 8 ? 4 : 5)) - (DEBUG ? (!DEEP && NP <= 8 ? 2 : 1) : 0);
}
template <int T, bool DEBUG, bool DEEP, int NP, bool HEAD4>
__global__ __launch_bounds__(kRowsBlock, rows_min_waves(DEBUG, DEEP, NP)) void k_pileup_rows(RowsArgs a)
{
    constexpr int kBlock = kRowsBlock;                     // (shadows the namespace's 256 inside this kernel)
    constexpr int PER = T / kBlock;
    static_assert(PER == 32 && T == 2048 && kBlock == 64, "a lane owns a block of 32 positions: T = 64 x 32, one wave");
    constexpr int G = 12;                                  // groups the wave has in flight: 48 rows before a second trip
    // LDS: the difference array and nothing else -- T packed words (raw + (low << 16): the kernel's comment), exactly
    // 8 192 bytes; with DEEP two arrays of T words, 16 384.  8 192 bytes admit 20 workgroups = 20 windows in flight per
    // CU (the kernel's time follows the number of windows a CU has in flight: profiles/r04_occupancy.txt).  With one wave per workgroup that is 5 waves per SIMD: at most 96 vector registers;
    // scalar registers do not bind (800 / 5).  One byte more of LDS would cost a workgroup per CU, so the byte
    // thresholds stay in registers (wlut, below).
    // The array is cleared, added to (atomics) and read by the same wave: what has to be ordered is that wave's own
    // LDS operations.  __syncthreads() is used for it -- in a workgroup of one wave it is the wait for the LDS counter
    // and a fence for the compiler, no s_barrier that anybody waits at.
    __shared__ __attribute__((aligned(16))) uint32_t s_diff[DEEP ? 2 * T : T];
    uint32_t *const s_raw = s_diff, *const s_low = s_diff + T;             // (DEEP only: raw_depth's words, low_mapq_count's)
#ifdef CL_ROWS_LDS_PAD
    __shared__ uint32_t s_pad[CL_ROWS_LDS_PAD / 4];        // (occupancy experiments only)
    s_pad[threadIdx.x] = threadIdx.x;
#endif

    const uint32_t w = (blockIdx.x & 7u) * a.n_win8 + (blockIdx.x >> 3);   // XCD-contiguous window ranges
    if (w >= a.n_win) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t W = w * (uint32_t)T;
    const uint32_t p0 = W + lane * PER;

    const WinMeta wm = a.win[w];
    const uint32_t lo = wm.lo, hi = wm.hi, wlo = wm.wlo, wn = wm.wn;
    const uint32_t n_cand = wn + (hi - lo);
    const uint32_t ng = wm.rn;                             // groups of 4 rows: the highest of the window's segments
    RowLane rl = row_lane(a.rows, wm, lane, 0u);

    // requested first, needed last: the window's rows (the first G groups of every segment), the reference bits
    // (a lane gets the units its segment has, and zeros for the rest: row_lane)
    uint4 rv[G];
#pragma unroll
    for (int j = 0; j < G; ++j) rv[j] = row_unit(rl, j);
    // ... and the window's first candidates: heads (above), U per lane and trip -- 512 in the first trip, which covers
    // a window of a 30x short-read contig (about 430), so that no second, dependent load stands behind the first
    constexpr int U = 8;
    typedef typename HeadOf<HEAD4>::type Head;
    // The ordinary candidates [lo, hi) are read through a buffer descriptor of exactly their heads, as the rows are: a
    // slot that is no ordinary candidate (a wide one, v < wn, or one past the last) asks for an offset beyond the
    // descriptor and gets a zeroed head -- no candidate -- without touching memory.  So the U loads of a trip are
    // straight code that is issued back to back behind the rows'.  (With a branch around each load, every head waited
    // for all the loads before it, the rows included: 4 dependent round trips to memory per wave before round 21.)
    // Wide candidates are rare and come first: only a trip that has some (a scalar test) fetches them, index then head.
    const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(static_cast<const char *>(a.heads) + (size_t)lo * sizeof(Head)), 0, (int)((hi - lo) * (uint32_t)sizeof(Head)), 0x00020000);
    // A trip of a window without wide candidates (a scalar test; every window of a short-read contig): slot v of the
    // trip is head v of the descriptor, so the descriptor's own range check is the whole validity test.  The lane forms
    // the byte offset of its first slot once, and slot u, 64 u heads on, takes its distance from the load's immediate
    // offset (at most 7 x 64 x 8 bytes): no vector instruction per load.  Nothing wraps: base < n_cand < 2^28 here, so
    // the offsets stay below 2^31 + 4 096, and every one at or beyond (hi - lo) x sizeof(Head) returns a zeroed head.
    const bool plain_heads = wn == 0u && n_cand < (1u << 28);
    auto load_heads = [&](uint32_t base, Head (&hh)[U]) {
        if (plain_heads) {
            const uint32_t ob = (base + lane) * (uint32_t)sizeof(Head);
#pragma unroll
            for (int u = 0; u < U; ++u) hh[u] = head_fetch<HEAD4>(hrs, ob + (uint32_t)(u * kBlock) * (uint32_t)sizeof(Head));
            return;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t o = base + (uint32_t)u * kBlock + lane - wn;      // (wraps for a wide slot: beyond hi - lo)
            // (0xFFFFFFF0: beyond the heads of any window -- fewer than 2^29 of at most 8 bytes --, and + 7 does not wrap)
            hh[u] = head_fetch<HEAD4>(hrs, o < hi - lo ? o * (uint32_t)sizeof(Head) : 0xFFFFFFF0u);
        }
        if (wn > base) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t v = base + (uint32_t)u * kBlock + lane;
                if (v < wn) {
                    const uint32_t r = a.wide_idx[wlo + v];
                    __builtin_assume(r < (1u << 29));
                    hh[u] = head_at<HEAD4>(a.heads, r);
                }
            }
        }
    };
    Head hh[U];
    load_heads(0u, hh);
    // ... and the lane's word of the byte thresholds: those of depths 4 lane .. 4 lane + 3.  The 256 bytes stay in the
    // wave's registers; the fast path below fetches the word of depth d from lane d >> 2 (ds_bpermute: no LDS memory)
    const uint32_t wlut = a.lut8[lane];
    // (bit p of refn: the reference base at p is 'N' / 'n' or lies beyond the reference, mod.rs:79-80, :100-101)
    const uint32_t refn = a.refn[(size_t)w * (T / 32) + lane];

    // ---- clear ----
    {
        uint4 *d4 = reinterpret_cast<uint4 *>(s_diff);
#pragma unroll
        for (int i = 0; i < (DEEP ? 2 * T : T) / 4 / kBlock; ++i) d4[i * kBlock + lane] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();                                       // (this wave's clear before its atomics: see the LDS comment)

    // ---- the window's rows: every group into the lane's own counter planes.  The group count is in a scalar register,
    //      so the tests on group numbers are scalar branches: a group slot past the window's highest segment costs
    //      nothing, and the loads of a next trip are only issued when there is one (some segment with more than 12
    //      groups: depth beyond 48).  The planes never leave the registers ----
    uint32_t c[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) c[p] = 0u;
    if (ng) {
        for (uint32_t g0 = 0; g0 < ng; g0 += (uint32_t)G) {
            // (a chunk of four group slots: 16 rows through one tree when the window's highest segment has three or four
            // groups there, 8 rows when it has one or two -- slots a segment does not have hold zeros --, nothing when
            // it has none)
#pragma unroll
            for (int j = 0; j < G; j += 4) {
                if (g0 + (uint32_t)j + 2u < ng) bs_add16<NP>(c, rv[j], rv[j + 1], rv[j + 2], rv[j + 3]);
                else if (g0 + (uint32_t)j < ng) bs_add8<NP>(c, rv[j], rv[j + 1]);
            }
            if (g0 + (uint32_t)G < ng) {                   // a deeper window: the next trip's groups (requested only now)
                row_advance(rl, G);
#pragma unroll
                for (int j = 0; j < G; ++j) rv[j] = row_unit(rl, j);
            }
        }
    }
    // ---- the window's candidates.  +-1 at the clipped span ends (mod.rs:22-28: every read covering a position counts,
    //      D/N included).  The first trip's heads were requested at the top and have arrived behind the rows ----
    for (uint32_t base = 0;;) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const HeadCand hc = head_cand<T>(hh[u], W);
            // (a head of a cut span may lie past the window; a zeroed head: no candidate in this slot)
            if (hc.hit) {
                const uint32_t cb = hc.cb, ce = hc.ce;
                if (DEEP) {
                    atomicAdd(&s_raw[cb], 1u);
                    if (ce < (uint32_t)T) atomicAdd(&s_raw[ce], 0xFFFFFFFFu);
                    if (hc.low) {
                        atomicAdd(&s_low[cb], 1u);
                        if (ce < (uint32_t)T) atomicAdd(&s_low[ce], 0xFFFFFFFFu);
                    }
                } else {
                    // both counts in one word: two atomics per head whatever its mapq
                    const uint32_t v = 1u + (hc.low << 16);
                    atomicAdd(&s_diff[cb], v);
                    if (ce < (uint32_t)T) atomicAdd(&s_diff[ce], 0u - v);
                }
            }
        }
        base += (uint32_t)U * kBlock;
        if (base >= n_cand) break;
        load_heads(base, hh);
    }
    __syncthreads();                                       // (this wave's atomics before its reads: see the LDS comment)

    // ---- final phase: depths, low-MAPQ rule, state, counts -- the lane's own 32 positions, bit i <-> position p0 + i ----
    // qc_depth against the two depth thresholds (callable_profiler.rs:108-113), bit-sliced on the lane's own planes
    const uint32_t ltb = bs_less_than<NP>(c, (unsigned long long)a.min_depth);
    // qc > max_depth  <=>  !(qc < max_depth + 1); the rule is off for max_depth == 0
    const uint32_t gtb = a.max_depth > 0u ? ~bs_less_than<NP>(c, (unsigned long long)a.max_depth + 1ull) : 0u;
    // quality_bases (contig_profiler.rs:71): the sum of the block's 32 counts = sum over the planes of 2^p x set bits
    unsigned long long nbits = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) nbits += (unsigned long long)__popc(c[p]) << p;

    // The lane's differences: its 32 packed words (DEEP: 32 words of either array, re-read from LDS where they are
    // needed), and first their sum, for the scan over the lanes.  A packed word is the difference of raw + (low << 16)
    // at its position, and everything from here to the running sum is linear mod 2^32: the lane's sum, the scan over
    // the lanes and the offsets may wrap and borrow between the fields as they like (a lane's sum may well be negative
    // in either field: ends without starts) -- one chain of adds and ONE scan serve both counts.  What is exact is the
    // running sum AT a position: raw | low << 16 with low <= raw <= 32 767, for without DEEP a window has at most
    // 32 767 candidates (callable_loci.hip: kNeedDeep).  Bit 15 and bit 31 of it are clear; the tests below use that.
    constexpr int NX = DEEP ? 1 : PER;                     // packed words that the lane holds
    uint32_t x[NX];
    uint32_t tr = 0, tl = 0;                               // (tr: the packed sum; tl: DEEP only)
    if constexpr (DEEP) {
        x[0] = 0u;
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            const uint4 xq = reinterpret_cast<const uint4 *>(s_raw)[lane * (PER / 4) + q];
            const uint4 yq = reinterpret_cast<const uint4 *>(s_low)[lane * (PER / 4) + q];
            tr += xq.x + xq.y + xq.z + xq.w; tl += yq.x + yq.y + yq.z + yq.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < NX / 4; ++q) {
            const uint4 xq = reinterpret_cast<const uint4 *>(s_diff)[lane * (NX / 4) + q];
            x[4 * q] = xq.x; x[4 * q + 1] = xq.y; x[4 * q + 2] = xq.z; x[4 * q + 3] = xq.w;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) tr += x[i];
    }
    // (two's complement in 32 bits; with DEEP the two scans stay separate)
    const uint32_t offr = dpp_incl_scan_u32(tr) - tr;
    uint32_t offl = 0u;
    if constexpr (DEEP) offl = dpp_incl_scan_u32(tl) - tl;

    // raw_depth > 0, and the low-MAPQ rule (callable_profiler.rs:100-101): the two per-position tests, each a difference
    // whose sign bit says "no", shifted into a mask by v_alignbit ({mask, d} >> 31) as the running sums walk the lane's
    // positions upwards: position 0 ends in bit 31, one v_bfrev per mask puts it right.  No array of depths is held.
    uint32_t covb = 0, lowb = 0, mx = 0;
    if constexpr (!DEEP) {
        // The fast path: the thresholds as bytes, trusted while the lane sees no depth of 255 or more (255 = never; a
        // count is at most the depth).  raw - 1 wraps when raw == 0; low - threshold is negative when low < threshold.
        // The byte of depth d: word d >> 2 of the table, held by that lane (a wrong lane's word beyond 255: not used).
        // Eight positions at a time: their depths first and the eight fetches behind each other, then the tests, so
        // that the wave waits for one round trip per eight positions and not for one per position.
        //
        // One running word s = raw | low << 16 serves all of it, its fields never split:
        //   the fetch: ds_bpermute takes the lane from bits [7:2] of its address and nothing else, so it is given s
        //     itself -- bits [7:2] of raw, raw >> 2 while raw < 256; v_alignbyte takes its byte count from bits [1:0]
        //     of s, raw & 3, and turns the fetched word so that the byte of depth raw is its lowest;
        //   raw > 0: (s << 16) - 0x10000 = (raw - 1) << 16, negative for raw == 0 only, because raw < 32 768 (bit 15
        //     clear: raw << 16 is not negative itself).  The signed maximum of these words is that of raw - 1;
        //   low >= threshold: (s >> 16) - (the turned word & 0xFF), written so that it is ONE subtraction with operand
        //     selects (v_sub_u32_sdwa, word 1 of s and byte 0 of the turned word: read in the listing, no assembly).
        uint32_t s = offr, ncov = 0, nlow = 0;
        int32_t mc = -0x10000;                             // the largest (raw - 1) << 16 of the lane
        constexpr int B = 8;
#pragma unroll
        for (int g = 0; g < PER; g += B) {
            uint32_t s8[B], t8[B];
#pragma unroll
            for (int k = 0; k < B; ++k) {
                s += x[g + k];
                s8[k] = s;
                t8[k] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)s, (int)wlut);
            }
#pragma unroll
            for (int k = 0; k < B; ++k) {
                const uint32_t thr = __builtin_amdgcn_alignbyte(t8[k], t8[k], s8[k]) & 0xFFu;
                const uint32_t dc = (s8[k] << 16) - 0x10000u;
                mc = (int32_t)dc > mc ? (int32_t)dc : mc;
                ncov = __builtin_amdgcn_alignbit(ncov, dc, 31);
                nlow = __builtin_amdgcn_alignbit(nlow, (s8[k] >> 16) - thr, 31);
                if (DEBUG) {
                    if (a.dbg_raw) a.dbg_raw[p0 + g + k] = s8[k] & 0xFFFFu;
                    if (a.dbg_low) a.dbg_low[p0 + g + k] = s8[k] >> 16;
                }
            }
        }
        mx = ((uint32_t)mc + 0x10000u) >> 16;
        covb = ~__builtin_bitreverse32(ncov); lowb = ~__builtin_bitreverse32(nlow);
    }
    if (DEEP || mx >= 255u) {
        // The general path, for the lanes that need it (the lane's positions again: its differences from LDS, two
        // positions per step).  The same two sign bits as above, so that no test's outcome waits in a pair of scalar
        // registers for the others: a threshold is clamped to 2^31 - 1 = never (a count is below 2^29), and so is that
        // of a depth below min_depth_for_low_mapq; lut[0] is "never" already (build_lut fills with 0xFFFFFFFF and starts
        // at depth 1).  A depth beyond the table takes the f64 divide (its load of the table's last entry is not used).
        const uint32_t mdl = a.min_depth_for_low_mapq < 0x7FFFFFFFu ? a.min_depth_for_low_mapq : 0x7FFFFFFFu;
        uint32_t sr = offr, sl = offl, ncov = 0, nlow = 0;
        mx = 0;
#pragma unroll 1
        for (int h = 0; h < PER / 2; ++h) {
            uint32_t dr[2], dl[2];
            if (DEEP) {
                dr[0] = s_raw[lane * PER + 2 * h]; dr[1] = s_raw[lane * PER + 2 * h + 1];
                dl[0] = s_low[lane * PER + 2 * h]; dl[1] = s_low[lane * PER + 2 * h + 1];
            } else {                                       // the packed words: sr is the running word, split per position
                dr[0] = s_diff[lane * PER + 2 * h]; dr[1] = s_diff[lane * PER + 2 * h + 1];
                dl[0] = dl[1] = 0u;
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                sr += dr[k]; sl += dl[k];
                const uint32_t raw = DEEP ? sr : sr & 0xFFFFu, low = DEEP ? sl : sr >> 16;
                mx = raw > mx ? raw : mx;
                uint32_t thr = a.lut[raw < kLutSize ? raw : kLutSize - 1u];
                thr = thr < 0x7FFFFFFFu ? thr : 0x7FFFFFFFu;
                thr |= (uint32_t)((int32_t)(raw - mdl) >> 31) >> 1;
                uint32_t d = low - thr;
                if (raw >= kLutSize) {
                    const bool is_low = raw >= a.min_depth_for_low_mapq && ((double)low / (double)raw) > a.max_low_mapq_fraction;   // IEEE f64 divide
                    d = is_low ? 0u : 0x80000000u;
                }
                ncov = __builtin_amdgcn_alignbit(ncov, raw - 1u, 31);
                nlow = __builtin_amdgcn_alignbit(nlow, d, 31);
                if (DEBUG) {
                    if (a.dbg_raw) a.dbg_raw[p0 + 2 * h + k] = raw;
                    if (a.dbg_low) a.dbg_low[p0 + 2 * h + k] = low;
                }
            }
        }
        covb = ~__builtin_bitreverse32(ncov); lowb = ~__builtin_bitreverse32(nlow);
    }
    const uint32_t n_ok = p0 >= a.extent ? 0u : (a.extent - p0 < (uint32_t)PER ? a.extent - p0 : (uint32_t)PER);
    const uint32_t okb = n_ok >= (uint32_t)PER ? 0xFFFFFFFFu : ((1u << n_ok) - 1u);          // positions < extent
    // priorities of callable_profiler.rs:104-116, resolved into disjoint masks:
    // REF_N > NO_COVERAGE > POOR_MAPPING_QUALITY > LOW_COVERAGE > EXCESSIVE_COVERAGE > CALLABLE
    const uint32_t Nk = refn & okb, notN = ~refn & okb, covk = covb & okb;
    const uint32_t t0 = notN & covk;
    const uint32_t rLow = t0 & lowb, t1 = t0 & ~lowb;
    const uint32_t rLT = t1 & ltb, t2 = t1 & ~ltb;
    const uint32_t rGT = t2 & gtb, rC = t2 & ~gtb;
    const uint32_t rNC = notN & ~covk;
    // the state (types.rs:36-43: REF_N 0, CALLABLE 1, NO_COVERAGE 2, LOW_COVERAGE 3, EXCESSIVE_COVERAGE 4,
    // POOR_MAPPING_QUALITY 5) as three bit planes
    const uint32_t s0 = rC | rLT | rLow, s1 = rNC | rLT, s2 = rGT | rLow;
    auto state_at = [&](uint32_t j) -> uint32_t { return ((s0 >> j) & 1u) | (((s1 >> j) & 1u) << 1) | (((s2 >> j) & 1u) << 2); };
    if (DEBUG) {
#pragma unroll 1
        for (uint32_t i = 0; i < (uint32_t)PER; ++i) {
            uint32_t qc = 0;
#pragma unroll
            for (int p = 0; p < NP; ++p) qc |= ((c[p] >> i) & 1u) << p;
            if (a.dbg_qc) a.dbg_qc[p0 + i] = qc;
            a.state[p0 + i] = (uint8_t)(((okb >> i) & 1u) ? state_at(i) : 0xFFu);
        }
    }
    // run boundaries strictly inside the window: position p (> W) whose state differs from p-1.  The state before the
    // lane's first position is the lane below's last; lane 0 takes its own first state (no boundary at the window's
    // first position: the seam between windows is the tail's)
    const uint32_t last_st = state_at((uint32_t)PER - 1u);
    const uint32_t below = (uint32_t)__shfl_up((int)last_st, 1);
    const uint32_t pv = lane > 0 ? below : state_at(0u);
    const uint32_t bnd = ((s0 ^ ((s0 << 1) | (pv & 1u))) | (s1 ^ ((s1 << 1) | ((pv >> 1) & 1u))) | (s2 ^ ((s2 << 1) | (pv >> 2)))) & okb;
    const uint32_t nb = __popc(bnd);
    const uint32_t inc = dpp_incl_scan_u32(nb);            // (lane 63's: the window's n_inner)
    if (nb) {
        uint16_t *dst = a.runs + (size_t)w * T + (inc - nb);
        for (uint32_t m = bnd; m; m &= m - 1u) {             // (a lane has a boundary or two, rarely more)
            const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
            *dst++ = (uint16_t)((lane * PER + j) | (state_at(j) << 12));
        }
    }
    // ---- the window's record (kernels.hip.h: WinRecord) and its packed word.  A lane's counts are <= 32 and the
    //      window's <= 2048: packed words of two 16-bit fields, one inclusive scan each; with 8 planes the window's set
    //      bits (<= 255 x 2048 < 2^19; a lane's <= 255 x 32) ride above the 12 bits of n_cov, so four scans and the
    //      maximum are all.  The totals are LANE 63's scan values, so lane 63 stores them as they stand, and the packed
    //      word with them -- n_inner is its `inc`, the last state its own, the first lane 0's: no total goes through a
    //      scalar register and none is steered into a lane ----
    {
        const uint32_t t0 = dpp_incl_scan_u32(__popc(Nk) | (__popc(rC) << 16));
        const uint32_t t1 = dpp_incl_scan_u32(__popc(rNC) | (__popc(rLT) << 16));
        const uint32_t t2 = dpp_incl_scan_u32(__popc(rGT) | (__popc(rLow) << 16));
        const uint32_t t3 = dpp_incl_scan_u32(__popc(covk) | (NP == 8 ? (uint32_t)nbits << 12 : 0u));
        // (16 planes: the window's set bits are below 2^32, 65 535 x 2048 < 2^27; 32 planes: a 64-bit sum)
        unsigned long long qc = 0;
        if constexpr (NP == 16) qc = dpp_incl_scan_u32((uint32_t)nbits);
        else if constexpr (NP > 16) qc = wave_sum_u64(nbits);
        const uint32_t tm = dpp_incl_max_u32(mx);
        const uint32_t first_w = (uint32_t)__builtin_amdgcn_readfirstlane((int)state_at(0u));
        if (lane == (uint32_t)kBlock - 1u) {
            uint4 *rec = reinterpret_cast<uint4 *>(a.winpart + w);
            rec[0] = make_uint4(t0, t1, t2, t3);
            rec[1] = make_uint4((uint32_t)qc, (uint32_t)(qc >> 32), tm, 0u);
            a.win_words[w] = win_word(inc, first_w, last_st);
        }
    }
    if (w == 0u) summary_start(a.summary, a.summary_start, lane);   // (a scalar branch)
}

} // namespace clk
