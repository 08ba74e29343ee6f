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
// The units are read through a buffer descriptor of the WINDOW's own bytes, so that no lane can read outside them
// whatever its offset, and a lane whose segment has no unit k asks for an offset beyond the descriptor: the load
// returns zeros without touching memory.  That is straight code -- no branch around a load, every add waits for its
// own load only -- and a segment lower than the window's highest simply adds zeros for the units beyond it.  A lane
// gets the byte offset of its 16 bytes of unit g0 of its segment (g0: the first unit its wave takes) and how many
// units the segment has from there on (n <= 0 for none).  Relative to g0, so that the k of an unrolled loop is a constant.
// (The upload refuses a window whose units take 2^31 bytes or more, so offsets fit 32 bits: callable_loci.hip, size_for_extent.)
typedef unsigned int RowWords __attribute__((ext_vector_type(4)));
constexpr uint32_t kRowNoUnit = 0x80000000u;               // an offset no window's descriptor reaches (and + 16 k neither)
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
    const RowWords v = __builtin_amdgcn_raw_buffer_load_b128(rl.rs, (k < rl.n ? rl.off : kRowNoUnit) + (uint32_t)k * 128u, 0, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void row_advance(RowLane &rl, int by) { rl.off += (uint32_t)by * 128u; rl.n -= by; }

// ---------------------------------------------------------------------------------------------
// k_pileup_rows: the pass-bit form of the pileup (the default; DUT_QUAL_FORM=bytes selects the byte forms, k_pileup).
//
// "qual >= min_base_quality" (mod.rs:33) is decided once on the host, where the quality bytes are touched anyway
// (cl_push_reads: one bit per base, qual_pack.cpp), and the bits reach the device as ROWS (pass_rows.h): per window a
// stack of T-bit rows, bit p of a row <-> reference position W + p, every read of the window (mapq >= min) alone in its
// stretch of a row.  qc_depth[p] (mod.rs:30-37) is then the column sum of the window's rows -- taken BIT-SLICED: a lane
// owns a block of 32 positions, a wave streams groups of 4 rows (one 16-byte load per lane: a unit of 128 bytes per
// segment of 8 lanes, as many as the segment's own stack is high -- row_lane above --, no masks, no shifts), and adds
// them into NP counter planes (plane k = bit k of
// the 32 counts) with carry-save adders: three-input boolean operations (v_bitop3), about 4.5 instructions per row
// for 32 positions.  No LDS atomics, no CIGAR, no offsets.  The other waves' planes are added by wave 0 and compared --
// still bit-sliced -- with min_depth and max_depth (callable_profiler.rs:108-113): two 32-bit masks per block.
// quality_bases is the number of set bits (contig_profiler.rs:71: taken from the planes, sum of 2^p x popcount);
// summed_baseq comes with the bits from the host's walk (contig_profiler.rs:70, per-read separable: SURVEY 8a-7).
//
// The window's candidates are heads (8 or 4 bytes, one per read with a reference span; above): the +-1 scatter of raw_depth
// and low_mapq_count (mod.rs:22-28) into difference arrays in LDS, nothing else -- the reads' other separable sums
// (summed_coverage, summed_mapq) come from the host's walk too.
//
// The final phase works in the BIT DOMAIN: per position only the two tests that need the position's integers (raw_depth
// > 0; the low-MAPQ rule, callable_profiler.rs:100-101) are taken, each leaving one bit; from there a thread's PER
// positions are PER bits of a register -- the reference's N bits (one bit per position in HBM), the two compare masks,
// the priorities of callable_profiler.rs:104-116 as boolean operations on masks, the state as three bit planes, the
// state counts as popcounts, run boundaries as planes ^ (planes << 1 | previous state), the run list by a loop over the
// set bits of the boundary mask.
//
// NP: counter planes -- 8 while no window has more than 255 rows (63 groups), 16 up to 65 535, else 32.
// DEEP: 32-bit difference words (a window with more than 32 767 candidates), as in k_pileup.
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

// What k_pileup_rows takes (callable_loci.hip: rows_args fills it, every member, in this order).  The scalar registers
// of a wave are one of the three things that limit the production instantiation's residency (see the LDS comment in the
// kernel) and every argument that is read takes one or two of them.
struct RowsArgs {
    const uint4    *rows;         // per window and segment, units of 4 rows x 8 blocks (host, at upload)
    const void     *heads;        // per read with a reference span: 8 bytes, or 4 in an instantiation with HEAD4 (above)
    const uint32_t *wide_idx;     // read indices of the wide reads, ascending
    const WinMeta  *win;
    const uint32_t *refn;         // bit p = the reference base at p is 'N' / 'n' (or beyond the reference)
    const uint32_t *lut8;         // the low-MAPQ thresholds of depths 0..255 as bytes (255 = never): 64 words, built once per
                                  // engine from its options (callable_loci.hip: build_lut8)
    uint16_t       *runs;
    uint8_t        *first_state, *last_state;
    WinPartial     *winpart;
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

// threads per workgroup: 2 waves, 16 positions per thread in the final phase (against 256 threads, the measured winner,
// what a wave does once per window -- scans, reductions, the planes' hand-over -- is done half as often)
constexpr int kRowsBlock = 128;
// the waves per SIMD the register allocation is to leave room for: what LDS admits -- 8 for the production form (16
// workgroups of 2 waves per CU), 7 for 16 planes without DEEP (12 KB: 13 workgroups), 3 for the large forms; the
// DEBUG forms (test dumps: s_dbg adds 2 to 8 KB of LDS) keep the bounds they always had
constexpr int rows_min_waves(bool DEBUG, bool DEEP, int NP)
{
    if (DEBUG) return (DEEP || NP > 8) ? 3 : 6;
    return (DEEP || NP > 16) ? 3 : (NP > 8 ? 7 : 8);
}
template <int T, bool DEBUG, bool DEEP, int NP, bool HEAD4>
__global__ __launch_bounds__(kRowsBlock, rows_min_waves(DEBUG, DEEP, NP)) void k_pileup_rows(RowsArgs a)
{
    constexpr int kBlock = kRowsBlock;                     // (shadows the namespace's 256 inside this kernel)
    constexpr int PER = T / kBlock;
    static_assert(PER == 16 && T == 2048, "a lane owns a block of 32 positions: T = 64 x 32");
    constexpr int kWaves = kBlock / 64;
    constexpr int kDiffWords = DEEP ? T : T / 2;
    constexpr int G = 6;                                   // groups a wave has in flight: 12 per window before a second trip
    __shared__ __attribute__((aligned(16))) uint32_t s_raw[kDiffWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_low[kDiffWords];
    // LDS: the two difference arrays and ONE pool that is used twice -- 10 240 bytes in all, which admits 16 workgroups
    // per CU (the kernel's time follows the number of workgroups a CU runs: profiles/r04_occupancy.txt).  LDS is one of
    // three limits and with 2 waves per workgroup all three must allow 8 waves per SIMD: at most 64 vector registers,
    // and at most 80 scalar registers (.sgpr_count; 81..96 leave 7 waves = 14 workgroups, 97.. leave 6 = 12, which is
    // where this kernel stood while the compiler's own figure said 8: profiles/r11_rows_residency.json):
    //   first   the counter planes of waves 1.. (wave 0 adds them to its own after the barrier; it is their only reader)
    //   then    s_lt / s_gt and the low-MAPQ thresholds s_lut: a lane of wave 0 writes its words after it has read its
    //           planes (they lie in the slots of that lane's own planes 0, 1 and kLutPlane of wave 1); s_last, s_wtot, s_wmax:
    //           written behind the NEXT barrier, when wave 0 is long done with the planes
    // (the waves' totals for the prefix sums across waves travel in the difference arrays: a lane's own, consumed slot)
    constexpr int kPoolWords = (kWaves - 1) * NP * 64;
    constexpr int kTenantsEnd = 128 + kBlock / 4 + kWaves * 24 + kWaves;        // words: s_lt, s_gt, s_last, s_wtot, s_wmax
    constexpr int kLutPlane = (kTenantsEnd + 63) / 64;                          // the thresholds: the first whole plane behind them
    static_assert(NP >= 8 && kLutPlane < NP && kPoolWords >= (kLutPlane + 1) * 64, "the pool holds its second tenants");
    __shared__ __attribute__((aligned(16))) uint32_t s_pool[kPoolWords];
    uint32_t (*s_pl)[NP][64] = reinterpret_cast<uint32_t (*)[NP][64]>(s_pool);
    uint32_t *const s_lt = s_pool, *const s_gt = s_pool + 64;                  // per block: qc < min_depth, qc > max_depth
    uint8_t *const s_last = reinterpret_cast<uint8_t *>(s_pool + 128);         // kBlock bytes
    unsigned long long (*s_wtot)[12] = reinterpret_cast<unsigned long long (*)[12]>(s_pool + 128 + kBlock / 4);
    uint32_t *const s_wmax = s_pool + 128 + kBlock / 4 + kWaves * 24;
    // the low-MAPQ thresholds of depths below 255 as bytes: 255 = never (a count is at most the depth): a copy of a.lut8
    uint8_t *const s_lut = reinterpret_cast<uint8_t *>(s_pool + kLutPlane * 64);
    __shared__ uint32_t s_dbg[DEBUG ? NP : 1][64];         // DEBUG: the window's planes, for the dump of qc_depth
#ifdef CL_ROWS_LDS_PAD
    __shared__ uint32_t s_pad[CL_ROWS_LDS_PAD / 4];        // (occupancy experiments only)
    s_pad[threadIdx.x] = threadIdx.x;
#endif

    const uint32_t w = (blockIdx.x & 7u) * a.n_win8 + (blockIdx.x >> 3);   // XCD-contiguous window ranges
    if (w >= a.n_win) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t W = w * (uint32_t)T;
    // (the wave number from a scalar register: whatever is indexed or bounded by it below is scalar code)
    const uint32_t lane = tid & 63u, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t p0 = W + tid * PER;

    const WinMeta wm = a.win[w];
    const uint32_t lo = wm.lo, hi = wm.hi, wlo = wm.wlo, wn = wm.wn;
    const uint32_t n_cand = wn + (hi - lo);
    const uint32_t ng = wm.rn;                             // groups of 4 rows: the highest of the window's segments
    RowLane rl = row_lane(a.rows, wm, lane, wv);

    // requested first, needed last: the window's rows (this wave's first G groups), the reference bytes
    // (a lane gets the units its segment has, and zeros for the rest: row_lane)
    uint4 rv[G];
#pragma unroll
    for (int j = 0; j < G; ++j) rv[j] = row_unit(rl, kWaves * j);
    // ... and the window's first candidates: heads (above), U per lane and trip
    constexpr int U = 4;
    typedef typename HeadOf<HEAD4>::type Head;
    auto load_heads = [&](uint32_t base, Head (&hh)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t v = base + (uint32_t)u * kBlock + tid;
            uint32_t r = lo + (v - wn);
            if (v < wn) r = a.wide_idx[wlo + v];
            __builtin_assume(r < (1u << 29));
            hh[u] = Head();
            if (v < n_cand) hh[u] = head_at<HEAD4>(a.heads, r);
        }
    };
    Head hh[U];
    load_heads(0u, hh);
    // ... and wave 0's word of the byte thresholds, which it puts into LDS once it is done with the planes there
    uint32_t wlut = 0u;
    if (wv == 0) wlut = a.lut8[lane];
    // (bit p of refn: the reference base at p is 'N' / 'n' or lies beyond the reference, mod.rs:79-80, :100-101)
    const uint32_t refn = (uint32_t)reinterpret_cast<const uint16_t *>(a.refn)[(size_t)w * (T / 16) + tid];

    // ---- clear ----
    {
        const uint4 z = make_uint4(0, 0, 0, 0);
        uint4 *r4 = reinterpret_cast<uint4 *>(s_raw), *l4 = reinterpret_cast<uint4 *>(s_low);
        const uint4 zb = DEEP ? z : make_uint4(0x8000u, 0x8000u, 0x8000u, 0x8000u);
        for (int i = tid; i < kDiffWords / 4; i += kBlock) { r4[i] = zb; l4[i] = zb; }
    }
    __syncthreads();

    // ---- the window's rows: this wave's groups wv, wv + 2, ... into its counter planes.  The wave number is taken
    //      from a scalar register so that the tests on group numbers are scalar branches: a group slot past the window's
    //      highest segment costs nothing (the kernel is bound by vector issue), and the loads of a next trip are only
    //      issued when there is one (some segment with more than 12 groups: depth beyond 48) ----
    uint32_t c[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) c[p] = 0u;
    if (ng) {
        for (uint32_t g0 = wv; g0 < ng; g0 += (uint32_t)kWaves * G) {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if (g0 + (uint32_t)kWaves * j < ng) bs_add4<NP>(c, rv[j]);
            }
            if (g0 + (uint32_t)kWaves * G < ng) {          // a deeper window: the next trip's groups (requested only now)
                row_advance(rl, kWaves * G);
#pragma unroll
                for (int j = 0; j < G; ++j) rv[j] = row_unit(rl, kWaves * j);
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
                uint32_t ib, vb, ie, ve2;
                if (DEEP) { ib = cb; vb = 1u; ie = ce; ve2 = 0xFFFFFFFFu; }
                else {
                    ib = cb >> 1; vb = (cb & 1u) ? 0x10000u : 1u;
                    ie = ce >> 1; ve2 = (ce & 1u) ? 0xFFFF0000u : 0xFFFFFFFFu;
                }
                atomicAdd(&s_raw[ib], vb);
                if (ce < (uint32_t)T) atomicAdd(&s_raw[ie], ve2);
                if (hc.low) {
                    atomicAdd(&s_low[ib], vb);
                    if (ce < (uint32_t)T) atomicAdd(&s_low[ie], ve2);
                }
            }
        }
        base += (uint32_t)U * kBlock;
        if (base >= n_cand) break;
        load_heads(base, hh);
    }

    if (wv != 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) s_pl[wv - 1][p][lane] = c[p];
    }
    __syncthreads();

    // ---- final phase: depths, low-MAPQ rule, state, counts (16 positions per thread) ----
    {
        // wave 0: the waves' planes added (a bit-sliced ripple adder per wave) and compared with the two depth
        // thresholds (callable_profiler.rs:108-113); the other waves go on with their prefix sums meanwhile
        unsigned long long nbits = 0;                      // set bits of the window's rows, by wave 0's lanes (-> quality_bases)
        if (wv == 0) {
#pragma unroll
            for (int v = 1; v < kWaves; ++v) {
                uint32_t carry = 0u;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const uint32_t d = s_pl[v - 1][p][lane];
                    const uint32_t s = c[p] ^ d ^ carry;
                    carry = bs_maj(c[p], d, carry);
                    c[p] = s;
                }
            }
            // quality_bases (contig_profiler.rs:71): the sum of the block's 32 counts = sum over the planes of 2^p x set bits
#pragma unroll
            for (int p = 0; p < NP; ++p) nbits += (unsigned long long)__popc(c[p]) << p;
            s_lt[lane] = bs_less_than<NP>(c, (unsigned long long)a.min_depth);
            // qc > max_depth  <=>  !(qc < max_depth + 1); the rule is off for max_depth == 0
            s_gt[lane] = a.max_depth > 0u ? ~bs_less_than<NP>(c, (unsigned long long)a.max_depth + 1ull) : 0u;
            if (DEBUG) {
#pragma unroll
                for (int p = 0; p < NP; ++p) s_dbg[p][lane] = c[p];
            }
            // the thresholds of depths 4 lane .. 4 lane + 3, four bytes in the lane's own word (requested at the top)
            s_pool[kLutPlane * 64 + lane] = wlut;
        }
        uint32_t vr[PER], vl[PER];
        uint32_t sr = 0, sl = 0;
        if (DEEP) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                sr += s_raw[tid * PER + i]; vr[i] = sr;
                sl += s_low[tid * PER + i]; vl[i] = sl;
            }
        } else {
#pragma unroll
            for (int h = 0; h < PER / 2; ++h) {
                const uint32_t wr = s_raw[tid * (PER / 2) + h], wl = s_low[tid * (PER / 2) + h];
                sr += (wr & 0xFFFFu) - 0x8000u; vr[2 * h] = sr;
                sr += (uint32_t)((int32_t)wr >> 16); vr[2 * h + 1] = sr;
                sl += (wl & 0xFFFFu) - 0x8000u; vl[2 * h] = sl;
                sl += (uint32_t)((int32_t)wl >> 16); vl[2 * h + 1] = sl;
            }
        }
        // (a thread's sum of differences may be negative: two's complement in 32 bits, so the two scans stay separate)
        const uint32_t ir = dpp_incl_scan_u32(sr), il = dpp_incl_scan_u32(sl);
        // the wave's totals, for the waves behind it: in the first slot this lane has just consumed
        constexpr int kSlot = DEEP ? PER : PER / 2;
        if (lane == 63) { s_raw[tid * kSlot] = ir; s_low[tid * kSlot] = il; }
        __syncthreads();
        uint32_t offr = ir - sr, offl = il - sl;
        for (uint32_t i = 0; i < wv; ++i) { offr += s_raw[(i * 64u + 63u) * kSlot]; offl += s_low[(i * 64u + 63u) * kSlot]; }
        uint32_t mx = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) { vr[i] += offr; vl[i] += offl; mx = vr[i] > mx ? vr[i] : mx; }
        const uint32_t n_ok = p0 >= a.extent ? 0u : (a.extent - p0 < (uint32_t)PER ? a.extent - p0 : (uint32_t)PER);
        // From here on the thread's PER positions are PER bits of a register: bit i <-> position p0 + i.
        constexpr uint32_t FULL = 0xFFFFu;
        const uint32_t okb = n_ok >= (uint32_t)PER ? FULL : ((1u << n_ok) - 1u);            // positions < extent
        // qc_depth < min_depth, qc_depth > max_depth: PER consecutive bits of block (tid * PER) >> 5
        const uint32_t ltb = (s_lt[(tid * PER) >> 5] >> ((tid * PER) & 31u)) & FULL;
        const uint32_t gtb = (s_gt[(tid * PER) >> 5] >> ((tid * PER) & 31u)) & FULL;
        // raw_depth > 0, and the low-MAPQ rule (callable_profiler.rs:100-101): the two per-position tests
        uint32_t covb = 0, lowb = 0;
        if (!DEEP && mx < 255u) {
            // two instructions per test: a difference whose sign bit says "no" (raw - 1 wraps when raw == 0; low - lut
            // is negative when low < lut: all are below 2^31), shifted into the mask by v_alignbit ({mask, d} >> 31)
            uint32_t ncov = 0, nlow = 0;
#pragma unroll
            for (int i = PER - 1; i >= 0; --i) {
                const uint32_t raw = vr[i];
                ncov = __builtin_amdgcn_alignbit(ncov, raw - 1u, 31);
                nlow = __builtin_amdgcn_alignbit(nlow, vl[i] - (uint32_t)s_lut[raw], 31);
            }
            covb = ~ncov & FULL; lowb = ~nlow & FULL;
        } else {
            // The same two sign bits as above, so that no test's outcome waits in a pair of scalar registers for the
            // others: a threshold is clamped to 2^31 - 1 = never (a count is below 2^29), and so is that of a depth
            // below min_depth_for_low_mapq; lut[0] is "never" already (build_lut fills with 0xFFFFFFFF and starts at depth
            // 1).  A depth beyond the table takes the f64 divide (its load of the table's last entry is not used).
            const uint32_t mdl = a.min_depth_for_low_mapq < 0x7FFFFFFFu ? a.min_depth_for_low_mapq : 0x7FFFFFFFu;
            uint32_t ncov = 0, nlow = 0;
#pragma unroll
            for (int i = PER - 1; i >= 0; --i) {
                const uint32_t raw = vr[i], low = vl[i];
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
            }
            covb = ~ncov & FULL; lowb = ~nlow & FULL;
        }
        // priorities of callable_profiler.rs:104-116, resolved into disjoint masks:
        // REF_N > NO_COVERAGE > POOR_MAPPING_QUALITY > LOW_COVERAGE > EXCESSIVE_COVERAGE > CALLABLE
        const uint32_t Nk = refn & okb, notN = ~refn & okb, covk = covb & okb;
        const uint32_t t0 = notN & covk;
        const uint32_t rLow = t0 & lowb, t1 = t0 & ~lowb;
        const uint32_t rLT = t1 & ltb, t2 = t1 & ~ltb;
        const uint32_t rGT = t2 & gtb, rC = t2 & ~gtb;
        const uint32_t rNC = notN & ~covk;
        uint32_t cnt[6];
        cnt[0] = __popc(Nk); cnt[1] = __popc(rC); cnt[2] = __popc(rNC);
        cnt[3] = __popc(rLT); cnt[4] = __popc(rGT); cnt[5] = __popc(rLow);
        const uint32_t ncov = __popc(covk);
        // the state (types.rs:36-43: REF_N 0, CALLABLE 1, NO_COVERAGE 2, LOW_COVERAGE 3, EXCESSIVE_COVERAGE 4,
        // POOR_MAPPING_QUALITY 5) as three bit planes
        const uint32_t s0 = rC | rLT | rLow, s1 = rNC | rLT, s2 = rGT | rLow;
        auto state_at = [&](uint32_t j) -> uint32_t { return ((s0 >> j) & 1u) | (((s1 >> j) & 1u) << 1) | (((s2 >> j) & 1u) << 2); };
        if (DEBUG) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                uint32_t qc = 0;
                const uint32_t bit = ((tid * PER) & 31u) + (uint32_t)i;
#pragma unroll
                for (int p = 0; p < NP; ++p) qc |= ((s_dbg[p][(tid * PER) >> 5] >> bit) & 1u) << p;
                if (a.dbg_raw) a.dbg_raw[p0 + i] = vr[i];
                if (a.dbg_low) a.dbg_low[p0 + i] = vl[i];
                if (a.dbg_qc) a.dbg_qc[p0 + i] = qc;
                a.state[p0 + i] = (uint8_t)(((okb >> i) & 1u) ? state_at((uint32_t)i) : 0xFFu);
            }
        }
        // run boundaries strictly inside the window: position p (> W) whose state differs from p-1
        const uint32_t last_st = state_at((uint32_t)PER - 1u);
        s_last[tid] = (uint8_t)last_st;
        mx = dpp_wave_max_u32(mx);
        if (lane == 0) s_wmax[wv] = mx;
        __syncthreads();
        const uint32_t pv = tid > 0 ? (uint32_t)s_last[tid - 1] : state_at(0u);
        const uint32_t bnd = ((s0 ^ ((s0 << 1) | (pv & 1u))) | (s1 ^ ((s1 << 1) | ((pv >> 1) & 1u))) | (s2 ^ ((s2 << 1) | (pv >> 2)))) & okb;
        const uint32_t nb = __popc(bnd);
        if (!DEEP && NP == 8) {
            // a thread's counts are <= PER = 16 and every wave total <= 1024: packed words of two 11-bit fields, one
            // butterfly reduction each; the window's set bits (all with wave 0) are <= 255 x 2048 < 2^19
            constexpr int NW = 5;
            uint32_t pk[NW];
            pk[0] = cnt[0] | (cnt[1] << 11);
            pk[1] = cnt[2] | (cnt[3] << 11);
            pk[2] = cnt[4] | (cnt[5] << 11);
            pk[3] = ncov | (nb << 11);
            pk[4] = (uint32_t)nbits;
#pragma unroll
            for (int q = 0; q < NW; ++q) pk[q] = dpp_wave_sum_u32(pk[q]);
            if (lane == 0) {
                unsigned long long *t = s_wtot[wv];
                t[0] = pk[0] & 2047u; t[1] = pk[0] >> 11;
                t[2] = pk[1] & 2047u; t[3] = pk[1] >> 11;
                t[4] = pk[2] & 2047u; t[5] = pk[2] >> 11;
                t[6] = pk[3] & 2047u; t[9] = pk[3] >> 11;
                t[7] = pk[4];
                t[8] = 0;
                t[10] = 0; t[11] = 0;                    // (the reads' separable sums come from the host's walk)
            }
        } else {
            unsigned long long v[10];
#pragma unroll
            for (int q = 0; q < 6; ++q) v[q] = cnt[q];
            v[6] = ncov; v[7] = nbits; v[8] = 0; v[9] = nb;
#pragma unroll
            for (int q = 0; q < 10; ++q) {
                const unsigned long long r = wave_sum_u64(v[q]);
                if (lane == 0) s_wtot[wv][q] = r;
            }
            if (lane == 0) { s_wtot[wv][10] = 0; s_wtot[wv][11] = 0; }
        }
        __syncthreads();
        {
            const uint32_t inc = dpp_incl_scan_u32(nb);
            if (nb) {
                uint32_t off = inc - nb;
                for (uint32_t i = 0; i < wv; ++i) off += (uint32_t)s_wtot[i][9];
                uint16_t *dst = a.runs + (size_t)w * T + off;
                for (uint32_t m = bnd; m; m &= m - 1u) {     // (a lane has a boundary or two, rarely more)
                    const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
                    *dst++ = (uint16_t)((tid * PER + j) | (state_at(j) << 12));
                }
            }
            if (tid == 0) a.first_state[w] = (uint8_t)state_at(0u);
            if (tid == kBlock - 1) a.last_state[w] = (uint8_t)last_st;
        }
    }
    // the window's partial: twelve 8-byte words, one per lane -- word k < 9 is the waves' total k (cnt[6], n_cov, sum_qc,
    // sum_q), words 9 and 10 are totals 10 and 11 (sum_reflen, sum_mapq_reflen), word 11 is {n_inner = total 9, max_raw}
    static_assert(sizeof(WinPartial) == 96 && offsetof(WinPartial, sum_reflen) == 72 && offsetof(WinPartial, n_inner) == 88 &&
                  offsetof(WinPartial, max_raw) == 92, "WinPartial as twelve 8-byte words");
    if (tid < 12u) {
        const uint32_t q = tid < 9u ? tid : (tid == 11u ? 9u : tid + 1u);
        unsigned long long v = 0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) v += s_wtot[i][q];
        if (tid == 11u) {
            uint32_t m = 0;
#pragma unroll
            for (int i = 0; i < kWaves; ++i) m = s_wmax[i] > m ? s_wmax[i] : m;
            v = (unsigned long long)(uint32_t)v | ((unsigned long long)m << 32);
        }
        reinterpret_cast<unsigned long long *>(a.winpart + w)[tid] = v;
    }
}

} // namespace clk
