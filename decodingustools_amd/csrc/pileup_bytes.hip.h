// pileup_bytes.hip.h -- k_pileup, the byte forms of the pileup (DUT_QUAL_FORM=bytes), and everything only it uses.
//
// The quality bytes themselves are on the device and the kernel tests them there: short-read contigs as 16-byte RECORDS
// (ReadRec: a head per read and a piece per further M/=/X run), long-read contigs as a table of match pieces per window
// (the run table); the host builds both at upload, the kernel decodes no CIGAR in either form and none is uploaded.
// These are the forms of rounds 1-3.  The product runs k_pileup_rows (pileup_rows.hip.h); this kernel is kept as round 3
// left it -- its experiment hooks are gone, their results are in DESIGN.md section 5 and profiles/r02_*, r03_* -- so that
// bench.py's byte_form leg and the tests that run both forms stay reproducible.  It shares with k_pileup_rows what
// kernels.hip.h holds and nothing else.  (Since the tail is one launch it differs from round 3's by exactly what that
// needs of either pileup: ONE store of the window's packed word where the two state bytes were stored, and the copy of
// the summary's start values by the workgroup of window 0.)
#pragma once
#include "kernels.hip.h"
#include <type_traits>

namespace clk {

struct Opts {
    uint32_t min_depth;
    uint32_t max_depth;
    uint32_t min_mapq;
    uint32_t min_depth_for_low_mapq;
    uint32_t max_low_mapq;
    double   max_low_mapq_fraction;
    // byte-parallel "quality >= min_base_quality" constants (see pass_bytes)
    uint32_t ge_k, ge_c;
    // the same for "qc_depth >= min_depth" (md_all: min_depth > 255, every byte-sized count is below)
    // and "qc_depth >= max_depth + 1" (xd_on: max_depth in 1..254), used by the byte-parallel final phase
    uint32_t md_add, md_or, md_and, md_all;
    uint32_t xd_add, xd_or, xd_and, xd_on;
};

struct Reads {
    const int32_t  *pos;        // run-table form: the windows' candidates (+-1 span scatter, owner sums)
    const uint8_t  *mapq;
    const uint8_t  *qual;       // points kQualPad bytes into the allocation
    uint32_t n;
};

// The short-read form of k_pileup reads RECORDS, 16 bytes each, one aligned load; the host builds them at upload
// (callable_loci.hip: gen_read_recs) in read order, the records of a read side by side:
//   head record  {pos, span, qual_lo, mapq | 0x100 | seglen << 16}: the read as the pileup holds it, [pos, pos + span)
//                (span = bam_cigar2rlen: D and N included) -- the +-1 scatter and, in the window that holds pos, the
//                separable sums.  When the read's first M/=/X run starts at pos (the usual case) the head carries it too:
//                seglen bases whose quality bytes start at qual_lo; else seglen = 0.
//   piece record {pos of the run, 0, qual_lo, mapq | seglen << 16}: one further M/=/X run (or the next 65 535 bases of
//                a longer one), clipped to the bases that have a quality byte.
// qual_lo = the low 32 bits of the run's quality offset: a window's candidates lie within 2^32 bytes of its q0.
// A read without a reference span has no record at all.
struct __attribute__((aligned(16))) ReadRec {
    int32_t  pos;
    uint32_t span;
    uint32_t qual_lo;
    uint32_t meta;
};

// ---------------------------------------------------------------------------------------------
// byte-parallel ">= threshold" on four bytes at once, given the three constants of make_ge_consts()
// (callable_loci.hip) for a threshold T: 0x80 in each byte >= T.
//   T == 0        : always                    add = 0x80.., OR form
//   1 <= T <= 128 : hi(x) | (lo7(x) >= T)     add = 128 - T, OR form
//   T >= 129      : hi(x) & (lo7(x) >= T-128) add = 256 - T, AND form
// lo7 + add never carries out of its byte (both <= 127 / 128+127 < 256).  Used by the final phase for
// "qc_depth >= min_depth" / "> max_depth"; the quality threshold itself is pass_bytes() below.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t swar_ge7(uint32_t q, uint32_t add, uint32_t orm, uint32_t andm)
{
    const uint32_t d = (q & 0x7f7f7f7fu) + add;
    return ((d | (q & orm)) & (q | andm)) & 0x80808080u;
}

// What k_pileup takes (callable_loci.hip: bytes_args fills it, every member, in this order)
struct BytesArgs {
    Reads R;
    Opts o;
    const ReadRec *rec;           // the records of the short-read form (it reads these and nothing else per read)
    const uint32_t *end;          // per read, from the host (run-table form)
    const WinMeta *win;
    const uint32_t *wide_idx;           // read indices of the wide reads, ascending
    const uint8_t  *ref;          // padded with 'N' up to n_win*T
    const uint32_t *lut;          // kLutSize entries: smallest low count that is "too many"
    const uint2    *runtab;       // run-table form (LONG = 2): per window, the M/=/X pieces of its reads (host, at upload)
    uint8_t        *state;        // n_win*T bytes; written by the DEBUG instantiation only (test dumps)
    uint16_t       *runs;         // per window T entries: the run starts strictly inside the window, rel. position | state << 12
    uint32_t       *win_words;    // per window: n_inner | first state << 16 | last state << 24 (kernels.hip.h: win_word; run seams)
    WinPartial     *winpart;
    unsigned long long *summary;  // the contig summary as 16 words, and the start values of a run (callable_loci.hip: d_sum0):
    const unsigned long long *summary_start;   // the workgroup of window 0 copies them (kernels.hip.h: summary_start)
    uint32_t        extent;       // positions >= extent are not classified
    uint32_t        n_win;
    uint32_t        n_win8;       // ceil(n_win/8): XCD-contiguous window ranges
    // debug dumps (nullptr in production)
    uint32_t *dbg_raw, *dbg_qc, *dbg_low;
    uint32_t upl;                 // quality units per lane and trip in the consume loop: 2 for reads of up to ~128 bases, else 3
    uint8_t  *win_wide;           // per window: 1 = a position deeper than 255 was seen here, use 16-bit fields (sticky
                                  // for the resident contig; set by k_pileup itself, see mode8 below)
    uint32_t *err_flag;           // kNeedWide8 is raised here
};

// ---------------------------------------------------------------------------------------------
// k_pileup: one workgroup per window of T reference positions.
//
// Pass over the window's candidates (LONG = 0: the records of its reads, ReadRec; the wide reads' that start before
// the ordinary range first), 256 at a time, one lane per candidate, waves never synchronising:
//   * +1/-1 at the clipped span ends into raw / low-mapq difference arrays (mod.rs:22-28: every
//     read covering a position counts, D/N included)
//   * the lane writes the window-clipped M/=/X segment of its record (mapq >= min_mapq) into its wave's private
//     LDS list (in lane = position order); no CIGAR is decoded -- the host's walk at upload made the records
//   * lane quads consume the list: a lane handles units of 16 reference positions = one unaligned
//     16-byte load of quality bytes, a byte-parallel "quality >= min" test (mod.rs:30-37) and
//     adds into packed 8-bit (two sets) or 16-bit LDS counters (qc_depth); the sum of the passing
//     qualities feeds summed_baseq (contig_profiler.rs:68-70)
// then one barrier and a final phase per position: prefix sums -> raw_depth / low_mapq_count,
// the low-MAPQ rule and the state (callable_profiler.rs:100-116), the window's totals and its run
// list (the positions inside the window where the state changes).
// Neither the per-position counters nor the per-position states ever exist in HBM.
//
// Candidates are dealt to waves round-robin (candidate = base + 4*lane + wave): a wave's list holds every fourth
// read, and consecutive candidates alternate between the two 8-bit counter sets.
//
// LONG = 2 (the run-table form; what a contig with 8 or more CIGAR operations per read gets -- indel-rich ONT-like
// reads and HiFi-like long match runs alike; the operation-parallel form that decoded CIGARs on the device, LONG = 1 of
// rounds 1-3, lost to it on both and is gone): the host's walk over the CIGARs at upload leaves, per window, a flat
// table of the M/=/X pieces of its reads --
// 8 bytes each: {quality offset, window-relative start | end - 1 | counter set}, a piece never longer than two
// 16-position units, reads below min_mapq already dropped -- and the kernel streams its window's entries coalesced,
// one entry per lane, two entries and four quality loads in flight per lane.  The +-1 span scatter and the owner sums
// take pos / end / mapq of the window's candidates.
//
// DEEP = false: 8/16-bit counters and 16-bit differences; valid while the window has <= 32767 candidates
// (otherwise host_window_bounds raises kNeedDeep and the contig runs with DEEP = true: one
// 32-bit counter per position).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pass_bytes(uint32_t xw, uint32_t vm, const Opts &o)
{
    // 0x01 in every byte of xw that is a valid position (vm) and passes the threshold (mod.rs:33).  v_lerp_u8 is a
    // per-byte (x + k + (c & 1)) >> 1 with a 9-bit sum: with k = 256 - min_base_quality its bit 7 is the carry, i.e.
    // x >= min_base_quality, for every threshold 1..255 (0: k = 255 and the rounding bit make it always set) -- one
    // instruction where the masked add needs three (measured: 4.5 against 3 x 2.8 cycles per wave instruction)
    return (__builtin_amdgcn_lerp(xw, o.ge_k, o.ge_c) >> 7) & vm;
}

// 8-bit counters, two sets (reads alternate between the sets, a window handled this way is
// touched by <= 510 reads, so no byte exceeds 255): positions 8e..8e+7 are one 8-byte entry
// e = 2u + h of set `set`, stored at 2u + (h ^ ((u>>3)&1)); one ds_add_u64 covers 8 positions.
__device__ __forceinline__ uint32_t apply_unit8(const Q16 &v, const uint4 vm, uint32_t u, uint32_t set_off,
                                                unsigned long long *__restrict__ s_qc, const Opts &o)
{
    const uint32_t i0 = pass_bytes(v.w[0], vm.x, o), i1 = pass_bytes(v.w[1], vm.y, o);
    const uint32_t i2 = pass_bytes(v.w[2], vm.z, o), i3 = pass_bytes(v.w[3], vm.w, o);
    uint32_t sq = __builtin_amdgcn_udot4(v.w[0], i0, 0u, false);      // += quality of every passing byte
    sq = __builtin_amdgcn_udot4(v.w[1], i1, sq, false);
    sq = __builtin_amdgcn_udot4(v.w[2], i2, sq, false);
    sq = __builtin_amdgcn_udot4(v.w[3], i3, sq, false);
    const uint32_t e0 = set_off + ((u << 1) | ((u >> 3) & 1u));
    atomicAdd(&s_qc[e0], ((unsigned long long)i1 << 32) | i0);
    atomicAdd(&s_qc[e0 ^ 1u], ((unsigned long long)i3 << 32) | i2);
    return sq;
}

// 16-bit counters: positions 4e..4e+3 are one 8-byte entry e = 4u + jj, stored at
// 4u + (jj ^ ((u>>2)&3)) so that lanes holding the same jj spread over all banks.
__device__ __forceinline__ uint32_t apply_unit16(const Q16 &v, const uint4 vm, uint32_t u,
                                                 unsigned long long *__restrict__ s_qc, const Opts &o)
{
    uint32_t sq = 0;
    const uint32_t e0 = (u << 2) | ((u >> 2) & 3u);       // entry index for jj = 0, xor jj for the others
    const uint32_t vmw[4] = {vm.x, vm.y, vm.z, vm.w};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const uint32_t xw = v.w[jj];
        const uint32_t inc = pass_bytes(xw, vmw[jj], o);
        const uint32_t lo = __builtin_amdgcn_perm(0u, inc, 0x0c010c00u);   // bytes 0,1 -> 16-bit fields
        const uint32_t hi = __builtin_amdgcn_perm(0u, inc, 0x0c030c02u);   // bytes 2,3
        atomicAdd(&s_qc[e0 ^ (uint32_t)jj], ((unsigned long long)hi << 32) | lo);
        sq = __builtin_amdgcn_udot4(xw, inc, sq, false);
    }
    return sq;
}

__device__ __forceinline__ uint32_t apply_unit32(const Q16 &v, const uint4 vm, uint32_t u,
                                                 uint32_t *__restrict__ s_qc, const Opts &o)
{
    uint32_t sq = 0;
    const uint32_t vmw[4] = {vm.x, vm.y, vm.z, vm.w};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const uint32_t xw = v.w[jj];
        const uint32_t inc = pass_bytes(xw, vmw[jj], o);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if ((inc >> (8 * i)) & 1u) atomicAdd(&s_qc[(u << 4) + 4 * jj + i], 1u);
        sq = __builtin_amdgcn_udot4(xw, inc, sq, false);
    }
    return sq;
}

// a list entry {quality offset, srel | (len-1)<<16 | set<<30 | valid<<31} as a lane quad sees it
struct SegView {
    uint32_t srel, trel, qoff, u1, ub, set;
    bool on;
};
__device__ __forceinline__ SegView seg_view(uint2 d, uint32_t ql)
{
    SegView s;
    s.on = (d.y >> 31) != 0u;
    s.set = (d.y >> 30) & 1u;
    s.srel = d.y & 0xFFFFu;
    s.trel = s.srel + ((d.y >> 16) & 0x3FFFu) + 1u;
    s.qoff = d.x + (uint32_t)kQualPad - s.srel;      // + 16*u = byte offset of unit u from the padded base
    s.u1 = (s.trel - 1u) >> 4;
    s.ub = (s.srel >> 4) + ql;
    return s;
}

template <int T, bool DEBUG, bool DEEP, int LONG>
__global__ __launch_bounds__(kBlock, DEEP ? 4 : 8) void k_pileup(BytesArgs a)
{
    constexpr int PER = T / kBlock;                 // positions per thread in the final phase
    static_assert(PER == 8 || PER == 4, "T must be 2048 or 1024");
    constexpr int kWaves = kBlock / 64;
    static_assert(LONG == 0 || LONG == 2, "forms of k_pileup: 0 records (short reads), 2 run table (long reads)");
    constexpr int kListCap = LONG == 2 ? 1 : 64 + 16;   // entries of one wave's list: a pass's 64 + the < 16 carried over
    constexpr uint32_t kLutLds = 256;
    // +-1 differences of raw_depth / low_mapq_count.  DEEP: one 32-bit word per position.  Otherwise two
    // positions per word as 16-bit halves: the low half is biased by 0x8000 so that adding -1 (a
    // subtraction of 1 from the whole word) never borrows from the high half; exact while the window
    // is touched by < 32768 reads (host_window_bounds raises kNeedDeep beyond that).
    constexpr int kDiffWords = DEEP ? T : T / 2;
    __shared__ __attribute__((aligned(16))) uint32_t s_raw[kDiffWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_low[kDiffWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_qcw[DEEP ? T : T / 2];   // qc_depth counters
    __shared__ __attribute__((aligned(8))) uint2 s_list[kWaves][kListCap];
    __shared__ uint16_t s_lut[kLutLds];             // low-mapq threshold for raw < 256 (0xFFFF = never)
    // validity masks of a 16-position unit: byte i of s_mstart[vs] is 0x01 iff i >= vs,
    // byte i of s_mend[ve] is 0x01 iff i < ve (vs, ve in 0..16)
    __shared__ __attribute__((aligned(16))) uint4 s_mstart[17], s_mend[17];
    __shared__ uint32_t s_wraw[kWaves], s_wlow[kWaves], s_wmax[kWaves];
    __shared__ uint8_t s_last[kBlock];
    // per-wave totals: cnt[6], n_cov, sum_qc, sum_q, n_inner.  (Same-address LDS atomics are avoided:
    // hipcc turns them into a scalar loop over the active lanes.)
    __shared__ unsigned long long s_wtot[kWaves][12];          // [10], [11]: sums of the reads the window owns (LONG = 0)

    // XCD-aware window order: blocks b, b+8, b+16.. share an XCD (round-robin dispatch), give
    // each XCD one contiguous range of windows so neighbouring windows share its L2.
    const uint32_t w = (blockIdx.x & 7u) * a.n_win8 + (blockIdx.x >> 3);
    if (w >= a.n_win) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t W = w * (uint32_t)T;
    const uint32_t Wend = W + (uint32_t)T;
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    const uint32_t p0 = W + tid * PER;

    const WinMeta wm = a.win[w];
    const uint32_t lo = wm.lo, hi = wm.hi;
    // candidates: first the wn wide reads that start before read lo, then the reads [lo, hi)
    const uint32_t wlo = wm.wlo, wn = wm.wn;
    const uint32_t n_cand = wn + (hi - lo);
    // all quality bytes of the candidates lie within 2^32 of the first one's (checked by
    // host_window_bounds), so they are addressed by 32-bit offsets from a uniform base.  The base
    // sits kQualPad bytes low so that the offset of a unit start never goes negative.
    const unsigned long long qwin = wm.q0;
    const uint8_t *qbase = a.R.qual + qwin - kQualPad;

    // reference bytes of this thread's positions: needed last, requested first
    uint32_t refw[PER / 4];
#pragma unroll
    for (int i = 0; i < PER / 4; ++i) refw[i] = reinterpret_cast<const uint32_t *>(a.ref + p0)[i];

    // ---- clear ----
    {
        const uint4 z = make_uint4(0, 0, 0, 0);
        uint4 *r4 = reinterpret_cast<uint4 *>(s_raw), *l4 = reinterpret_cast<uint4 *>(s_low),
              *q4 = reinterpret_cast<uint4 *>(s_qcw);
        const uint4 zb = DEEP ? z : make_uint4(0x8000u, 0x8000u, 0x8000u, 0x8000u);
        for (int i = tid; i < kDiffWords / 4; i += kBlock) { r4[i] = zb; l4[i] = zb; }
        for (int i = tid; i < (DEEP ? T : T / 2) / 4; i += kBlock) q4[i] = z;
        if (tid < 34) {
            const uint32_t e = tid < 17 ? tid : tid - 17;                       // vs or ve
            const uint32_t bits = tid < 17 ? (0xFFFFu & ~((1u << e) - 1u)) : ((1u << e) - 1u);
            uint4 m;
            m.x = __umul24(bits & 15u, 0x204081u) & 0x01010101u;
            m.y = __umul24((bits >> 4) & 15u, 0x204081u) & 0x01010101u;
            m.z = __umul24((bits >> 8) & 15u, 0x204081u) & 0x01010101u;
            m.w = __umul24((bits >> 12) & 15u, 0x204081u) & 0x01010101u;
            if (tid < 17) s_mstart[e] = m; else s_mend[e] = m;
        }
        if (tid < kLutLds) {
            // fold "raw >= min_depth_for_low_mapq" into the table: below it the rule never fires
            const uint32_t v = (tid >= a.o.min_depth_for_low_mapq && tid > 0) ? a.lut[tid] : 0xFFFFFFFFu;
            s_lut[tid] = v > 0xFFFFu ? (uint16_t)0xFFFFu : (uint16_t)v;
        }
    }
    __syncthreads();

    // qc_depth counters: two sets of bytes when the window is touched by <= 510 reads (the reads
    // alternate between the sets, so no byte can pass 255), else 16-bit fields (DEEP: 32-bit words)
    // The bytes cannot overflow with <= 510 candidates.  With more (deeper data: 36x of 150-base reads
    // already has ~515 candidates per window) they still cannot while no position is covered by more than
    // 255 reads -- a byte counts reads of one set covering its position -- so the 8-bit sets are used
    // optimistically and the window's maximum raw depth, known in the final phase, is the check: beyond
    // 255 the kernel marks the window in win_wide, raises kNeedWide8, and the host runs the contig again:
    // marked windows then use the 16-bit fields.
    // (LONG = 2: the counter set of a piece is its read's parity in the contig, not in the window's candidate list, so the
    // candidate count bounds nothing and the maximum raw depth is the check for every window.)
    constexpr bool kByDepth = LONG == 2;
    const bool mode8 = !DEEP && ((!kByDepth && n_cand <= 510u) || a.win_wide[w] == 0);

    // ---- the pass over the reads ----
    uint32_t sq32 = 0;                              // sum of passing qualities handled by this lane
    unsigned long long sumq = 0;
    const uint32_t ql = lane & 3u, quad = lane >> 2;
    uint2 *list = s_list[wv];
    uint32_t n_keep = 0;                            // list entries carried over from the previous round (< 16)
    unsigned long long win_len = 0, win_mq = 0;     // wave-uniform sums over the reads this window owns
    // quads consume list entries [0, n_use), Q = n_use/16 (rounded up) entries each.  Three units per lane and
    // trip: u, u+4, u+8; a unit past the end is clamped onto the last one and gets an empty mask.
    // MODE 0: 8-bit two-set counters, 1: 16-bit fields, 2: 32-bit words (DEEP)
    // UPL units per lane and trip: 3 (12 unit slots per quad: fits a 150-base read) or 2 (8 slots: reads of
    // up to ~128 bases would leave a third of the 12 empty)
    auto consume = [&](auto mode_tag, auto upl_tag, uint32_t n_use) {
        constexpr int MODE = decltype(mode_tag)::value;
        constexpr int UPL = decltype(upl_tag)::value;
        const uint32_t Q = (n_use + 15u) >> 4;
        for (uint32_t i = 0; i < Q; ++i) {
            // quad q takes entries q, q + 16, ...: the 16 quads of a trip work on 16 neighbouring segments, so the
            // 128-byte line that holds the end of one read's qualities and the start of the next is touched by two
            // quads of the same trip instead of microseconds apart (measured: 1 714 instead of 1 798 MB fetched per
            // launch, time equal within the run-to-run spread, against quad q taking entries q*Q .. q*Q+Q-1)
            const uint32_t idx = i * 16u + quad;
            uint2 d = make_uint2(0u, 0u);
            if (idx < n_use) d = list[idx];
            const SegView sv = seg_view(d, ql);
            for (uint32_t u = sv.ub; u <= sv.u1; u += 4u * UPL) {
                Q16 v[UPL];
                uint32_t uu[UPL];
#pragma unroll
                for (int j = 0; j < UPL; ++j) {
                    const uint32_t un = u + 4u * j;
                    uu[j] = un < sv.u1 ? un : sv.u1;
                    __builtin_memcpy(&v[j], qbase + (sv.qoff + (uu[j] << 4)), 16);
                }
#pragma unroll
                for (int j = 0; j < UPL; ++j) {
                    const uint32_t ps = uu[j] << 4;
                    const uint32_t vs = sv.srel > ps ? sv.srel - ps : 0u;
                    uint32_t ve = (sv.trel - ps) < 16u ? (sv.trel - ps) : 16u;
                    ve = (sv.on && u + 4u * j <= sv.u1) ? ve : 0u;
                    const uint4 ms = s_mstart[vs], me = s_mend[ve];
                    const uint4 vm = make_uint4(ms.x & me.x, ms.y & me.y, ms.z & me.z, ms.w & me.w);
                    // a slot past the segment's end adds zeros: to the word of its own unit number, not (with the lanes
                    // beside it) to the word of the segment's last unit
                    const uint32_t un = u + 4u * j, ua = un < (uint32_t)(T / 16) ? un : (uint32_t)(T / 16) - 1u;
                    if (MODE == 2) sq32 += apply_unit32(v[j], vm, uu[j], s_qcw, a.o);
                    else if (MODE == 0) sq32 += apply_unit8(v[j], vm, ua, sv.set * (uint32_t)(T / 8), reinterpret_cast<unsigned long long *>(s_qcw), a.o);
                    else sq32 += apply_unit16(v[j], vm, uu[j], reinterpret_cast<unsigned long long *>(s_qcw), a.o);
                }
            }
        }
    };
    auto consume_list = [&](uint32_t n_use) {
        using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
        if (DEEP) consume(std::integral_constant<int, 2>{}, I3{}, n_use);
        else if (mode8) { if (a.upl == 2u) consume(std::integral_constant<int, 0>{}, I2{}, n_use); else consume(std::integral_constant<int, 0>{}, I3{}, n_use); }
        else consume(std::integral_constant<int, 1>{}, I3{}, n_use);
    };
    if constexpr (LONG == 2) {
        // ---- run-table form.  (1) the window's candidates: +-1 at the clipped span ends, and the separable sums of the
        //      reads that start here (contig_profiler.rs:74) ----
        for (uint32_t base = 0; base < n_cand; base += kBlock) {
            const uint32_t v = base + tid;
            unsigned long long own_len = 0, own_mq = 0;
            if (v < n_cand) {
                const uint32_t r = v < wn ? a.wide_idx[wlo + v] : lo + (v - wn);
                const uint32_t x = (uint32_t)a.R.pos[r], e = a.end[r], mq = a.R.mapq[r];
                if (x >= W) {                                    // the window that holds the read's start owns its sums
                    own_len = e - x;
                    own_mq = mq >= a.o.min_mapq ? (unsigned long long)mq * (e - x) : 0ull;
                }
                if (e > W) {
                    const uint32_t cb = x > W ? x - W : 0u, ce = e - W;
                    uint32_t ib, vb, ie, ve2;
                    if (DEEP) { ib = cb; vb = 1u; ie = ce; ve2 = 0xFFFFFFFFu; }
                    else {
                        ib = cb >> 1; vb = (cb & 1u) ? 0x10000u : 1u;
                        ie = ce >> 1; ve2 = (ce & 1u) ? 0xFFFF0000u : 0xFFFFFFFFu;
                    }
                    atomicAdd(&s_raw[ib], vb);
                    if (ce < (uint32_t)T) atomicAdd(&s_raw[ie], ve2);
                    if (mq <= a.o.max_low_mapq) {
                        atomicAdd(&s_low[ib], vb);
                        if (ce < (uint32_t)T) atomicAdd(&s_low[ie], ve2);
                    }
                }
            }
            win_len += wave_sum_u64(own_len); win_mq += wave_sum_u64(own_mq);
        }
        // ---- (2) the window's pieces, streamed: entry {x, y}: x + 16 u = byte offset of unit u's qualities from qbase;
        //      y = start (11 bits) | end - 1 (11) | - | counter set (bit 29) | - | valid (bit 31).  A piece covers the
        //      unit of its start and at most the next one.  Lane t takes entries t, t + 256, ...: a wave's 64 entries are
        //      consecutive pieces of (mostly) one read, their quality bytes ~1 KB of one stretch of memory. ----
        {
            constexpr int E = 2;                                 // entries per lane and trip: 2 E quality loads in flight
            const uint2 *ent = a.runtab + wm.rlo;
            const uint32_t nent = wm.rn;
            // (every load of the loop is unconditional -- an index past the end is clamped and its entry marked invalid --:
            // behind a load in a conditional block hipcc waits for vmcnt(0).  A clamped lane keeps the last entry's start
            // and end and only loses the valid bit: its two quality loads then go where that entry's go.  With the
            // whole word cleared they went to unit 0 of the window, up to 2 047 bytes in front of the entry's bytes -- in
            // front of the quality array itself when the window's last piece belongs to the contig's first read.)
            auto fetch = [&](uint32_t b, uint2 (&d)[E]) {
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    const uint32_t idx = b + (uint32_t)j * kBlock + tid;
                    const bool in = idx < nent;
                    d[j] = ent[in ? idx : nent - 1u];
                    d[j].y = in ? d[j].y : (d[j].y & 0x7FFFFFFFu);
                }
            };
            uint2 d[E], dn[E];
            if (nent) fetch(0u, d);
            for (uint32_t b = 0; b < nent; b += kBlock * E) {     // block-uniform
                fetch(b + kBlock * E, dn);                        // the next trip's entries are requested first
                Q16 v[E][2];
                uint32_t u0[E], two[E];
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    u0[j] = (d[j].y & 2047u) >> 4;
                    two[j] = (((d[j].y >> 11) & 2047u) >> 4) - u0[j];          // 0 or 1
                    __builtin_memcpy(&v[j][0], qbase + (d[j].x + (u0[j] << 4)), 16);
                    __builtin_memcpy(&v[j][1], qbase + (d[j].x + ((u0[j] + two[j]) << 4)), 16);
                }
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    const uint32_t srel = d[j].y & 2047u, trel = ((d[j].y >> 11) & 2047u) + 1u;
                    const uint32_t set_off = ((d[j].y >> 29) & 1u) * (uint32_t)(T / 8);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        if ((d[j].y >> 31) && (h == 0 || two[j])) {
                            const uint32_t u = u0[j] + (uint32_t)h, ps = u << 4;
                            const uint32_t vs = srel > ps ? srel - ps : 0u;
                            const uint32_t ve = (trel - ps) < 16u ? (trel - ps) : 16u;
                            const uint4 ms = s_mstart[vs], me = s_mend[ve];
                            const uint4 vm = make_uint4(ms.x & me.x, ms.y & me.y, ms.z & me.z, ms.w & me.w);
                            if (DEEP) sq32 += apply_unit32(v[j][h], vm, u, s_qcw, a.o);
                            else if (mode8) sq32 += apply_unit8(v[j][h], vm, u, set_off, reinterpret_cast<unsigned long long *>(s_qcw), a.o);
                            else sq32 += apply_unit16(v[j][h], vm, u, reinterpret_cast<unsigned long long *>(s_qcw), a.o);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < E; ++j) d[j] = dn[j];
                sumq += sq32; sq32 = 0;
            }
        }
    } else if constexpr (LONG == 0) {
        // ---- short-read form: the candidates are RECORDS (ReadRec), 256 at a time, one lane per record, the records
        //      dealt round-robin to the 4 waves; waves never synchronise during the pass.  No CIGAR is decoded on the device:
        //      the host's walk at upload turned every read into a head record (its span: the +-1 scatter, mod.rs:22-28, and
        //      the sums of the window that holds its start, contig_profiler.rs:74) that also carries the read's first
        //      M/=/X run when that starts at the read's position -- all there is to 96 reads in 100 of aligner output --
        //      and one piece record per further run (mod.rs:30-37 visits exactly those bases). ----
        for (uint32_t base = 0; base < n_cand; base += kBlock) {
            const uint32_t v = base + 4u * lane + wv;   // candidate number; consecutive candidates alternate counter sets
            uint32_t r = lo + (v - wn);
            if (v < wn) r = a.wide_idx[wlo + v];
            __builtin_assume(r < (1u << 29));           // the host refuses contigs with >= 2^29 records
            uint2 seg = make_uint2(0u, 0u);
            uint32_t own_l = 0, own_m = 0;              // spans below 2^16: the wave's sums fit 32 bits
            bool big = false;                           // a head record with a wider span (rare: exact 64-bit sums below)
            uint32_t big_span = 0, big_mq = 0;
            if (v < n_cand) {
                uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
                // (one 16-byte load: left alone, hipcc splits it and fetches fields behind the tests that need them)
                asm volatile("" : "+v"(rr.x), "+v"(rr.y), "+v"(rr.z), "+v"(rr.w));
                const uint32_t x = rr.x, span = rr.y, mq = rr.w & 255u, seglen = rr.w >> 16;
                const bool hq = mq >= a.o.min_mapq;
                if ((rr.w & 0x100u) && span) {                   // head record: the read as the pileup holds it, [x, x + span)
                    const uint32_t e = x + span;
                    if (x >= W) {                                // every read starts in exactly one window
                        if (span < 0x10000u) { own_l = span; own_m = hq ? mq * span : 0u; }
                        else { big = true; big_span = span; big_mq = hq ? mq : 0u; }
                    }
                    if (e > W) {
                        const uint32_t cb = x > W ? x - W : 0u, ce = e - W;
                        uint32_t ib, vb, ie, ve2;            // word index and addend of the +1 and of the -1
                        if (DEEP) { ib = cb; vb = 1u; ie = ce; ve2 = 0xFFFFFFFFu; }
                        else {
                            ib = cb >> 1; vb = (cb & 1u) ? 0x10000u : 1u;
                            ie = ce >> 1; ve2 = (ce & 1u) ? 0xFFFF0000u : 0xFFFFFFFFu;
                        }
                        atomicAdd(&s_raw[ib], vb);
                        if (ce < (uint32_t)T) atomicAdd(&s_raw[ie], ve2);
                        if (mq <= a.o.max_low_mapq) {
                            atomicAdd(&s_low[ib], vb);
                            if (ce < (uint32_t)T) atomicAdd(&s_low[ie], ve2);
                        }
                    }
                }
                // the record's run of seglen bases with a quality byte each, from reference position x
                const uint32_t sp = x > W ? x : W, te = x + seglen, tp = te < Wend ? te : Wend;
                if (hq && seglen && sp < tp)
                    seg = make_uint2(rr.z - (uint32_t)qwin + (sp - x), (sp - W) | ((tp - sp - 1u) << 16) | ((v & 1u) << 30) | 0x80000000u);
            }
            win_len += dpp_wave_sum_u32(own_l); win_mq += dpp_wave_sum_u32(own_m);
            if (__any(big)) {
                win_len += wave_sum_u64(big ? (unsigned long long)big_span : 0ull);
                win_mq += wave_sum_u64(big ? (unsigned long long)big_mq * big_span : 0ull);
            }
            // -- wave-private list in lane (= position) order: carried-over entries, then this pass's --
            uint32_t n_list = n_keep;
            {
                const bool has = (seg.y >> 31) != 0u;
                const unsigned long long m = __ballot(has);
                if (has) {
                    const uint32_t idx = n_list + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    list[idx] = seg;
                }
                n_list += (uint32_t)__popcll(m);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // -- only full groups of 16 entries are consumed now; the < 16 left over move to the front
            //    of the list and wait for the next pass (or for the flush after the last one) --
            const uint32_t n_full = n_list & ~15u;
            if (n_full) consume_list(n_full);
            n_keep = n_list - n_full;
            uint2 carry = make_uint2(0u, 0u);
            if (n_full && lane < n_keep) carry = list[n_full + lane];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();       // the list is rewritten below and in the next pass
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (n_full && lane < n_keep) list[lane] = carry;
            sumq += sq32; sq32 = 0;
        }
    }
    if (n_keep) {                                   // flush what the last round left over
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        consume_list(n_keep);
        sumq += sq32; sq32 = 0;
    }
    __syncthreads();

    // ---- final phase: depths, low-MAPQ rule, state, counts (8 positions per thread) ----
    uint32_t first_st = 0;
    {
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
                // low half: biased by 0x8000; high half: two's complement 16-bit
                sr += (wr & 0xFFFFu) - 0x8000u; vr[2 * h] = sr;
                sr += (uint32_t)((int32_t)wr >> 16); vr[2 * h + 1] = sr;
                sl += (wl & 0xFFFFu) - 0x8000u; vl[2 * h] = sl;
                sl += (uint32_t)((int32_t)wl >> 16); vl[2 * h + 1] = sl;
            }
        }
        const uint32_t ir = dpp_incl_scan_u32(sr), il = dpp_incl_scan_u32(sl);
        if (lane == 63) { s_wraw[wv] = ir; s_wlow[wv] = il; }
        // 8-bit mode: the thread's PER positions are PER consecutive bytes of entry 2u+h (8 positions
        // each) of the two counter sets
        uint32_t qc8a[PER / 4], qc8b[PER / 4];
#pragma unroll
        for (int h = 0; h < PER / 4; ++h) { qc8a[h] = 0; qc8b[h] = 0; }
        if (!DEEP && mode8) {
            const uint32_t ent = (tid * PER) >> 3, u = ent >> 1;
            const uint32_t e = (u << 1) | ((ent & 1u) ^ ((u >> 3) & 1u));
#pragma unroll
            for (int h = 0; h < PER / 4; ++h) {
                const uint32_t wsel = PER == 8 ? (uint32_t)h : (tid & 1u);          // which half of the entry
                qc8a[h] = s_qcw[2u * e + wsel];
                qc8b[h] = s_qcw[2u * (T / 8 + e) + wsel];
            }
        }
        __syncthreads();
        uint32_t offr = ir - sr, offl = il - sl;
        for (uint32_t i = 0; i < wv; ++i) { offr += s_wraw[i]; offl += s_wlow[i]; }
        uint32_t mx = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) { vr[i] += offr; vl[i] += offl; mx = vr[i] > mx ? vr[i] : mx; }
        const uint32_t n_ok = p0 >= a.extent ? 0u : (a.extent - p0 < (uint32_t)PER ? a.extent - p0 : (uint32_t)PER);

        uint32_t S[PER / 4];                        // state bytes of the thread's positions
        uint32_t cnt[6] = {0, 0, 0, 0, 0, 0}, ncov = 0;
        unsigned long long sqc = 0;
        if (!DEEP && mode8 && mx < kLutLds && n_ok == (uint32_t)PER) {
            // ---- byte-parallel path: every column is shallower than 256, so qc_depth (<= raw_depth)
            //      fits a byte and four positions are classified per 32-bit word ----
            const uint32_t ONES = 0x01010101u;
#pragma unroll
            for (int h = 0; h < PER / 4; ++h) {
                const uint32_t q4 = qc8a[h] + qc8b[h];                       // no byte can carry
                uint32_t cov = 0, low = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t raw = vr[4 * h + i];
                    cov |= (raw < 1u ? raw : 1u) << (8 * i);
                    // low-MAPQ rule through the table (callable_profiler.rs:100-101)
                    low |= (vl[4 * h + i] >= (uint32_t)s_lut[raw] ? 1u : 0u) << (8 * i);
                }
                const uint32_t x = (refw[h] | 0x20202020u) ^ 0x6e6e6e6eu;   // zero byte <=> 'N' or 'n'
                const uint32_t nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7;
                const uint32_t N = ~nz & ONES;
                uint32_t lt = ONES;                                          // qc < min_depth
                if (!a.o.md_all) lt = ~(swar_ge7(q4, a.o.md_add, a.o.md_or, a.o.md_and) >> 7) & ONES;
                uint32_t gt = 0;                                             // qc > max_depth (max_depth in 1..254)
                if (a.o.xd_on) gt = swar_ge7(q4, a.o.xd_add, a.o.xd_or, a.o.xd_and) >> 7;
                // priorities of callable_profiler.rs:104-116, resolved into disjoint flags
                const uint32_t t0 = ~N & cov;
                const uint32_t rLow = t0 & low, t1 = t0 & ~low;
                const uint32_t rLT = t1 & lt, t2 = t1 & ~lt;
                const uint32_t rGT = t2 & gt, rC = t2 & ~gt;
                const uint32_t rNC = ~N & ~cov & ONES;
                S[h] = rC + (rNC << 1) + rLT + (rLT << 1) + (rGT << 2) + rLow + (rLow << 2);
                cnt[0] += __popc(N); cnt[1] += __popc(rC); cnt[2] += __popc(rNC);
                cnt[3] += __popc(rLT); cnt[4] += __popc(rGT); cnt[5] += __popc(rLow);
                ncov += __popc(cov);
                sqc += __builtin_amdgcn_udot4(q4, ONES, 0u, false);
                if (DEBUG) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (a.dbg_raw) a.dbg_raw[p0 + 4 * h + i] = vr[4 * h + i];
                        if (a.dbg_low) a.dbg_low[p0 + 4 * h + i] = vl[4 * h + i];
                        if (a.dbg_qc) a.dbg_qc[p0 + 4 * h + i] = (q4 >> (8 * i)) & 0xFFu;
                    }
                }
            }
        } else {
            // ---- general path, one position at a time ----
            uint32_t qc[PER];
            if (DEEP) {
#pragma unroll
                for (int i = 0; i < PER; ++i) qc[i] = s_qcw[tid * PER + i];
            } else if (mode8) {
#pragma unroll
                for (int i = 0; i < PER; ++i)
                    qc[i] = ((qc8a[i >> 2] >> (8 * (i & 3))) & 0xFFu) + ((qc8b[i >> 2] >> (8 * (i & 3))) & 0xFFu);
            } else {
                const uint2 *q2 = reinterpret_cast<const uint2 *>(s_qcw);
#pragma unroll
                for (int h = 0; h < PER / 4; ++h) {
                    const uint32_t e = tid * (PER / 4) + h;                 // entry 4u+jj: u = e>>2, jj = e&3
                    const uint2 c = q2[(e & ~3u) | ((e & 3u) ^ ((e >> 4) & 3u))];
                    qc[4 * h + 0] = c.x & 0xFFFFu; qc[4 * h + 1] = c.x >> 16;
                    qc[4 * h + 2] = c.y & 0xFFFFu; qc[4 * h + 3] = c.y >> 16;
                }
            }
            uint32_t st[PER];
            for (int i = 0; i < PER; ++i) {
                const uint32_t raw = vr[i], low = vl[i];
                bool is_low = false;                                                  // callable_profiler.rs:100-101
                if (raw >= a.o.min_depth_for_low_mapq && raw > 0) {
                    if (raw < kLutSize) is_low = low >= a.lut[raw];
                    else is_low = ((double)low / (double)raw) > a.o.max_low_mapq_fraction;   // IEEE f64 divide
                }
                const uint32_t rb = (refw[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                uint32_t sx = 1u;                                                     // CALLABLE
                sx = (a.o.max_depth > 0 && qc[i] > a.o.max_depth) ? 4u : sx;          // EXCESSIVE_COVERAGE
                sx = qc[i] < a.o.min_depth ? 3u : sx;                                 // LOW_COVERAGE
                sx = is_low ? 5u : sx;                                                // POOR_MAPPING_QUALITY
                sx = raw == 0 ? 2u : sx;                                              // NO_COVERAGE
                sx = ((rb | 0x20u) == 'n') ? 0u : sx;                                 // REF_N
                const bool ok = (uint32_t)i < n_ok;
                if (ok) { cnt[sx] += 1; ncov += raw > 0 ? 1u : 0u; sqc += qc[i]; }
                st[i] = ok ? sx : 0xFFu;
                if (DEBUG) {
                    if (a.dbg_raw) a.dbg_raw[p0 + i] = raw;
                    if (a.dbg_low) a.dbg_low[p0 + i] = low;
                    if (a.dbg_qc) a.dbg_qc[p0 + i] = qc[i];
                }
            }
#pragma unroll
            for (int h = 0; h < PER / 4; ++h)
                S[h] = st[4 * h] | (st[4 * h + 1] << 8) | (st[4 * h + 2] << 16) | (st[4 * h + 3] << 24);
        }
        // run boundaries strictly inside the window: position p (> W) whose state differs from p-1
        s_last[tid] = (uint8_t)(S[PER / 4 - 1] >> 24);
        mx = dpp_wave_max_u32(mx);
        if (lane == 0) s_wmax[wv] = mx;
        __syncthreads();
        uint32_t nb = 0;
        uint32_t bmk[PER / 4];                                               // 0x01 in the bytes that start a run
        {
            uint32_t prevb = tid > 0 ? (uint32_t)s_last[tid - 1] : (S[0] & 0xFFu);
            const uint4 okm = s_mend[n_ok];                                  // 0x01 for the positions < extent
            const uint32_t okw[2] = {okm.x, okm.y};
#pragma unroll
            for (int h = 0; h < PER / 4; ++h) {
                const uint32_t P = (S[h] << 8) | prevb;
                const uint32_t d = S[h] ^ P;
                bmk[h] = ((((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) >> 7) & okw[h];
                nb += __popc(bmk[h]);
                prevb = S[h] >> 24;
            }
        }
        if (DEBUG) {
#pragma unroll
            for (int h = 0; h < PER / 4; ++h) reinterpret_cast<uint32_t *>(a.state + p0)[h] = S[h];
        }
        if (mode8) {
            // <= 510 reads: a thread's counts are <= 8 and every wave total fits 10 bits (sum_qc 17,
            // sum_q 29): five packed words, one butterfly reduction each
            uint32_t pk[5];
            pk[0] = cnt[0] | (cnt[1] << 10) | (cnt[2] << 20);
            pk[1] = cnt[3] | (cnt[4] << 10) | (cnt[5] << 20);
            pk[2] = ncov | (nb << 10);
            pk[3] = (uint32_t)sqc;
            pk[4] = (uint32_t)sumq;
#pragma unroll
            for (int c = 0; c < 5; ++c) pk[c] = dpp_wave_sum_u32(pk[c]);
            if (lane == 0) {
                unsigned long long *t = s_wtot[wv];
                t[0] = pk[0] & 1023u; t[1] = (pk[0] >> 10) & 1023u; t[2] = pk[0] >> 20;
                t[3] = pk[1] & 1023u; t[4] = (pk[1] >> 10) & 1023u; t[5] = pk[1] >> 20;
                t[6] = pk[2] & 1023u; t[9] = pk[2] >> 10;
                t[7] = pk[3]; t[8] = pk[4];
                t[10] = win_len; t[11] = win_mq;
            }
        } else {
            // denser windows: totals may pass 2^32
            unsigned long long v[10];
#pragma unroll
            for (int c = 0; c < 6; ++c) v[c] = cnt[c];
            v[6] = ncov; v[7] = sqc; v[8] = sumq; v[9] = nb;
#pragma unroll
            for (int c = 0; c < 10; ++c) {
                const unsigned long long r = wave_sum_u64(v[c]);
                if (lane == 0) s_wtot[wv][c] = r;
            }
            if (lane == 0) { s_wtot[wv][10] = win_len; s_wtot[wv][11] = win_mq; }
        }
        __syncthreads();
        // the window's run list: every run start strictly inside the window, in position order
        // (k_tail turns the lists into intervals; the per-position states never reach HBM)
        {
            const uint32_t inc = dpp_incl_scan_u32(nb);
            if (nb) {
                uint32_t off = inc - nb;
                for (uint32_t i = 0; i < wv; ++i) off += (uint32_t)s_wtot[i][9];
                uint16_t *dst = a.runs + (size_t)w * T + off;
#pragma unroll
                for (int h = 0; h < PER / 4; ++h)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((bmk[h] >> (8 * j)) & 1u) *dst++ = (uint16_t)((tid * PER + 4 * h + j) | (((S[h] >> (8 * j)) & 7u) << 12));
            }
            first_st = S[0] & 0xFFu;                                             // (thread 0's is the window's)
        }
    }
    if (tid == 0) {
        WinPartial wp;
        unsigned long long tot[12];
        for (int c = 0; c < 12; ++c) { tot[c] = 0; for (int i = 0; i < kWaves; ++i) tot[c] += s_wtot[i][c]; }
        for (int c = 0; c < 6; ++c) wp.cnt[c] = tot[c];
        wp.n_cov = tot[6]; wp.sum_qc = tot[7]; wp.sum_q = tot[8];
        wp.sum_reflen = tot[10]; wp.sum_mapq_reflen = tot[11];
        wp.n_inner = (uint32_t)tot[9];
        uint32_t m = 0;
        for (int i = 0; i < kWaves; ++i) m = s_wmax[i] > m ? s_wmax[i] : m;
        wp.max_raw = m;
        a.winpart[w] = wp;
        // the window's packed word for the tail (s_last: every thread's last state, written before the barriers above)
        a.win_words[w] = win_word(wp.n_inner, first_st, (uint32_t)s_last[kBlock - 1]);
        if (!DEEP && mode8 && (kByDepth || n_cand > 510u) && m > 255u) { a.win_wide[w] = 1; atomicOr(a.err_flag, kNeedWide8); }
    }
    if (w == 0u) summary_start(a.summary, a.summary_start, tid);
}

} // namespace clk
