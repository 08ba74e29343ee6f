// site_scan.hip.h -- the dense form of the site pileup (config 5): base counts and SNV calls at EVERY position of a
// range of the resident site tile (cl_site_upload), instead of at the sites of a list.
//
// k_site_pileup (site_engine.hip.h) is built for a sparse list: one thread per read, a read leaves at once when no site
// lies in its span, 64 sites per workgroup in LDS.  With a site at every base none of that helps, and the histogram
// (64 bytes per position) has to cross HBM and the link.  Here a workgroup owns a window of kScanWin reference positions:
// it counts the bases of every read over the window in LDS, applies the calling rule of caller.rs:132-149 there and
// writes back only the positions that differ from the reference (or, in the dense mode, the counters per position).
//
// Per position the semantics are those of k_site_pileup, condition by condition (hist[p][c] of cl_site_run for the
// 1-based site p + 1): read start < contig_len, mapq >= min_quality, bases of M/=/X operations, query index < l_seq,
// p < ref_len.  The unfiltered form has no flag or base-quality filter.
//
// The kernels:
//   k_site_scan_index   once per resident tile: the reference end of every read and, per window, the index range
//                       [first, last) of the reads that overlap it (atomicMin / atomicMax of the read's index over
//                       the windows of its span).  The range holds every overlapping read whatever the order of the
//                       tile, so an unsorted tile gives exact counts too -- its ranges are merely wider.
//   k_site_scan<FILTERED, MODE>
//                       one workgroup per window: reads of the window's range are dealt to the threads, a thread walks
//                       its read's CIGAR over the window and adds into LDS counter planes (one ds_add without return
//                       per base, consecutive positions in consecutive banks).  What happens to the finished planes is
//                       the MODE: the counters themselves go out (SCAN_DENSE), or every thread judges positions and the
//                       candidates are compacted with one ballot and one atomic per wave -- by the calling rule
//                       (SCAN_CALLS), the second-allele rule (SCAN_MINOR) or the count rule of a deletion (SCAN_DELS) or
//                       an insertion (SCAN_INS), one judge for both -- or every position gets one byte of the called
//                       sequence and nothing is compacted (SCAN_CONS).  The planes that SCAN_DELS, SCAN_INS and SCAN_CONS
//                       build from range ends (scan_run_ends; kScanEnds / kScanEnds0 say which) become counts in one
//                       place, scan_window_counts, the head of those three modes' tails.
//   k_site_scan_settle  filtered form only: the 16-code histogram of the few positions the planes cannot classify.
//   k_site_scan_ins_alleles<FILTERED>
//                       behind SCAN_INS: what was inserted at the called positions, one workgroup per position.
//
// The unfiltered form (ScanForm<false>) counts in six planes: A, C, G, T, N, any other code.  Six planes and not
// sixteen: depth = their sum, and the call needs the largest single code.  That is one of the five named planes unless
// the codes of the sixth plane (=, IUPAC ambiguity codes) together reach 7/10 of the depth; such a position cannot be
// classified from six counters (one code with 7/10 is "uncomparable", several that share it are "mixed").  It is
// reported as ambiguous and the host settles it with the 16-code histogram of cl_site_run.
//
// The filtered, strand-aware form (ScanForm<true>) is for a resident tile that carries an attachment
// (cl_site_attach_quals): per read its BAM flag, per base one pass bit (qual >= min_base_quality, taken on the host;
// bit i of word w <-> base 64 w + i in the numbering of seq4).  It runs over the same index and the same window of
// kScanWin positions per workgroup.  Relative to the unfiltered form:
//   per read   one 2-byte load of the flag and one early exit on (flag & exclude_flags); flag & 0x10 picks the strand;
//   per base   one bit of a 64-bit word of pass bits that is loaded once per CIGAR operation and once more whenever
//              the base index crosses a multiple of 64 -- never the quality bytes;
//   counters   ten LDS planes instead of six: A C G T by strand (forward, reverse), N, any other code.  Exactly 40 KB of
//              LDS per workgroup: 4 workgroups (16 waves) per CU of 160 KiB where the unfiltered kernel has 6.
// The call sums the strands and is the same rule (scan_classify); a candidate also carries the per-strand counts of its
// alternative and reference bases.  A position whose "other" plane holds 7/10 of the depth is reported as ambiguous
// exactly as in the unfiltered form, and settled with k_site_scan_settle under the same filter (cl_site_run's histogram
// is unfiltered and cannot serve).  The unfiltered instantiations hold no flag load, no pass-bit load and no test of
// use_base_quality: the filter is an empty type there and every use of it sits behind if constexpr.
//
// The minor mode (cl_site_scan_minor) asks another question of the same planes: does a second base of A C G T stand
// beside the most frequent one?  major = the largest of A C G T, minor = the largest of the other three (the first in
// that order among equals, both times); a position is low_depth (depth < min_depth, the depth of scan_classify: N and
// the other codes included), minor (c2 >= min_minor_count and 10000 c2 >= min_minor_per_10k depth, in 64 bits) or
// single.  Nothing is ambiguous: N and the other codes take part only through the depth.
//
// The deletion mode (cl_site_scan_dels) counts what the other modes step over: per position the reads whose D operation
// (CIGAR op 2; not N) covers it, beside the scan's depth.  It needs no base code and loads no seq4.  Its planes are
// depth and del (by strand under a filter) and they are built from range ends: a run of counted positions is one +1 at
// its first position and one -1 behind its last (uint32 wrap-around; a -1 that would fall on index kScanWin is dropped),
// and one workgroup-wide inclusive scan per plane turns the ends into counts.  A D operation is one run with one pass
// bit, that of its carrier: the read's last query base before it (query index y - 1, 1 <= y <= l_seq; a leading D, a D
// behind the read's last base and every D of a read without bases do not count).  Without a filter an M run is one run
// too; under a filter the depth is added per base, by the pass bits.  span = depth + del; a position is low_depth
// (span < min_depth), deleted (del >= min_del_count and 10000 del >= min_del_per_10k span, in 64 bits) or kept.
//
// The insertion mode (cl_site_scan_ins) counts the third thing the walk steps over: I operations (CIGAR op 1), at their
// anchor -- the position of the last base of the M/=/X operation directly in front (VCF's placement).  An insertion
// counts when that operation is a match of at least one base, the anchor base and every inserted base exist in the read
// (query index < l_seq), the anchor lies below min(contig_len, ref_len) and, under a base-quality filter, the anchor's pass
// bit is set.  Planes: depth and ins (by strand under a filter), the deletion mode's layout; depth is built as there, ins
// is one plain add at the anchor, so only the unfiltered depth plane is scanned.  It loads no seq4 either: a position is
// low_depth (depth < min_depth), inserted (ins >= min_ins_count and 10000 ins >= min_ins_per_10k depth, in 64 bits) or
// kept, and only for the inserted ones does k_site_scan_ins_alleles fetch the inserted bases: per counting insertion one
// observation {pos, len, key, strand}, key being the first 32 inserted 4-bit codes, most significant nibble first.
//
// The consensus mode (cl_site_scan_consensus) composes the calling rule and the deletion rule into one byte per position:
// planes A C G T rest del in both forms (strands are not kept: 24 KB, six workgroups per CU under a filter too), bases
// added as in the calling modes, del built from range ends and scanned as in the deletion mode.  span = depth + del; a
// position is low_depth (span < min_depth: n), deleted (the deletion rule over span: -), low_depth again (depth <
// min_depth: n), ref or alt (10 m >= 7 depth for the largest m of A C G T, the first among equals: the base) or no_call
// (N).  If the rest plane held 7/10 of the depth m would hold less than 3/10: nothing is ambiguous, nothing is settled.
// It compacts nothing: every thread packs its four positions' bytes into one word of a buffer indexed from the first
// window's start, and the class counts go through scan_reduce_classes.
#pragma once

#include <type_traits>

#include "kernels.hip.h"

namespace clk {

constexpr uint32_t kScanWin = 1024;          // positions per workgroup: 6 planes x 1024 x 4 B = 24 KB of LDS, 6 workgroups per CU (10 planes: 40 KB, 4)
enum { SCAN_LOW_DEPTH = 0, SCAN_MIXED = 1, SCAN_UNCOMPARABLE = 2, SCAN_MATCH = 3, SCAN_VARIANT = 4, SCAN_AMBIGUOUS = 5, SCAN_CLASSES = 6 };

// one compacted position: a variant (alt = 'A' 'C' 'G' 'T') or an ambiguous one (alt = 0, settled by the host)
struct ScanCand {
    uint32_t pos;                            // 1-based
    uint8_t  ref, alt, pad[2];
    uint32_t a, c, g, t, depth;
};

struct ScanCandEx {
    uint32_t pos;                            // 1-based
    uint8_t  ref, alt, pad[2];
    uint32_t a, c, g, t, depth;              // both strands
    uint32_t alt_fwd, alt_rev, ref_fwd, ref_rev;
};

// one compacted position of the minor mode; the strand counts are 0 in the unfiltered form
struct ScanMinorCand {
    uint32_t pos;                            // 1-based
    uint8_t  ref, major, minor, pad;
    uint32_t a, c, g, t, depth;              // both strands
    uint32_t major_fwd, major_rev, minor_fwd, minor_rev;
};
enum { MINOR_LOW_DEPTH = 0, MINOR_SINGLE = 1, MINOR_MINOR = 2 };             // its classes, in the first slots of cls

// one compacted position of the deletion or the insertion mode (there pos is the anchor), laid out as cl_del_candidate
// and cl_ins_candidate: n is the del or the ins count; the strand counts are 0 in the unfiltered form
struct ScanCountCand {
    uint32_t pos;                            // 1-based
    uint8_t  ref, pad[3];
    uint32_t n, depth;                       // both strands
    uint32_t n_fwd, n_rev, depth_fwd, depth_rev;
};
enum { COUNT_LOW_DEPTH = 0, COUNT_KEPT = 1, COUNT_CALLED = 2 };              // the two modes' classes (called: deleted, inserted), in the first slots of cls

// k_site_scan_ins_alleles: a called position as the host sends it (the candidates in ascending position; off = the
// exclusive prefix sum of their ins) and one counting insertion there as the device answers
struct ScanInsSite { uint32_t pos, ins; unsigned long long off; };          // pos 1-based
struct ScanInsObs {
    uint32_t pos, len;                       // 1-based anchor; inserted bases
    unsigned long long key[2];               // the first min(len, 32) codes: base j in key[j / 16], bits 60 - 4 (j % 16)
    uint32_t strand, pad;                    // 1 reverse (always 0 in the unfiltered form)
};

enum { CONS_LOW_DEPTH = 0, CONS_DELETED = 1, CONS_NO_CALL = 2, CONS_REF = 3, CONS_ALT = 4 };   // the consensus mode's classes, in the first slots of cls
constexpr uint32_t kConsPad = 0;             // the byte of a position of a launched window outside the range

enum ScanMode { SCAN_CALLS = 0, SCAN_DENSE = 1, SCAN_MINOR = 2, SCAN_DELS = 3, SCAN_INS = 4, SCAN_CONS = 5 };

struct ScanNoHook {};                        // a hook of scan_walk_read that a mode does not use
template <class T> inline constexpr bool scan_hooked = !std::is_same_v<std::remove_cv_t<std::remove_reference_t<T>>, ScanNoHook>;

struct ScanNoFilter {};

struct ScanFilter {
    const uint16_t *flag;                    // per read
    const unsigned long long *pass;          // one bit per base of seq4
    uint32_t exclude_flags, use_bq;
};

// everything the two forms differ in
template <bool FILTERED>
struct ScanForm {
    static constexpr uint32_t kStrands = FILTERED ? 2u : 1u;
    static constexpr uint32_t kPlanes = 4u * kStrands + 2u;    // A C G T N other, or A+ A- C+ C- G+ G- T+ T- N other  (+ forward, - reverse: flag & 0x10)
    static constexpr uint32_t kDense = 4u * kStrands + 1u;     // dense counters per position: A C G T depth, or A+ A- C+ C- G+ G- T+ T- depth
    using Cand = std::conditional_t<FILTERED, ScanCandEx, ScanCand>;
    using Filter = std::conditional_t<FILTERED, ScanFilter, ScanNoFilter>;
    // the plane of a 4-bit base code on strand rev (always 0 in the unfiltered form)
    static __device__ __forceinline__ uint32_t plane(uint32_t code, uint32_t rev)
    {
        return code == 1u ? rev : code == 2u ? kStrands + rev : code == 4u ? 2u * kStrands + rev : code == 8u ? 3u * kStrands + rev
             : code == 15u ? 4u * kStrands : 4u * kStrands + 1u;
    }
};

struct ScanIndexArgs {
    const SiteRec *rec;                      // n + 1
    const uint32_t *cigar;                   // padded by 8 words
    uint32_t n, contig_len;
    uint32_t *end;                           // n: pos + reference span, clamped to 2^32 - 1; 0 for a read that never counts
    uint32_t *wfirst, *wlast;                // per window of kScanWin positions of the contig: preset to 0xFFFFFFFF / 0
};

struct ScanArgs {
    const SiteRec *rec;
    const unsigned long long *seq_base;      // per kBlock reads: base offset of the first one
    const uint32_t *cigar;
    const uint8_t  *seq4;                    // (never read by the deletion and insertion modes)
    const uint32_t *end, *wfirst, *wlast;
    uint32_t min_quality, contig_len, min_depth;
    unsigned long long ref_len;
    uint32_t start, end_pos;                 // the range, 0-based half open, end_pos <= contig_len
    uint32_t win0;                           // window of blockIdx.x == 0
    const uint8_t *refb;                     // reference bytes of [start, min(end_pos, ref_len)), refb[0] <-> start
    unsigned long long *cls;                 // SCAN_CLASSES counts
    uint32_t *n_cand;                        // candidates wanted (also beyond cand_cap)
    uint32_t cand_cap;
    uint32_t *dense;                         // SCAN_DENSE: (end_pos - start) * ScanForm::kDense
};

// What a mode is to k_site_scan: the candidate it compacts, the thresholds of its rule beside min_depth (none, or a count and
// parts per 10 000) and, for scan_judge_positions, the class it emits.  Primary: SCAN_CALLS, whose record SCAN_DENSE keeps.
struct ScanNoThresholds {};
struct ScanThresholds { uint32_t min_count, min_per_10k; };
template <bool FILTERED, ScanMode MODE> struct ScanModeTraits {
    using Cand = typename ScanForm<FILTERED>::Cand;
    using Thresholds = ScanNoThresholds;
};
template <bool FILTERED> struct ScanModeTraits<FILTERED, SCAN_MINOR> {
    using Cand = ScanMinorCand;
    using Thresholds = ScanThresholds;
    static __device__ __forceinline__ bool emits(int cls) { return cls == MINOR_MINOR; }
};
struct ScanCountTraits {                                                      // the deletion and the insertion mode
    using Cand = ScanCountCand;
    using Thresholds = ScanThresholds;
    static __device__ __forceinline__ bool emits(int cls) { return cls == COUNT_CALLED; }
};
template <bool FILTERED> struct ScanModeTraits<FILTERED, SCAN_DELS> : ScanCountTraits {};
template <bool FILTERED> struct ScanModeTraits<FILTERED, SCAN_INS> : ScanCountTraits {};
// the consensus mode compacts nothing: its "candidates" are the packed bytes, one word per four positions
template <bool FILTERED> struct ScanModeTraits<FILTERED, SCAN_CONS> {
    using Cand = uint32_t;
    using Thresholds = ScanThresholds;                                       // the deletion rule's
};
template <bool FILTERED, ScanMode MODE> struct ScanModeArgs {                // the kernel's record
    ScanArgs s;
    typename ScanForm<FILTERED>::Filter f;
    typename ScanModeTraits<FILTERED, MODE>::Cand *cand;
    [[no_unique_address]] typename ScanModeTraits<FILTERED, MODE>::Thresholds t;
};

// LDS planes of a mode: depth and del (ins) by strand in the deletion (insertion) mode (8 KB, 16 KB); A C G T rest del in
// the consensus mode, which keeps no strands (24 KB in both forms); the form's base planes otherwise
template <ScanMode MODE> inline constexpr bool kScanTwoCounts = MODE == SCAN_DELS || MODE == SCAN_INS;
constexpr uint32_t kConsPlanes = 6u, kConsRest = 4u, kConsDel = 5u;
template <bool FILTERED, ScanMode MODE> inline constexpr uint32_t kScanPlanes = MODE == SCAN_CONS ? kConsPlanes
                                                                              : kScanTwoCounts<MODE> ? 2u * ScanForm<FILTERED>::kStrands : ScanForm<FILTERED>::kPlanes;
// ... of which the kScanEnds planes from kScanEnds0 on hold range ends that scan_window_counts turns into counts: both
// unfiltered planes and the del planes under a filter, always the last two, in the deletion mode; the unfiltered depth
// plane, the first, in the insertion mode; the del plane, the last, in the consensus mode
template <bool FILTERED, ScanMode MODE> inline constexpr uint32_t kScanEnds = MODE == SCAN_DELS ? 2u : ((MODE == SCAN_INS && !FILTERED) || MODE == SCAN_CONS) ? 1u : 0u;
template <bool FILTERED, ScanMode MODE> inline constexpr uint32_t kScanEnds0 = MODE == SCAN_DELS ? kScanPlanes<FILTERED, MODE> - 2u : MODE == SCAN_CONS ? kConsDel : 0u;
// the modes whose tail is scan_window_counts: their planes are read four words at a time
template <ScanMode MODE> inline constexpr bool kScanQuads = kScanTwoCounts<MODE> || MODE == SCAN_CONS;

// number of CIGAR operations and bases of a read, with SiteRec's escape to the next record's offsets
__device__ __forceinline__ void scan_read_extent(const SiteRec *rec, uint32_t r, const uint4 &rr, uint32_t &k1, unsigned long long &slen)
{
    k1 = rr.y + ((rr.w >> 8) & 255u);
    slen = rr.w >> 16;
    if (((rr.w >> 8) & 255u) == 255u || slen == 0xFFFFull) {
        const uint4 nx = *reinterpret_cast<const uint4 *>(rec + r + 1);
        k1 = nx.y; slen = (uint32_t)(nx.z - rr.z);
    }
}

__global__ __launch_bounds__(kBlock) void k_site_scan_index(ScanIndexArgs a)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= a.n) return;
    const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
    uint32_t e = 0;
    if ((uint32_t)rr.x < a.contig_len) {                                    // fetch("chr:1-len"), caller.rs:33-36
        uint32_t k1; unsigned long long slen;
        scan_read_extent(a.rec, r, rr, k1, slen);
        unsigned long long reflen = 0;
        for (uint32_t kk = rr.y; kk < k1; ++kk) {
            const uint32_t c = a.cigar[kk];
            reflen += ((0x18Du >> (c & 15u)) & 1u) ? (c >> 4) : 0u;
        }
        if (reflen) {
            const unsigned long long x = (uint32_t)rr.x, xe = x + reflen;
            e = xe > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)xe;
            const uint32_t last_p = (e > a.contig_len ? a.contig_len : e) - 1u;   // x < contig_len and e > x: >= x
            for (uint32_t w = (uint32_t)x / kScanWin; w <= last_p / kScanWin; ++w) {
                atomicMin(&a.wfirst[w], r);
                atomicMax(&a.wlast[w], r + 1u);
            }
        }
    }
    a.end[r] = e;
}

// window w of the contig: [ws, ws + kScanWin); [lo, we) is the part that is asked for, [lo, hi) the part that can hold a
// count (p < ref_len, caller.rs:110-113).  lo <= we: the host launches overlapping windows only
struct ScanWindow { uint32_t ws, lo, we, hi; };

__device__ __forceinline__ ScanWindow scan_window(const ScanArgs &a, uint32_t w)
{
    const unsigned long long ws64 = (unsigned long long)w * kScanWin;
    ScanWindow v;
    v.ws = (uint32_t)ws64;
    v.lo = v.ws > a.start ? v.ws : a.start;
    v.we = (ws64 + kScanWin < (unsigned long long)a.end_pos) ? v.ws + kScanWin : a.end_pos;
    v.hi = (unsigned long long)v.we < a.ref_len ? v.we : (uint32_t)a.ref_len;
    return v;
}

// read start < contig_len (end = 0 otherwise), the mapping-quality gate (caller.rs:80), overlap with [lo, hi)
__device__ __forceinline__ bool scan_read_counts(const ScanArgs &a, const uint4 &rr, uint32_t e, uint32_t lo, uint32_t hi)
{
    return (rr.w & 255u) >= a.min_quality && e > lo && (uint32_t)rr.x < hi;
}

// The walk of read r over the bases of its M/=/X operations at the positions of [lo, hi).  Per operation:
// run = begin_run(bi, any) with the base bi of its first position in [lo, hi), in the numbering of seq4, and whether it
// has one at all; then per_base(p, bi, run) for every position p.  What a form keeps from base to base (the word of pass
// bits) is that run value: it does not outlive the operation, and so holds no register across the CIGAR loop.
// Two more hooks, for the deletion mode (ScanNoHook: not compiled in): on_run(p0, p1) once per M/=/X operation with a
// position in [lo, hi), [p0, p1) being the positions per_base would see; on_del(p0, p1, ci) once per D operation (op 2,
// not N) whose carrier exists, [p0, p1) being its positions in [lo, hi) and ci the carrier's base in the numbering of
// seq4.  per_base itself may be ScanNoHook.
// One more, for the insertion mode: on_ins(p, anchor_bi, first_bi, len) once per I operation (op 1) that stands directly
// behind an M/=/X operation of at least one base whose last position p lies in [lo, hi), when that base and all len
// inserted bases exist (query index < l_seq); anchor_bi and first_bi are the anchor's and the first inserted base in the
// numbering of seq4.  It fires from the match branch, by the next CIGAR word: an M that ends exactly at hi ends the loop.
template <class BeginRun, class PerBase, class OnRun = ScanNoHook, class OnDel = ScanNoHook, class OnIns = ScanNoHook>
__device__ __forceinline__ void scan_walk_read(const ScanArgs &a, uint32_t r, const uint4 &rr, uint32_t lo, uint32_t hi, BeginRun &&begin_run,
                                               PerBase &&per_base, OnRun &&on_run = OnRun{}, OnDel &&on_del = OnDel{}, OnIns &&on_ins = OnIns{})
{
    uint32_t k1; unsigned long long slen;
    scan_read_extent(a.rec, r, rr, k1, slen);
    const unsigned long long base = a.seq_base[r / kBlock];
    const unsigned long long s0 = base + (uint32_t)(rr.z - (uint32_t)base);
    unsigned long long x = (uint32_t)rr.x, y = 0;
    for (uint32_t kk = rr.y; kk < k1 && x < hi; ++kk) {
        const uint32_t c = a.cigar[kk];
        const uint32_t op = c & 15u, l = c >> 4;
        if (op_match(op)) {
            // [x, x + l) cut to [lo, hi) and to the bases the read has (query index < l_seq, caller.rs:105)
            unsigned long long p0 = x > lo ? x : lo, p1 = x + l < hi ? x + l : hi;
            if (y < slen) { if (p1 - x > slen - y && p1 > x) p1 = x + (slen - y); } else p1 = p0;
            if constexpr (scan_hooked<OnRun>) { if (p0 < p1) on_run((uint32_t)p0, (uint32_t)p1); }
            if constexpr (scan_hooked<PerBase>) {
                unsigned long long bi = s0 + y + (p0 - x);
                auto run = begin_run(bi, p0 < p1);
                for (unsigned long long p = p0; p < p1; ++p, ++bi) per_base((uint32_t)p, bi, run);
            }
            if constexpr (scan_hooked<OnIns>) {
                const unsigned long long pa = x + l - 1ull;                    // the anchor: this operation's last position
                if (l && pa >= lo && pa < hi && kk + 1u < k1) {
                    const uint32_t cn = a.cigar[kk + 1u];
                    // the anchor base (query index y + l - 1) and the cn >> 4 bases behind it exist
                    if ((cn & 15u) == 1u && y + l + (cn >> 4) <= slen) on_ins((uint32_t)pa, s0 + y + l - 1ull, s0 + y + l, cn >> 4);
                }
            }
            x += l; y += l;
        } else if (op_del(op)) {
            if constexpr (scan_hooked<OnDel>) {
                if (op == 2u && y >= 1ull && y <= slen) {                      // the carrier: query index y - 1
                    const unsigned long long p0 = x > lo ? x : lo, p1 = x + l < hi ? x + l : hi;
                    if (p0 < p1) on_del((uint32_t)p0, (uint32_t)p1, s0 + y - 1ull);
                }
            }
            x += l;
        } else if (op_ins(op)) {
            y += l;
        }
    }
}

__device__ __forceinline__ uint32_t scan_base_code(const uint8_t *seq4, unsigned long long bi)
{
    const uint32_t byte = seq4[bi >> 1];
    return (bi & 1ull) ? (byte & 15u) : (byte >> 4);
}

// the word of pass bits of a run's first base bi (all ones without a base-quality filter) ...
__device__ __forceinline__ unsigned long long scan_pass_word(const ScanFilter &f, unsigned long long bi, bool any)
{
    return (f.use_bq && any) ? f.pass[bi >> 6] : ~0ull;
}

// ... and the pass bit of base bi of that run: pw is loaded again when bi crosses a multiple of 64
__device__ __forceinline__ bool scan_base_passes(const ScanFilter &f, unsigned long long bi, unsigned long long &pw)
{
    if (!f.use_bq) return true;
    if ((bi & 63ull) == 0ull) pw = f.pass[bi >> 6];
    return (pw >> (bi & 63ull)) & 1ull;
}

// the pass bit of a single base b, loaded for it alone: a D operation's carrier, an I operation's anchor
__device__ __forceinline__ bool scan_pass_bit(const ScanFilter &f, unsigned long long b)
{
    return !f.use_bq || ((f.pass[b >> 6] >> (b & 63ull)) & 1ull);
}

// the unfiltered form of the three: nothing is kept from base to base and every base passes
__device__ __forceinline__ ScanNoFilter scan_pass_word(const ScanNoFilter &, unsigned long long, bool) { return {}; }
__device__ __forceinline__ bool scan_base_passes(const ScanNoFilter &, unsigned long long, ScanNoFilter &) { return true; }
__device__ __forceinline__ bool scan_pass_bit(const ScanNoFilter &, unsigned long long) { return true; }

// the begin_run of scan_walk_read for a form's filter
template <class Filter>
__device__ __forceinline__ auto scan_begin_run(const Filter &f)
{
    return [&f](unsigned long long bi, bool any) { return scan_pass_word(f, bi, any); };
}

// A run of counted positions [o0, o1) of the window in a plane of range ends: +1 at its first position, -1 behind its last
// (uint32 wrap-around; a -1 that would fall on index kScanWin is dropped).  scan_window_counts turns the ends into counts.
__device__ __forceinline__ void scan_run_ends(uint32_t *plane, uint32_t o0, uint32_t o1)
{
    atomicAdd(&plane[o0], 1u);
    if (o1 < kScanWin) atomicAdd(&plane[o1], 0xFFFFFFFFu);
}

// The calling rule.  Returns the class; rb becomes the upper-cased reference byte (anything but ACGT is "other"),
// alt the most frequent of A C G T N (the first in that order among equals) and ai its index in that order.
__device__ __forceinline__ int scan_classify(uint32_t A, uint32_t Cc, uint32_t G, uint32_t T, uint32_t N, uint32_t O, uint32_t &rb, uint32_t min_depth,
                                             uint32_t &alt, uint32_t &ai, unsigned long long &depth)
{
    depth = (unsigned long long)A + Cc + G + T + N + O;                     // below 2^32: one count per read
    uint32_t m = A; alt = 'A'; ai = 0;
    if (Cc > m) { m = Cc; alt = 'C'; ai = 1; }
    if (G > m) { m = G; alt = 'G'; ai = 2; }
    if (T > m) { m = T; alt = 'T'; ai = 3; }
    if (N > m) { m = N; alt = 'N'; ai = 4; }
    rb &= ~32u;
    const bool ref_ok = rb == 'A' || rb == 'C' || rb == 'G' || rb == 'T';
    // called <=> m / depth >= 0.7 in f64 <=> 10 m >= 7 depth (a ratio off 7/10 is off by more than an f64 divide rounds)
    if (depth < min_depth) return SCAN_LOW_DEPTH;
    if (10ull * m >= 7ull * depth) return (alt == 'N' || !ref_ok) ? SCAN_UNCOMPARABLE : (alt == rb ? SCAN_MATCH : SCAN_VARIANT);
    if (10ull * O >= 7ull * depth) return SCAN_AMBIGUOUS;
    return SCAN_MIXED;
}

// the candidates of a wave go out behind one another: one ballot, one atomic of lane 0 (every lane of the wave calls)
template <class Cand>
__device__ __forceinline__ void scan_compact(bool emit, const Cand &cd, uint32_t lane, uint32_t *n_cand, Cand *cand, uint32_t cand_cap)
{
    const unsigned long long bal = __ballot(emit);
    if (!bal) return;
    uint32_t base_i = 0;
    if (lane == 0) base_i = atomicAdd(n_cand, (uint32_t)__popcll(bal));
    base_i = __shfl(base_i, 0);
    if (emit) {
        const uint32_t i = base_i + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (i < cand_cap) cand[i] = cd;
    }
}

// The class counts of the threads: by wave, then by workgroup in s_cls, then one atomic per class.  s_cls is the first
// words of the counter planes (the filtered kernel has exactly 40 KB: four workgroups fit a CU's 160 KiB, a byte more
// and only three do), so it is cleared only once every thread has read its counters.
__device__ __forceinline__ void scan_reduce_classes(const uint32_t (&mine)[SCAN_CLASSES], unsigned long long *s_cls, unsigned long long *cls,
                                                    uint32_t tid, uint32_t lane)
{
    __syncthreads();
    if (tid < (uint32_t)SCAN_CLASSES) s_cls[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SCAN_CLASSES; ++k) {
        uint32_t v = mine[k];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
        if (lane == 0 && v) atomicAdd(&s_cls[k], (unsigned long long)v);
    }
    __syncthreads();
    if (tid < (uint32_t)SCAN_CLASSES && s_cls[tid]) atomicAdd(&cls[tid], s_cls[tid]);
}

// The second-allele rule.  cnt: A C G T.  major / minor become the indices of the largest and of the largest of the
// other three (the first in that order among equals), c2 the latter's count.
__device__ __forceinline__ int scan_classify_minor(const uint32_t (&cnt)[4], unsigned long long depth, uint32_t min_depth, uint32_t min_minor_count,
                                                   uint32_t min_minor_per_10k, uint32_t &major, uint32_t &minor, uint32_t &c2)
{
    uint32_t c1 = cnt[0];
    major = 0;
#pragma unroll
    for (uint32_t b = 1; b < 4u; ++b) if (cnt[b] > c1) { c1 = cnt[b]; major = b; }
    minor = major == 0u ? 1u : 0u;
    c2 = major == 0u ? cnt[1] : cnt[0];
#pragma unroll
    for (uint32_t b = 1; b < 4u; ++b) if (b != major && cnt[b] > c2) { c2 = cnt[b]; minor = b; }
    if (depth < min_depth) return MINOR_LOW_DEPTH;
    return (c2 >= min_minor_count && 10000ull * c2 >= (unsigned long long)min_minor_per_10k * depth) ? MINOR_MINOR : MINOR_SINGLE;
}

// The consensus rule: the deletion rule over span = depth + del first, then the calling rule over A C G T alone (rest: N
// and every other code, which take part only through the depth).  Returns the class; byte becomes n, -, the called base or N.
__device__ __forceinline__ int scan_classify_cons(uint32_t A, uint32_t Cc, uint32_t G, uint32_t T, uint32_t rest, uint32_t del, uint32_t rb, uint32_t min_depth,
                                                  uint32_t min_del_count, uint32_t min_del_per_10k, uint32_t &byte)
{
    const unsigned long long depth = (unsigned long long)A + Cc + G + T + rest, span = depth + del;
    uint32_t m = A, called = 'A';
    if (Cc > m) { m = Cc; called = 'C'; }
    if (G > m) { m = G; called = 'G'; }
    if (T > m) { m = T; called = 'T'; }
    byte = 'n';
    if (span < min_depth) return CONS_LOW_DEPTH;
    if (del >= min_del_count && 10000ull * del >= (unsigned long long)min_del_per_10k * span) { byte = '-'; return CONS_DELETED; }
    if (depth < min_depth) return CONS_LOW_DEPTH;
    if (10ull * m >= 7ull * depth) { byte = called; return called == (rb & ~32u) ? CONS_REF : CONS_ALT; }
    byte = 'N';
    return CONS_NO_CALL;
}

// The tail of the second-allele rule and of the count rule (the calling rule keeps its own, in the kernel).  A thread has kScanWin / kBlock
// positions: offset(j) is the window offset o of its j-th, judge(j, o, ref, cd) returns the class of position ws + o and
// fills cd but for its pos, ref() being the reference byte as sent ('N' at and beyond hi).  The emitted class is compacted.
template <bool FILTERED, ScanMode MODE, class Offset, class Judge>
__device__ __forceinline__ void scan_judge_positions(const ScanModeArgs<FILTERED, MODE> &ax, const ScanWindow &win, uint32_t *s_cnt, Offset &&offset, Judge &&judge)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t mine[SCAN_CLASSES] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < kScanWin / (uint32_t)kBlock; ++j) {                   // (uniform trip count: the ballot needs whole waves)
        const uint32_t o = offset(j), p = win.ws + o;
        int cls = -1;
        typename ScanModeTraits<FILTERED, MODE>::Cand cd;
        if (p >= win.lo && p < win.we) {
            cls = judge(j, o, [&]() -> uint32_t { return p < win.hi ? ax.s.refb[p - ax.s.start] : (uint32_t)'N'; }, cd);
            mine[cls] += 1u;
            cd.pos = p + 1u;
        }
        scan_compact(ScanModeTraits<FILTERED, MODE>::emits(cls), cd, lane, ax.s.n_cand, ax.cand, ax.s.cand_cap);
    }
    scan_reduce_classes(mine, reinterpret_cast<unsigned long long *>(s_cnt), ax.s.cls, tid, lane);     // (s_cnt: every judge has read it)
}

// The finished planes of a window into registers, four consecutive positions per thread: q[k][j] = plane k at window offset
// 4 tid + j.  The planes of range ends (kScanEnds of them from kScanEnds0 on, scan_run_ends) become counts on the way, by one
// inclusive scan over the window each: within the thread, over the wave by DPP, over the workgroup through the waves'
// totals, behind one barrier for all of them.  Sums are modulo 2^32, so a -1 may stand in front of its +1's total.
template <bool FILTERED, ScanMode MODE>
__device__ __forceinline__ void scan_window_counts(const uint32_t *s_cnt, uint32_t (&q)[kScanPlanes<FILTERED, MODE>][4])
{
    static_assert(kScanWin == 4u * (uint32_t)kBlock, "four positions per thread");
    constexpr uint32_t kE0 = kScanEnds0<FILTERED, MODE>, kEnds = kScanEnds<FILTERED, MODE>;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
#pragma unroll
    for (uint32_t k = 0; k < kScanPlanes<FILTERED, MODE>; ++k) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&s_cnt[k * kScanWin + 4u * tid]);
        q[k][0] = v.x; q[k][1] = v.y; q[k][2] = v.z; q[k][3] = v.w;
    }
    if constexpr (kEnds > 0u) {
        __shared__ uint32_t s_wtot[kEnds][kBlock / 64];
        uint32_t before[kEnds];                                                // the sum of the wave's earlier threads
#pragma unroll
        for (uint32_t e = 0; e < kEnds; ++e) {
            uint32_t (&v)[4] = q[kE0 + e];
            v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
            const uint32_t inc = dpp_incl_scan_u32(v[3]);
            if (lane == 63u) s_wtot[e][wv] = inc;
            before[e] = inc - v[3];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t e = 0; e < kEnds; ++e) {
            uint32_t add = before[e];
#pragma unroll
            for (uint32_t j = 0; j < (uint32_t)kBlock / 64u; ++j) add += j < wv ? s_wtot[e][j] : 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) q[kE0 + e][j] += add;
        }
    }
}

template <bool FILTERED, ScanMode MODE>
__global__ __launch_bounds__(kBlock) void k_site_scan(ScanModeArgs<FILTERED, MODE> ax)
{
    using Form = ScanForm<FILTERED>;
    constexpr uint32_t S = Form::kStrands;
    constexpr uint32_t kPlanes = kScanPlanes<FILTERED, MODE>;
    __shared__ alignas(kScanQuads<MODE> ? 16 : 8) uint32_t s_cnt[kPlanes * kScanWin];
    const ScanArgs &a = ax.s;
    const uint32_t tid = threadIdx.x;
    const uint32_t w = a.win0 + blockIdx.x;
    const ScanWindow win = scan_window(a, w);
    const uint32_t ws = win.ws, lo = win.lo, we = win.we, hi = win.hi;
    for (uint32_t i = tid; i < kPlanes * kScanWin; i += kBlock) s_cnt[i] = 0;
    __syncthreads();
    const uint32_t r_first = a.wfirst[w], r_last = a.wlast[w];
    if (r_first < r_last && lo < hi) {
        for (uint32_t r = r_first + tid; r < r_last; r += kBlock) {
            const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
            if (!scan_read_counts(a, rr, a.end[r], lo, hi)) continue;
            uint32_t rev = 0;
            if constexpr (FILTERED) {
                const uint32_t fl = ax.f.flag[r];
                if (fl & ax.f.exclude_flags) continue;
                rev = (fl >> 4) & 1u;
            }
            // The hooks the modes hang on the walk.  Planes: the form's base planes (calling modes), A C G T rest del (consensus),
            // depth by strand then del or ins by strand (deletion, insertion); second = the plane of this read's del or ins.
            constexpr bool kDepthFromEnds = kScanTwoCounts<MODE> && !FILTERED;   // without a filter an M run is one run of the depth plane
            const uint32_t second = MODE == SCAN_CONS ? kConsDel : S + rev;
            auto add = [&](uint32_t plane, uint32_t p) { atomicAdd(&s_cnt[plane * kScanWin + (p - ws)], 1u); };
            auto ends = [&](uint32_t plane, uint32_t p0, uint32_t p1) { scan_run_ends(&s_cnt[plane * kScanWin], p0 - ws, p1 - ws); };
            const auto begin_run = scan_begin_run(ax.f);
            auto base_by_code = [&](uint32_t p, unsigned long long bi, auto &pw) {
                if (!scan_base_passes(ax.f, bi, pw)) return;
                const uint32_t code = scan_base_code(a.seq4, bi);
                if constexpr (MODE == SCAN_CONS) add(code == 1u ? 0u : code == 2u ? 1u : code == 4u ? 2u : code == 8u ? 3u : kConsRest, p);
                else add(Form::plane(code, rev), p);
            };
            auto depth_by_base = [&](uint32_t p, unsigned long long bi, auto &pw) { if (scan_base_passes(ax.f, bi, pw)) add(rev, p); };
            auto depth_by_run = [&](uint32_t p0, uint32_t p1) { ends(0u, p0, p1); };
            auto del_run = [&](uint32_t p0, uint32_t p1, unsigned long long ci) { if (scan_pass_bit(ax.f, ci)) ends(second, p0, p1); };
            auto ins_anchor = [&](uint32_t p, unsigned long long ai, unsigned long long, uint32_t) { if (scan_pass_bit(ax.f, ai)) add(second, p); };
            if constexpr (MODE == SCAN_CONS) scan_walk_read(a, r, rr, lo, hi, begin_run, base_by_code, ScanNoHook{}, del_run);
            else if constexpr (MODE == SCAN_DELS && kDepthFromEnds) scan_walk_read(a, r, rr, lo, hi, ScanNoHook{}, ScanNoHook{}, depth_by_run, del_run);
            else if constexpr (MODE == SCAN_DELS) scan_walk_read(a, r, rr, lo, hi, begin_run, depth_by_base, ScanNoHook{}, del_run);
            else if constexpr (MODE == SCAN_INS && kDepthFromEnds) scan_walk_read(a, r, rr, lo, hi, ScanNoHook{}, ScanNoHook{}, depth_by_run, ScanNoHook{}, ins_anchor);
            else if constexpr (MODE == SCAN_INS) scan_walk_read(a, r, rr, lo, hi, begin_run, depth_by_base, ScanNoHook{}, ScanNoHook{}, ins_anchor);
            else scan_walk_read(a, r, rr, lo, hi, begin_run, base_by_code);
        }
    }
    __syncthreads();
    if constexpr (MODE == SCAN_DENSE) {
        // kDense counters per position of the range, in the order of the output array: consecutive threads, consecutive words
        const uint32_t nd = (we - lo) * Form::kDense;
        uint32_t *out = a.dense + (unsigned long long)(lo - a.start) * Form::kDense;
        for (uint32_t i = tid; i < nd; i += kBlock) {
            const uint32_t q = i / Form::kDense, cc = i - q * Form::kDense, o = lo - ws + q;
            uint32_t v;
            if (cc < Form::kDense - 1u) v = s_cnt[cc * kScanWin + o];
            else { v = 0; for (uint32_t k = 0; k < kPlanes; ++k) v += s_cnt[k * kScanWin + o]; }
            out[i] = v;
        }
    } else if constexpr (MODE == SCAN_CONS) {
        // The counts of the thread's four positions (scan_window_counts), the rule per position and one aligned word of four
        // bytes per thread: the buffer is indexed from the first window's start, so word blockIdx.x * kBlock + tid holds
        // positions ws + 4 tid .. + 3 whatever the range's start is.
        uint32_t q[kPlanes][4];
        scan_window_counts<FILTERED, MODE>(s_cnt, q);
        const uint32_t lane = tid & 63u;
        uint32_t mine[SCAN_CLASSES] = {0, 0, 0, 0, 0, 0};
        uint32_t word = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t p = ws + 4u * tid + j;
            uint32_t byte = kConsPad;
            if (p >= lo && p < we) {
                const uint32_t rb = p < hi ? a.refb[p - a.start] : (uint32_t)'N';
                const int cls = scan_classify_cons(q[0][j], q[1][j], q[2][j], q[3][j], q[kConsRest][j], q[kConsDel][j], rb, a.min_depth,
                                                   ax.t.min_count, ax.t.min_per_10k, byte);
                mine[cls] += 1u;
            }
            word |= byte << (8u * j);
        }
        ax.cand[(size_t)blockIdx.x * kBlock + tid] = word;
        scan_reduce_classes(mine, reinterpret_cast<unsigned long long *>(s_cnt), a.cls, tid, lane);     // (s_cnt: every thread has read it)
    } else if constexpr (kScanTwoCounts<MODE>) {
        // The count rule of both modes over the thread's four positions (scan_window_counts): n, the del or ins count, against
        // the rule's denominator -- span = depth + del for a deletion, which takes its reads out of the depth; the depth for
        // an insertion, whose reads are in it.  low_depth below min_depth of it, called at min_count and min_per_10k of it.
        uint32_t q[kPlanes][4];
        scan_window_counts<FILTERED, MODE>(s_cnt, q);
        scan_judge_positions(ax, win, s_cnt, [&](uint32_t j) { return 4u * tid + j; }, [&](uint32_t j, uint32_t, auto &&ref, ScanCountCand &cd) {
            // (j is a constant of the unrolled loop: q stays in registers)
            const uint32_t depth_f = q[0][j], depth_r = FILTERED ? q[S - 1u][j] : 0u, n_f = q[S][j], n_r = FILTERED ? q[2u * S - 1u][j] : 0u;
            const unsigned long long depth = (unsigned long long)depth_f + depth_r, n = (unsigned long long)n_f + n_r, of = MODE == SCAN_DELS ? depth + n : depth;
            const int cls = of < a.min_depth ? COUNT_LOW_DEPTH
                          : (n >= ax.t.min_count && 10000ull * n >= (unsigned long long)ax.t.min_per_10k * of) ? COUNT_CALLED : COUNT_KEPT;
            cd.ref = (uint8_t)(ref() & ~32u); cd.pad[0] = cd.pad[1] = cd.pad[2] = 0;
            cd.n = (uint32_t)n; cd.depth = (uint32_t)depth;
            cd.n_fwd = FILTERED ? n_f : 0u; cd.n_rev = n_r; cd.depth_fwd = FILTERED ? depth_f : 0u; cd.depth_rev = depth_r;
            return cls;
        });
    } else if constexpr (MODE == SCAN_MINOR) {
        scan_judge_positions(ax, win, s_cnt, [&](uint32_t j) { return j * (uint32_t)kBlock + tid; }, [&](uint32_t, uint32_t o, auto &&ref, ScanMinorCand &cd) {
            uint32_t f[4], v[4], cnt[4];                                    // A C G T: forward, reverse, both
            unsigned long long depth = (unsigned long long)s_cnt[(4u * S) * kScanWin + o] + s_cnt[(4u * S + 1u) * kScanWin + o];
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) {
                f[b] = s_cnt[(S * b) * kScanWin + o]; v[b] = FILTERED ? s_cnt[(S * b + 1u) * kScanWin + o] : 0u;
                cnt[b] = f[b] + v[b]; depth += cnt[b];
            }
            uint32_t major, minor, c2;
            const int cls = scan_classify_minor(cnt, depth, a.min_depth, ax.t.min_count, ax.t.min_per_10k, major, minor, c2);
            cd.ref = (uint8_t)(ref() & ~32u); cd.pad = 0;
            cd.major = (uint8_t)(0x54474341u >> (8u * major)); cd.minor = (uint8_t)(0x54474341u >> (8u * minor));   // "ACGT"
            cd.a = cnt[0]; cd.c = cnt[1]; cd.g = cnt[2]; cd.t = cnt[3]; cd.depth = (uint32_t)depth;
            cd.major_fwd = cd.major_rev = cd.minor_fwd = cd.minor_rev = 0;
            if constexpr (FILTERED) {
#pragma unroll
                for (uint32_t b = 0; b < 4u; ++b) {                           // (selects, not indexed registers)
                    if (b == major) { cd.major_fwd = f[b]; cd.major_rev = v[b]; }
                    if (b == minor) { cd.minor_fwd = f[b]; cd.minor_rev = v[b]; }
                }
            }
            return cls;
        });
    } else {
        // (a tail of its own: through scan_judge_positions the filtered form was 2 % slower, profiles/r14_scan_modes_folded.txt)
        uint32_t mine[SCAN_CLASSES] = {0, 0, 0, 0, 0, 0};
        const uint32_t lane = tid & 63u;
        for (uint32_t o0 = 0; o0 < kScanWin; o0 += kBlock) {                   // (uniform trip count: the ballot needs whole waves)
            const uint32_t o = o0 + tid, p = ws + o;
            int cls = -1;
            typename Form::Cand cd;
            if (p >= lo && p < we) {
                uint32_t f[4], v[4];                                            // A C G T, forward and reverse
#pragma unroll
                for (uint32_t b = 0; b < 4u; ++b) { f[b] = s_cnt[(S * b) * kScanWin + o]; v[b] = FILTERED ? s_cnt[(S * b + 1u) * kScanWin + o] : 0u; }
                const uint32_t A = f[0] + v[0], Cc = f[1] + v[1], G = f[2] + v[2], T = f[3] + v[3];
                uint32_t rb = p < hi ? a.refb[p - a.start] : (uint32_t)'N', alt, ai;
                unsigned long long depth;
                cls = scan_classify(A, Cc, G, T, s_cnt[(4u * S) * kScanWin + o], s_cnt[(4u * S + 1u) * kScanWin + o], rb, a.min_depth, alt, ai, depth);
                mine[cls] += 1u;
                cd.pos = p + 1u; cd.ref = (uint8_t)rb; cd.alt = cls == SCAN_VARIANT ? (uint8_t)alt : (uint8_t)0; cd.pad[0] = cd.pad[1] = 0;
                cd.a = A; cd.c = Cc; cd.g = G; cd.t = T; cd.depth = (uint32_t)depth;
                if constexpr (FILTERED) {
                    cd.alt_fwd = cd.alt_rev = cd.ref_fwd = cd.ref_rev = 0;
                    if (cls == SCAN_VARIANT) {
                        const uint32_t ri = rb == 'A' ? 0u : rb == 'C' ? 1u : rb == 'G' ? 2u : 3u;    // (a variant's reference base is of ACGT)
#pragma unroll
                        for (uint32_t b = 0; b < 4u; ++b) {                       // (selects, not indexed registers)
                            if (b == ai) { cd.alt_fwd = f[b]; cd.alt_rev = v[b]; }
                            if (b == ri) { cd.ref_fwd = f[b]; cd.ref_rev = v[b]; }
                        }
                    }
                }
            }
            scan_compact(cls == SCAN_VARIANT || cls == SCAN_AMBIGUOUS, cd, lane, a.n_cand, ax.cand, a.cand_cap);
        }
        scan_reduce_classes(mine, reinterpret_cast<unsigned long long *>(s_cnt), a.cls, tid, lane);
    }
}

// The 16-code histogram of single positions under the filter of ax: one workgroup per position of pos1 (1-based, inside
// the contig), over the reads of the position's window range.  For the few positions the ten planes cannot classify.
__global__ __launch_bounds__(kBlock) void k_site_scan_settle(ScanModeArgs<true, SCAN_CALLS> ax, const uint32_t *pos1, uint32_t *hist16)
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
            if (!scan_read_counts(a, rr, a.end[r], p, p + 1u)) continue;       // (p < contig_len <= 2^32 - 1)
            if ((uint32_t)ax.f.flag[r] & ax.f.exclude_flags) continue;
            scan_walk_read(a, r, rr, p, p + 1u, scan_begin_run(ax.f),
                [&](uint32_t, unsigned long long bi, unsigned long long &pw) {
                    if (scan_base_passes(ax.f, bi, pw)) atomicAdd(&s_h[scan_base_code(a.seq4, bi)], 1u);
                });
        }
    }
    __syncthreads();
    if (tid < 16u) hist16[(size_t)blockIdx.x * 16u + tid] = s_h[tid];
}

// What was inserted at the called positions of the insertion mode: one workgroup per site (ascending, off = the exclusive
// prefix sum of their ins), over the reads of the site's window range, under the gates and the filter of ax.  Every
// counting insertion anchored there takes a slot k of the workgroup's counter and, if k < ins, stores its observation at
// obs[off + k]: the buffer is exact and nothing is stored beyond a site's own slots.  found[c] = the slots taken.
template <bool FILTERED>
__global__ __launch_bounds__(kBlock) void k_site_scan_ins_alleles(ScanModeArgs<FILTERED, SCAN_INS> ax, const ScanInsSite *site, ScanInsObs *obs, uint32_t *found)
{
    __shared__ uint32_t s_n;
    const ScanArgs &a = ax.s;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const ScanInsSite st = site[blockIdx.x];
    const uint32_t p = st.pos - 1u;
    const uint32_t w = p / kScanWin;
    const uint32_t r_first = a.wfirst[w], r_last = a.wlast[w];
    if (r_first < r_last && (unsigned long long)p < a.ref_len) {
        for (uint32_t r = r_first + tid; r < r_last; r += kBlock) {
            const uint4 rr = *reinterpret_cast<const uint4 *>(a.rec + r);
            if (!scan_read_counts(a, rr, a.end[r], p, p + 1u)) continue;       // (p < contig_len <= 2^32 - 1)
            uint32_t rev = 0;
            if constexpr (FILTERED) {
                const uint32_t fl = ax.f.flag[r];
                if (fl & ax.f.exclude_flags) continue;
                rev = (fl >> 4) & 1u;
            }
            scan_walk_read(a, r, rr, p, p + 1u, ScanNoHook{}, ScanNoHook{}, ScanNoHook{}, ScanNoHook{},
                [&](uint32_t, unsigned long long ai, unsigned long long bi, uint32_t len) {
                    if (!scan_pass_bit(ax.f, ai)) return;
                    const uint32_t k = atomicAdd(&s_n, 1u);
                    if (k >= st.ins) return;
                    ScanInsObs o;
                    o.pos = st.pos; o.len = len; o.key[0] = o.key[1] = 0; o.strand = rev; o.pad = 0;
                    const uint32_t n = len < 32u ? len : 32u;
                    for (uint32_t j = 0; j < n; ++j) {
                        const unsigned long long code = scan_base_code(a.seq4, bi + j);
                        if (j < 16u) o.key[0] |= code << (60u - 4u * j); else o.key[1] |= code << (60u - 4u * (j - 16u));
                    }
                    obs[st.off + k] = o;
                });
        }
    }
    __syncthreads();
    if (tid == 0) found[blockIdx.x] = s_n;
}

} // namespace clk
