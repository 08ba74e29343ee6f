// pass_rows.h -- the pass-bit ROWS of the pileup kernel, built on the host at upload (plain C++, no HIP).
//
// qc_depth of a position (mod.rs:30-37) = the number of reads with mapq >= min_mapping_quality that have an M/=/X base
// there whose quality byte passes min_base_quality.  The byte test is taken once on the host (qual_pack.cpp: one bit
// per base, in query order, bit g of the contig's bit array <-> quality byte g); here the bits are laid out the way the
// kernel counts them: per window of T reference positions a stack of ROWS, a row = T bits, bit p of a row <-> reference
// position W + p.  Every read that covers the window gets one row in which no other read of the window overlaps it
// (reads arrive sorted by start: a row is free again when its last read has ended, and a new row is opened only when
// none is free, so a window has exactly as many rows as its deepest column of such reads); its M/=/X bases drop their
// pass bits at their reference positions, everything else (D, N, clipped and inserted bases, bases without a quality
// byte) stays 0.  The kernel then needs no CIGAR, no offsets and no shifts: qc_depth[p] = the number of rows with bit p
// set, a bit-sliced column sum over a coalesced stream.
//
// What the device holds (rows_window_segments): a window is cut into 8 SEGMENTS of 256 positions -- 8 blocks of 32, the
// blocks of lanes 8 s .. 8 s + 7 --, and every segment has a row stack of its own, as high as ITS deepest column: depth
// varies along a window, and a stack per window stored every block at the height of the deepest one.  A read takes a
// free row in every segment it overlaps.  Rows come in groups of 4; a UNIT = one group of one segment = 8 blocks x 4 rows
// x 32 bits = 128 bytes, dword index ((block & 7) << 2) | (row & 3) -- one 16-byte load per lane and group, one L2 line
// per segment.  A window's units are contiguous, segment after segment: segment s holds h_s units, the eight heights
// travel in the window's record (rows_heights_word).
//
// rows_window builds the UNIFORM layout, one stack per window: groups of 4 rows; a group = 64 blocks (32 positions each)
// x 4 rows x 32 bits = 1 KB, dword index (block << 2) | (row & 3).  It is what the segments are held against
// (cl_debug_pass_rows, tests/native) and is not sent to a device.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace dut {

constexpr uint32_t kRowGroupWords = 256;          // 32-bit words per group of 4 rows (T = 2048: 64 blocks x 4 rows)
constexpr uint32_t kRowSegments = 8;               // segments per window (T = 2048: 256 positions, 8 blocks each)
constexpr uint32_t kRowUnitWords = 32;            // 32-bit words per unit: 4 rows of one segment (128 bytes)
constexpr unsigned long long kRowSparse = 1ull << 63;   // flag in a read's bit offset: query-order bits + its CIGAR (below)

// host views of the staged contig (callable_loci.hip fills these from the context's staging arrays).  cl_push_reads
// leaves every read with mapq >= min_mapq and a reference span as a string of pass bits in REFERENCE order -- bit j of
// the string <-> position pos + j: the pass bit of the M/=/X base there, 0 for D, N and bases without a quality byte --,
// word-aligned in `bits` from word off[i] to off[i + 1] (a plain match read: its thresholded quality string as it is; any
// other read: mapped through its CIGAR in the walk that validates the tile, where the operations are in the cache).  Only
// a read whose span dwarfs its query (long N gaps: span > 4 ql + 1024) stays in QUERY order, flagged kRowSparse, with
// its CIGAR in sc[sc_off[i], sc_off[i + 1]): it is walked per window.
struct RowReads {
    const int32_t *pos;
    const uint32_t *end;                          // pos + bam_cigar2rlen
    const uint8_t *mapq;
    const unsigned long long *off;                // n + 1 word offsets into `bits` (| kRowSparse)
    const uint64_t *bits;
    const uint32_t *sc_off, *sc;                  // CIGARs of the sparse reads (n + 1 offsets)
    uint32_t min_mapq;
};

struct RowCur { uint32_t k, k1, x, y, qlen, pos, end; unsigned long long o; bool sparse; };

struct RowScratch { std::vector<uint32_t> rend; };

// n bits of `src` from bit offset o, OR-ed into row r of the window's groups at window-relative position d: up to 64
// bits a step (two destination words: the words of a row are 16 bytes apart, one per block of 32 positions)
// (gw: words per group of the stack `grp` -- a window's, or a segment's with d relative to the segment and a stretch
// that does not leave it)
inline void deposit_bits(const uint64_t *src, unsigned long long o, uint32_t n, uint32_t *grp, uint32_t r, uint32_t d,
                         uint32_t gw = kRowGroupWords)
{
    uint32_t *dst = grp + (size_t)(r >> 2) * gw + (r & 3u);
    while (n) {
        const uint32_t b = d >> 5, lo = d & 31u, take = std::min(64u - lo, n);
        const unsigned long long w = o >> 6;
        const uint32_t s = (uint32_t)(o & 63ull);
        uint64_t v = src[w] >> s;
        if (s + take > 64u) v |= src[w + 1] << (64u - s);
        if (take < 64u) v &= (1ull << take) - 1ull;
        v <<= lo;                                                   // lo + take <= 64
        dst[(size_t)b << 2] |= (uint32_t)v;
        if (lo + take > 32u) dst[((size_t)b + 1) << 2] |= (uint32_t)(v >> 32);
        o += take; d += take; n -= take;
    }
}

// A read's pass bits from query order (qw: bit k <-> base k, ql bases, TWO readable words behind them) to reference
// order: rw[0, ceil(span / 64)) is written whole.  What the column walk visits as (alignment, qpos) with !is_del are the
// bases of M/=/X operations (mod.rs:30-37); a base without a quality byte (k >= ql) never passes.  Written without a
// branch on the kind of operation (insertions and deletions alternate at random in long reads: a mispredicted branch per
// operation cost more than the work): every operation appends `lr` bits to the reference string -- its length if it
// consumes the reference, else 0 -- of which the first `lq` come from the query bits -- if it is a match -- and the rest
// are zeros.  unmatched[0, *n_unmatched): where the inserted / clipped bases lie in the query (the caller's scratch holds
// nops entries), for unmatched_pass_sum.
struct QueryStretch { unsigned long long y, l; };
inline void ref_bits_from_query(const uint64_t *qw, unsigned long long ql, const uint32_t *cig, uint32_t nops, uint64_t *rw,
                                QueryStretch *unmatched, size_t *n_unmatched, unsigned long long *query_len)
{
    uint64_t acc = 0;
    uint32_t accn = 0;
    size_t wout = 0, nu = 0;
    unsigned long long y = 0;
    for (uint32_t j = 0; j < nops; ++j) {
        const uint32_t cw = cig[j], op = cw & 15u;
        const unsigned long long l = cw >> 4;
        const unsigned long long ism = (0x181u >> op) & 1u, radv = (0x18Du >> op) & 1u, qadv = (0x193u >> op) & 1u;
        unmatched[nu].y = y; unmatched[nu].l = l;                   // (kept only for I and S)
        nu += (size_t)(qadv & (ism ^ 1ull));
        const unsigned long long avail = y < ql ? ql - y : 0ull;
        unsigned long long have = std::min(avail, l) & (0ull - ism);   // bits that come from the query
        unsigned long long rem = l & (0ull - radv);                    // bits this operation appends
        unsigned long long src = std::min(y, ql);                      // (clamped: read, then masked away, when have = 0)
        y += l & (0ull - qadv);
        while (rem) {                                               // one trip unless the operation crosses a word
            const unsigned long long take = std::min<unsigned long long>(rem, 64u - accn);
            const unsigned long long tb = std::min(have, take);
            const unsigned long long w = src >> 6;
            const uint32_t s = (uint32_t)(src & 63ull);
            uint64_t v = (qw[w] >> s) | ((qw[w + 1] << 1) << (63u - s));
            v &= tb >= 64ull ? ~0ull : ((1ull << tb) - 1ull);
            acc |= v << accn;
            accn += (uint32_t)take; src += tb; have -= tb; rem -= take;
            if (accn == 64u) { rw[wout++] = acc; acc = 0; accn = 0; }
        }
    }
    if (accn) rw[wout++] = acc;
    *n_unmatched = nu;
    *query_len = y;
}

// The passing quality bytes of a read that are NOT bases of M/=/X operations: inserted and clipped bases (listed by
// ref_bits_from_query), and whatever the quality string holds beyond the CIGAR's query length (contig_profiler.rs:65-70
// sums over the matched bases only: the read's share of summed_baseq is the sum over its whole string minus this).
inline uint64_t unmatched_pass_sum(const uint8_t *q, unsigned long long ql, const QueryStretch *unmatched, size_t n_unmatched,
                                   unsigned long long query_len, uint8_t thr)
{
    uint64_t s = 0;
    if (ql == 0) return 0;
    for (size_t k = 0; k < n_unmatched; ++k) {
        const unsigned long long y = unmatched[k].y, l = unmatched[k].l;
        const unsigned long long cnt = y < ql ? std::min(ql - y, l) : 0ull;
        // the first four bases without a branch (insertions are short), the rest of a long one in a loop
        for (unsigned b = 0; b < 4u; ++b) {
            const uint8_t v = q[std::min(y + b, ql - 1ull)];
            s += (b < cnt && v >= thr) ? v : 0u;
        }
        for (unsigned long long b = 4; b < cnt; ++b) s += q[y + b] >= thr ? q[y + b] : 0u;
    }
    for (unsigned long long b = query_len; b < ql; ++b) s += q[b] >= thr ? q[b] : 0u;
    return s;
}

// a read that covers positions at or after W enters the sweep (reads below min_mapq never do, mod.rs:25; neither do
// reads that left no bits: no quality string)
inline void rows_enter(std::vector<RowCur> &act, const RowReads &H, uint32_t r, uint32_t W)
{
    if (H.mapq[r] < H.min_mapq) return;
    const unsigned long long o0 = H.off[r] & ~kRowSparse, o1 = H.off[r + 1] & ~kRowSparse;
    if (o1 == o0) return;
    RowCur cu;
    cu.pos = (uint32_t)H.pos[r]; cu.end = H.end[r];
    if (cu.end <= W || cu.end <= cu.pos) return;
    cu.o = o0 << 6;
    cu.sparse = (H.off[r] & kRowSparse) != 0ull;
    const unsigned long long nb = (o1 - o0) << 6;                   // bits stored (whole words: the tail is zeros)
    cu.qlen = nb > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nb;
    cu.k = cu.k1 = 0; cu.x = cu.pos; cu.y = 0;
    if (cu.sparse) { cu.k = H.sc_off[r]; cu.k1 = H.sc_off[r + 1]; if (cu.k >= cu.k1) return; }
    act.push_back(cu);
}

// One window [W, W + T): every cursor of `act` (in read order = start order) takes a row and drops the pass bits of its
// M/=/X bases inside the window into out[0, cap_groups * kRowGroupWords) (groups are zeroed as they are opened), then
// moves on; reads that have ended leave the list.  Returns the number of groups, or SIZE_MAX when cap_groups did not
// suffice (the list is then spoilt: the caller restores its copy).
template <uint32_t T>
inline size_t rows_window(std::vector<RowCur> &act, const RowReads &H, uint32_t W, uint32_t *out, size_t cap_groups, RowScratch &sc)
{
    static_assert(T == 64u * 32u, "a group holds 64 blocks of 32 positions");
    const unsigned long long Wend = (unsigned long long)W + T;
    std::vector<uint32_t> &rend = sc.rend;
    uint32_t nr = 0, rot = 0, min_end = 0xFFFFFFFFu;
    size_t ng = 0, keep = 0;
    const size_t na = act.size();
    for (size_t i = 0; i < na; ++i) {
        RowCur cu = act[i];
        if (cu.end <= W) continue;                                  // ended exactly at the seam: nothing here
        // -- the read's row: any row whose last read ended at or before this one's start (looked for from the row
        //    after the last one given out: with reads of one length the rows come free in the order they were taken)
        const uint32_t s = cu.pos > W ? cu.pos - W : 0u;
        const uint32_t e = cu.end < Wend ? cu.end - W : T;
        uint32_t r = nr;
        if (nr && min_end <= s) {                                   // (min_end: a lower bound of every row's end -- when even
            uint32_t mn = 0xFFFFFFFFu;                              //  that lies behind s no row is free: thousands of reads
            for (uint32_t j = 0; j < nr; ++j) {                     //  stacked on one position would else scan all rows each)
                uint32_t q = rot + j;
                if (q >= nr) q -= nr;
                if (rend[q] <= s) { r = q; break; }
                mn = std::min(mn, rend[q]);
            }
            if (r == nr) min_end = mn;                              // every row looked at: exact now
        }
        if (r == nr) {
            if ((nr & 3u) == 0u) {
                if (ng == cap_groups) return SIZE_MAX;
                memset(out + ng * kRowGroupWords, 0, kRowGroupWords * sizeof(uint32_t));
                ++ng;
            }
            if (rend.size() <= nr) rend.resize((size_t)nr + 64);
            ++nr;
        }
        rend[r] = e;                                                // (a row's end only grows: min_end stays a lower bound)
        min_end = std::min(min_end, e);
        rot = r + 1u == nr ? 0u : r + 1u;
        if (!cu.sparse) {
            // -- reference-order bits: the window's stretch of the string, as it is
            const uint32_t sp = cu.pos > W ? cu.pos : W;
            unsigned long long tp = cu.end < Wend ? cu.end : Wend;
            tp = std::min<unsigned long long>(tp, (unsigned long long)cu.pos + cu.qlen);
            if (sp < tp) deposit_bits(H.bits, cu.o + (sp - cu.pos), (uint32_t)(tp - sp), out, r, sp - W);
            if (cu.end > Wend) act[keep++] = cu;
            continue;
        }
        // -- a sparse read: its M/=/X bases inside the window, operation by operation
        while (cu.k < cu.k1 && cu.x < Wend) {
            const uint32_t cw = H.sc[cu.k], op = cw & 15u, l = cw >> 4;
            const uint32_t radv = (0x18Du >> op) & 1u, qadv = (0x193u >> op) & 1u, ism = (0x181u >> op) & 1u;
            const uint32_t xe = cu.x + (radv ? l : 0u);
            if (xe < cu.x) { cu.k = cu.k1; break; }                 // wraps the 32-bit coordinate: flagged kErrRange at push
            if (ism) {
                const uint32_t sp = cu.x > W ? cu.x : W;
                const uint32_t lq = cu.y < cu.qlen ? std::min(cu.qlen - cu.y, l) : 0u;   // bases that have a (possibly zero) bit
                unsigned long long tp = xe < Wend ? xe : Wend;
                tp = std::min<unsigned long long>(tp, (unsigned long long)cu.x + lq);
                if (sp < tp) deposit_bits(H.bits, cu.o + cu.y + (sp - cu.x), (uint32_t)(tp - sp), out, r, sp - W);
            }
            if (xe > Wend) break;                                   // the operation goes on in the next window
            cu.x = xe; cu.y += qadv ? l : 0u; cu.k += 1u;
        }
        if (cu.k < cu.k1 && cu.end > Wend) act[keep++] = cu;
    }
    act.resize(keep);
    return ng;
}

// ---- one row stack per segment (what the device holds) ----
struct SegScratch {
    std::vector<uint32_t> rend[kRowSegments];     // per segment: where the last read of a row ends (window-relative)
    std::vector<uint32_t> stack;                  // the window's stacks while they grow: segment g from unit g * stride on
    uint32_t stride = 0;                          // ... units of room per segment
    uint32_t h[kRowSegments];                     // the last window's heights in units, as stored (equal in the equal-heights form)
    uint32_t most;                                // ... the largest of them
    unsigned long long word;                      // ... and the eight as bytes, segment 0 lowest (0: the equal-heights form)
};

// The heights of a window as its record carries them: eight bytes.  A window in which some segment needs more than 255
// units takes the EQUAL-HEIGHTS form -- every segment `most` units, word 0 --, which is also what `uniform` asks for.
inline unsigned long long rows_heights_word(uint32_t (&h)[kRowSegments], uint32_t &most, bool uniform)
{
    most = 0;
    for (uint32_t s = 0; s < kRowSegments; ++s) most = std::max(most, h[s]);
    if (uniform || most > 255u) { for (uint32_t s = 0; s < kRowSegments; ++s) h[s] = most; return 0ull; }
    unsigned long long w = 0;
    for (uint32_t s = 0; s < kRowSegments; ++s) w |= (unsigned long long)h[s] << (8u * s);
    return w;
}
// units of a window from its record's two fields (rn = the largest height, word as above)
inline uint64_t rows_window_units(uint32_t rn, unsigned long long word)
{
    if (!word) return (uint64_t)rn * kRowSegments;
    uint64_t n = 0;
    for (uint32_t s = 0; s < kRowSegments; ++s) n += (word >> (8u * s)) & 0xFFull;
    return n;
}

// One window [W, W + T) as rows_window, into stacks per segment: every cursor takes a free row in every segment its span
// overlaps -- free: the row's last read ended at or before this one's start, both clipped to the segment; reads arrive
// sorted by start, so a segment has exactly as many rows as its deepest column -- and drops its pass bits there.  Where a
// segment's units lie in the window depends on the heights of the segments in front of it, which are known when the last
// read is placed: the stacks grow side by side in the scratch (a few KB, in cache) and are copied to their places at the
// end.  out[0, units * kRowUnitWords) is written whole; sc.h / sc.most / sc.word describe the window.  Returns the number
// of units, or SIZE_MAX when cap_units did not suffice (the list is then spoilt: the caller restores its copy).
template <uint32_t T>
inline size_t rows_window_segments(std::vector<RowCur> &act, const RowReads &H, uint32_t W, uint32_t *out, size_t cap_units,
                                   SegScratch &sc, bool uniform)
{
    static_assert(T == kRowSegments * 8u * 32u, "a segment holds 8 blocks of 32 positions");
    constexpr uint32_t S = T / kRowSegments;
    const unsigned long long Wend = (unsigned long long)W + T;
    uint32_t nr[kRowSegments] = {}, rot[kRowSegments] = {}, min_end[kRowSegments];
    for (uint32_t g = 0; g < kRowSegments; ++g) min_end[g] = 0xFFFFFFFFu;
    if (sc.stride == 0) { sc.stride = 16; sc.stack.resize((size_t)kRowSegments * sc.stride * kRowUnitWords); }
    uint32_t rows[kRowSegments];                                    // the cursor's row in each segment it overlaps
    // [x0, x1) of the window, bits from bit offset o on: segment by segment into the cursor's rows
    auto put = [&](uint32_t x0, uint32_t x1, unsigned long long o) {
        while (x0 < x1) {
            const uint32_t g = x0 / S, stop = std::min(x1, (g + 1u) * S);
            deposit_bits(H.bits, o, stop - x0, sc.stack.data() + (size_t)g * sc.stride * kRowUnitWords, rows[g], x0 - g * S, kRowUnitWords);
            o += stop - x0; x0 = stop;
        }
    };
    size_t keep = 0;
    const size_t na = act.size();
    for (size_t i = 0; i < na; ++i) {
        RowCur cu = act[i];
        if (cu.end <= W) continue;                                  // ended exactly at the seam: nothing here
        if (cu.pos >= Wend) { act[keep++] = cu; continue; }         // (not of this window yet: no caller enters one so early)
        const uint32_t s = cu.pos > W ? cu.pos - W : 0u;
        const uint32_t e = cu.end < Wend ? cu.end - W : T;
        for (uint32_t g = s / S; g <= (e - 1u) / S; ++g) {
            // (the search of rows_window, per segment)
            const uint32_t ss = std::max(s, g * S), se = std::min(e, (g + 1u) * S);
            std::vector<uint32_t> &rend = sc.rend[g];
            const uint32_t n = nr[g];
            uint32_t r = n;
            if (n && min_end[g] <= ss) {
                uint32_t mn = 0xFFFFFFFFu;
                for (uint32_t j = 0; j < n; ++j) {
                    uint32_t q = rot[g] + j;
                    if (q >= n) q -= n;
                    if (rend[q] <= ss) { r = q; break; }
                    mn = std::min(mn, rend[q]);
                }
                if (r == n) min_end[g] = mn;
            }
            if (r == n) {
                if ((n & 3u) == 0u) {                               // a new unit of this segment: zeroed as it is opened
                    if ((n >> 2) == sc.stride) {                    // no room: twice the room per segment, the stacks moved
                        std::vector<uint32_t> wider((size_t)kRowSegments * sc.stride * 2u * kRowUnitWords);
                        for (uint32_t q = 0; q < kRowSegments; ++q)
                            memcpy(wider.data() + (size_t)q * sc.stride * 2u * kRowUnitWords, sc.stack.data() + (size_t)q * sc.stride * kRowUnitWords,
                                   (size_t)((nr[q] + 3u) >> 2) * kRowUnitWords * sizeof(uint32_t));
                        sc.stack.swap(wider);
                        sc.stride *= 2u;
                    }
                    memset(sc.stack.data() + ((size_t)g * sc.stride + (n >> 2)) * kRowUnitWords, 0, kRowUnitWords * sizeof(uint32_t));
                }
                if (rend.size() <= n) rend.resize((size_t)n + 64);
                nr[g] = n + 1u;
            }
            rend[r] = se;
            min_end[g] = std::min(min_end[g], se);
            rot[g] = r + 1u == nr[g] ? 0u : r + 1u;
            rows[g] = r;
        }
        if (!cu.sparse) {
            // -- reference-order bits: the window's stretch of the string, as it is
            const uint32_t sp = cu.pos > W ? cu.pos : W;
            unsigned long long tp = cu.end < Wend ? cu.end : Wend;
            tp = std::min<unsigned long long>(tp, (unsigned long long)cu.pos + cu.qlen);
            if (sp < tp) put(sp - W, (uint32_t)(tp - W), cu.o + (sp - cu.pos));
            if (cu.end > Wend) act[keep++] = cu;
            continue;
        }
        // -- a sparse read: its M/=/X bases inside the window, operation by operation (as rows_window)
        while (cu.k < cu.k1 && cu.x < Wend) {
            const uint32_t cw = H.sc[cu.k], op = cw & 15u, l = cw >> 4;
            const uint32_t radv = (0x18Du >> op) & 1u, qadv = (0x193u >> op) & 1u, ism = (0x181u >> op) & 1u;
            const uint32_t xe = cu.x + (radv ? l : 0u);
            if (xe < cu.x) { cu.k = cu.k1; break; }                 // wraps the 32-bit coordinate: flagged kErrRange at push
            if (ism) {
                const uint32_t sp = cu.x > W ? cu.x : W;
                const uint32_t lq = cu.y < cu.qlen ? std::min(cu.qlen - cu.y, l) : 0u;
                unsigned long long tp = xe < Wend ? xe : Wend;
                tp = std::min<unsigned long long>(tp, (unsigned long long)cu.x + lq);
                if (sp < tp) put(sp - W, (uint32_t)(tp - W), cu.o + cu.y + (sp - cu.x));
            }
            if (xe > Wend) break;                                   // the operation goes on in the next window
            cu.x = xe; cu.y += qadv ? l : 0u; cu.k += 1u;
        }
        if (cu.k < cu.k1 && cu.end > Wend) act[keep++] = cu;
    }
    act.resize(keep);
    // the heights, and the stacks to their places (the equal-heights form: zeros above a lower segment's own units)
    uint32_t own[kRowSegments];
    for (uint32_t g = 0; g < kRowSegments; ++g) sc.h[g] = own[g] = (nr[g] + 3u) >> 2;
    sc.word = rows_heights_word(sc.h, sc.most, uniform);
    size_t units = 0;
    for (uint32_t g = 0; g < kRowSegments; ++g) units += sc.h[g];
    if (units > cap_units) return SIZE_MAX;
    for (uint32_t g = 0; g < kRowSegments; ++g) {
        if (own[g]) memcpy(out, sc.stack.data() + (size_t)g * sc.stride * kRowUnitWords, (size_t)own[g] * kRowUnitWords * sizeof(uint32_t));
        if (sc.h[g] > own[g]) memset(out + (size_t)own[g] * kRowUnitWords, 0, (size_t)(sc.h[g] - own[g]) * kRowUnitWords * sizeof(uint32_t));
        out += (size_t)sc.h[g] * kRowUnitWords;
    }
    return units;
}

} // namespace dut
