// str_walk.h -- the walk of one read over one short-tandem-repeat locus (cl_site_str_lengths, dut_str_measure): how many
// bases the read holds between the locus's two flanks, whatever anchors its aligner chose for the gaps inside.  HIP-free:
// the kernel k_site_str_lengths (site_str.hip.h), the host route dut_str_measure (variants.cpp) and the sanitizer program
// (tests/native/str_walk_host.cpp) compile this one text.
//
// The rule.  A locus is [s, e) on the contig, 0-based half open, with a flank F >= 1.  The read's CIGAR is walked with x,
// the reference position reached, from pos:
//   M = X of length l   qlen    += |[x, x + l) cut with [s, e)|
//                       m_left  += |[x, x + l) cut with [s - F, s)|
//                       m_right += |[x, x + l) cut with [e, e + F)|;   x += l
//   I of length l at x  s <= x <= e: qlen += l (both borders belong to the locus);  s - F < x < s: i_left += l;
//                       e < x < e + F: i_right += l;  elsewhere nothing
//   D                   x += l, nothing else (the deleted positions are simply not in qlen)
//   N                   x += l; skipped = true if it overlaps [s, e)
//   S H P               take no part
// The read is spanning iff m_left == F, m_right == F, i_left == 0, i_right == 0 and not skipped: both flanks matched base
// by base with no gap inside them, which implies pos <= s - F and pos + span >= e + F.  A locus with s < F has no spanning
// read (m_left <= s < F; s - F is never formed).  delta = qlen - (e - s).  Stored bases take no part.
// x is 64 bits wide: a read may run past 2^32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)               /* (also a host source that hipcc compiles without the HIP runtime's headers) */
#define STR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define STR_HD inline
#endif

#define CL_STR_WALK_BINS 128            /* CL_STR_BINS of callable_loci.h */

namespace dut {

struct StrMeasure {
    bool spanning;
    long long delta;                    // meaningful when spanning
};

// |[a0, a1) cut with [b0, b1)|
STR_HD unsigned long long str_cut(unsigned long long a0, unsigned long long a1, unsigned long long b0, unsigned long long b1)
{
    const unsigned long long lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
    return hi > lo ? hi - lo : 0ull;
}

// cigar: n_ops BAM CIGAR words (length << 4 | op) of a read at pos; 0 < e - s, F >= 1
STR_HD StrMeasure str_measure_read(uint32_t pos, const uint32_t *cigar, uint32_t n_ops, uint32_t s, uint32_t e, uint32_t F)
{
    const unsigned long long s64 = s, e64 = e, rf = e64 + F;         // the right flank is [e, rf)
    const unsigned long long lf = s >= F ? s64 - F : 0ull;           // the left flank is [lf, s): shorter than F when s < F
    unsigned long long x = pos, qlen = 0, m_left = 0, m_right = 0, gaps = 0;
    bool skipped = false;
    for (uint32_t k = 0; k < n_ops && x < rf; ++k) {                 // (at and beyond e + F no operation has an effect)
        const uint32_t c = cigar[k];
        const uint32_t op = c & 15u;
        const unsigned long long l = c >> 4;
        if (op == 0u || op == 7u || op == 8u) {
            qlen += str_cut(x, x + l, s64, e64);
            m_left += str_cut(x, x + l, lf, s64);
            m_right += str_cut(x, x + l, e64, rf);
            x += l;
        } else if (op == 1u) {
            if (x >= s64 && x <= e64) qlen += l;
            else if ((x > lf && x < s64) || (x > e64 && x < rf)) gaps += l;     // i_left, i_right: only their being 0 is asked
        } else if (op == 2u) {
            x += l;
        } else if (op == 3u) {
            if (l && x < e64 && x + l > s64) skipped = true;
            x += l;
        }
    }
    StrMeasure m;
    m.spanning = m_left == F && m_right == F && gaps == 0 && !skipped;
    m.delta = (long long)qlen - (long long)(e64 - s64);
    return m;
}

// the bin of a spanning read's delta: delta + 63 for -63 <= delta <= 63, else the last one ("other")
STR_HD uint32_t str_bin(long long delta)
{
    return (delta >= -63 && delta <= 63) ? (uint32_t)(delta + 63) : (uint32_t)(CL_STR_WALK_BINS - 1);
}

} // namespace dut
