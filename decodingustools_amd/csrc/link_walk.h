// link_walk.h -- the walk of one read over an anchor site and its partners (cl_site_link_counts, dut_link_measure): what
// the read observes at each of up to 16 ascending positions, so that the counts of a pair of sites can be taken per read
// instead of per column.  HIP-free: the kernel k_site_links (site_links.hip.h), the host route dut_link_measure
// (variants.cpp) and the sanitizer program (tests/native/link_walk_host.cpp) compile this one text.
//
// The pair set.  sites[0..n) are 0-based positions, strictly ascending.  For anchor i the partners are j = i + 1, i + 2, ...
// while j <= i + K and sites[j] - sites[i] <= D (link_partner_count); first[i] is the running sum of those counts, pair
// first[i] + (j - i - 1) is (i, j), first[n] the number of pairs.
//
// The observation of a read at a position p.  The CIGAR is walked from pos with x, the reference position reached (64
// bits wide: a read may run past 2^32), and y, the stored bases consumed (M I S = X consume them; D N H P do not).  L is
// the read's stored base count.
//   p in an M = X operation   q = y + (p - x).  q < L and passes(q): the class of code(q) -- 1 -> A (0), 2 -> C (1),
//                             4 -> G (2), 8 -> T (3), every other code -> other (5).  Otherwise none.
//   p in a D operation        its carrier is query index y - 1.  1 <= y <= L and passes(y - 1): del (4).  Otherwise none.
//   p in an N, outside the span   none
// These are the conventions of the dense scans for bases (cl_site_scan_counts) and for deletions (cl_site_scan_dels).
// `source` answers code(q) and passes(q) for q < L: the device reads seq4 and the pass bits, the host plain arrays.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)               /* (also a host source that hipcc compiles without the HIP runtime's headers) */
#define LINK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LINK_HD inline
#endif

#define CL_LINK_WALK_CLASSES      6     /* CL_LINK_CLASSES of callable_loci.h: A C G T del other */
#define CL_LINK_WALK_MAX_PARTNERS 15    /* CL_LINK_MAX_PARTNERS */
#define LINK_DEL   4u
#define LINK_OTHER 5u
#define LINK_NONE  15u

namespace dut {

// the partners of anchor i: the sites behind it, at most K of them, no further than D positions away
LINK_HD uint32_t link_partner_count(const uint32_t *sites, uint64_t n, uint64_t i, uint32_t D, uint32_t K)
{
    uint32_t k = 0;
    while (k < K && i + 1u + k < n && sites[i + 1u + k] - sites[i] <= D) ++k;
    return k;
}

// the class of a 4-bit base code
LINK_HD uint32_t link_class(uint32_t code)
{
    return code == 1u ? 0u : code == 2u ? 1u : code == 4u ? 2u : code == 8u ? 3u : LINK_OTHER;
}

// observation k of a packed word, and the word with observation k set
LINK_HD uint32_t link_obs(uint64_t packed, uint32_t k) { return (uint32_t)(packed >> (4u * k)) & 15u; }
LINK_HD uint64_t link_with(uint64_t packed, uint32_t k, uint32_t c) { return (packed & ~(15ull << (4u * k))) | ((uint64_t)c << (4u * k)); }

// cigar: n_ops BAM CIGAR words (length << 4 | op) of a read at pos with L stored bases; sites: m <= 16 strictly ascending
// positions, sites[0] >= pos.  One pass over the CIGAR, which ends behind the last site or the end of the read.  Returns
// the 16 observations as nibbles, site k in bits [4k, 4k + 4); LINK_NONE where there is none, and for k >= m.
template <class Source>
LINK_HD uint64_t link_observe_read(uint32_t pos, const uint32_t *cigar, uint32_t n_ops, uint32_t L, const uint32_t *sites, uint32_t m, Source &&source)
{
    uint64_t packed = ~0ull;
    unsigned long long x = pos, y = 0;
    uint32_t j = 0;
    for (uint32_t k = 0; k < n_ops && j < m; ++k) {
        const uint32_t c = cigar[k];
        const uint32_t op = c & 15u;
        const unsigned long long l = c >> 4;
        if (op == 0u || op == 7u || op == 8u) {
            for (; j < m && sites[j] < x + l; ++j) {                         // (sites[j] >= x: every site below x is behind j)
                const unsigned long long q = y + (sites[j] - x);
                if (q < L && source.passes((uint32_t)q)) packed = link_with(packed, j, link_class(source.code((uint32_t)q)));
            }
            x += l; y += l;
        } else if (op == 2u) {
            if (j < m && sites[j] < x + l) {                                 // (the carrier is asked for only when a site lies inside)
                const bool carried = y >= 1ull && y <= L && source.passes((uint32_t)(y - 1ull));
                for (; j < m && sites[j] < x + l; ++j)
                    if (carried) packed = link_with(packed, j, LINK_DEL);
            }
            x += l;
        } else if (op == 3u) {
            while (j < m && sites[j] < x + l) ++j;
            x += l;
        } else if (op == 1u || op == 4u) {
            y += l;
        }
    }
    return packed;
}

} // namespace dut
