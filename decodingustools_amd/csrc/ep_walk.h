// ep_walk.h -- the walk of one read for the error profile (cl_site_error_profile, dut_error_profile_measure): which of its
// bases are aligned to which reference position, and which insertions and deletions it carries, each with the query index
// the table is keyed by.  HIP-free: the kernel k_site_error_profile (site_errors.hip.h), the host route
// dut_error_profile_measure (variants.cpp) and the sanitizer program (tests/native/ep_walk_host.cpp) compile this one text.
//
// The rule.  The read's CIGAR is walked from pos with x, the reference position reached (64 bits wide: a read may run
// past 2^32), and y, the stored bases consumed (M I S = X consume them; D N H P do not).  L is the read's stored base
// count.  Over the sub-range [lo, hi), 0-based half open:
//   M = X of length l   base(p, q) for every position p of [x, x + l) cut with [lo, hi) whose query index
//                       q = y + (p - x) is < L;  x += l, y += l
//   I of length l >= 1  ins(x - 1, y - 1, l) when it stands directly behind an M/=/X operation of at least one base, that
//                       operation's last position x - 1 (the anchor) lies in [lo, hi), and the anchor base and all l
//                       inserted bases exist: y + l <= L;  y += l
//   D of length l >= 1  del(x, y - 1, l) when its first deleted position x lies in [lo, hi) and its carrier, query index
//                       y - 1, exists: 1 <= y <= L;  x += l
//   N                   x += l
//   S                   y += l
//   H P                 take no part
// An event belongs to the one sub-range that holds its anchor or first position, whichever windows the operation
// crosses: walks of one read over the pieces of a range report each base and each event once.
//
// The bases of an M/=/X operation are dealt to n_lanes callers of the same read: caller `lane` takes every n_lanes-th
// position from its own, and lane 0 alone reports the events.  (lane, n_lanes) = (0, 1): one caller sees everything.
// Every caller runs the CIGAR loop and the loop over a run the same number of times, but base() itself is called under a
// condition: only by the callers that have a position in that step (the last step of a run is short), and ins() and del()
// only by lane 0.  A sink on a wave may therefore use only cross-lane operations that act on the lanes active at the call
// (a ballot, a read of the first active lane); a shuffle over the whole wave or a barrier inside a sink is wrong.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)               /* (also a host source that hipcc compiles without the HIP runtime's headers) */
#define EP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define EP_HD inline
#endif

#define CL_EP_WALK_MAX_CYCLES 256       /* CL_EP_MAX_CYCLES of callable_loci.h */

namespace dut {

// distance of query index q < L from the 5' end of the molecule as it was sequenced, and from its 3' end
EP_HD uint32_t ep_d5(uint32_t q, uint32_t L, uint32_t rev) { return rev ? L - 1u - q : q; }
EP_HD uint32_t ep_d3(uint32_t q, uint32_t L, uint32_t rev) { return rev ? q : L - 1u - q; }

// 4 * from + to in A C G T of an aligned base with 4-bit code c over the reference byte ref, complemented for a reverse
// read; 16: not comparable (a code that is not one of 1 2 4 8, a reference byte that is not one of ACGT in either case)
EP_HD uint32_t ep_cell(uint32_t c, uint32_t ref, uint32_t rev)
{
    const uint32_t R = ref & ~32u;
    const uint32_t f = R == 'A' ? 0u : R == 'C' ? 1u : R == 'G' ? 2u : R == 'T' ? 3u : 4u;
    const uint32_t t = c == 1u ? 0u : c == 2u ? 1u : c == 4u ? 2u : c == 8u ? 3u : 4u;
    if (f > 3u || t > 3u) return 16u;
    return rev ? 4u * (3u - f) + (3u - t) : 4u * f + t;
}

// cigar: n_ops BAM CIGAR words (length << 4 | op) of a read at pos with L stored bases; hi - lo + n_lanes <= 2^32
template <class Sink>
EP_HD void ep_walk_read(uint32_t pos, const uint32_t *cigar, uint32_t n_ops, uint32_t L, uint32_t lo, uint32_t hi, uint32_t lane,
                        uint32_t n_lanes, Sink &&sink)
{
    unsigned long long x = pos, y = 0;
    bool behind_match = false;                                      // the operation in front was an M/=/X of at least one base
    // (at hi an I directly behind a match still has its anchor inside; beyond it nothing has an effect)
    for (uint32_t k = 0; k < n_ops && (x < hi || (x == hi && behind_match)); ++k) {
        const uint32_t c = cigar[k];
        const uint32_t op = c & 15u;
        const unsigned long long l = c >> 4;
        if (op == 0u || op == 7u || op == 8u) {
            if (x < hi && y < L) {                                  // (x < hi <= 2^32 - 1 and y < L <= 2^32 - 1: 32 bits hold the run)
                const uint32_t x32 = (uint32_t)x, y32 = (uint32_t)y;
                const uint32_t p0 = x32 > lo ? x32 : lo;
                uint32_t p1 = x + l < hi ? (uint32_t)(x + l) : hi;
                if (p1 - x32 > L - y32) p1 = x32 + (L - y32);
                const uint32_t n = p1 > p0 ? p1 - p0 : 0u, q0 = y32 + (p0 - x32);
                for (uint32_t i = 0; i < n; i += n_lanes) {         // (hi - lo + n_lanes <= 2^32: i does not wrap)
                    const uint32_t j = i + lane;
                    if (j < n) sink.base(p0 + j, q0 + j);
                }
            }
            x += l; y += l;
            behind_match = l != 0ull;
            continue;
        }
        if (op == 1u) {
            if (behind_match && l && x - 1ull >= lo && x - 1ull < hi && y + l <= L && lane == 0u) sink.ins((uint32_t)(x - 1ull), (uint32_t)(y - 1ull), (uint32_t)l);
            y += l;
        } else if (op == 2u) {
            if (l && x >= lo && x < hi && y >= 1ull && y <= L && lane == 0u) sink.del((uint32_t)x, (uint32_t)(y - 1ull), (uint32_t)l);
            x += l;
        } else if (op == 3u) {
            x += l;
        } else if (op == 4u) {
            y += l;
        }
        behind_match = false;
    }
}

} // namespace dut
