// site_pass_bits.h -- the pass bits of a site tile's attachment (cl_site_attach_quals), built on the host: one bit per
// base, (qual >= min_base_quality), addressed by the base index of seq4 (seq_off numbering).  The quality values are
// numbered by qual_off, which need not agree: base i of read r has the value qual[qual_off[r] + i] when
// i < qual_off[r + 1] - qual_off[r], otherwise none.  A base without a value passes, and so does 0xFF.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "qual_pack.h"

namespace dut {

// Words [w0, w1) of the bit array into out[0, w1 - w0): bit i of word w <-> base 64 w + i.  Bits that belong to no read
// are zero.  Each call is independent of every other, so the words of a tile can be produced in pieces, in any order.
inline void site_pass_words(uint64_t n_reads, const uint64_t *seq_off, const uint64_t *qual_off, const uint8_t *qual,
                            uint8_t thr, uint64_t w0, uint64_t w1, uint64_t *out)
{
    if (w0 >= w1) return;
    memset(out, 0, (size_t)(w1 - w0) * 8);
    if (!n_reads) return;
    const uint64_t b0 = w0 * 64, b1 = w1 * 64;
    // the first read whose bases end beyond b0
    uint64_t r = (uint64_t)(std::upper_bound(seq_off + 1, seq_off + n_reads + 1, b0) - (seq_off + 1));
    std::vector<uint64_t> t;
    for (; r < n_reads && seq_off[r] < b1; ++r) {
        const uint64_t len = seq_off[r + 1] - seq_off[r];
        if (!len) continue;
        const uint64_t nq = std::min<uint64_t>(len, qual_off[r + 1] - qual_off[r]);
        const uint64_t nw = (len + 63) / 64;
        t.assign(nw, 0);
        if (nq) (void)qual_pass_read(qual + qual_off[r], nq, thr, t.data());      // zeros above bit nq
        for (uint64_t i = nq; i < len;) {                                          // no quality value: passes
            const uint64_t lo = i & 63, n = std::min<uint64_t>(64 - lo, len - i);
            t[i >> 6] |= (n == 64 ? ~0ull : ((1ull << n) - 1ull) << lo);
            i += n;
        }
        const uint64_t d = seq_off[r], sh = d & 63;
        for (uint64_t j = 0; j < nw; ++j) {
            const uint64_t W = (d >> 6) + j, v = t[j];
            if (W >= w0 && W < w1) out[W - w0] |= v << sh;
            if (sh && W + 1 >= w0 && W + 1 < w1) out[W + 1 - w0] |= v >> (64 - sh);
        }
    }
}

} // namespace dut
