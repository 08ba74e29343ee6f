// engine_limits.h -- the constants that the kernels of the callable-loci engine and the host walk over a tile of reads
// (tile_walk.h) both need (plain C++, no HIP): kernels.hip.h includes this, and so does everything that includes it.
#pragma once
#include <stdint.h>

namespace clk {

constexpr uint32_t kLongOps = 64;    // reads with more CIGAR ops get a checkpoint (reference, query position) before
                                     // every 64th op (op numbering of the contig's CIGAR array): host side only
constexpr uint32_t kWideSpan = 16384; // reads spanning more reference than this are "wide": looked up per window
                                      // in their own list instead of widening every window's candidate range
// most positions one head of k_pileup_rows spans (pileup_rows.hip.h): a longer span is cut into several heads
constexpr uint32_t kHeadSpanMax = 0x7FFFFFFFu;

enum : uint32_t { kErrCigar = 1u, kErrRange = 2u, kNeedDeep = 4u, kNeedWide8 = 8u };

} // namespace clk
