// target_pieces.h -- the piece list of cl_contig_target_order (include/callable_loci.h), plain C++ without HIP, so that a
// stand-alone CPU program can run it under the sanitizers (tests/native/target_pieces_host.cpp).
//
// Every target is clipped as cl_contig_targets clips it (e = min(end, extent), s = min(start, e)); a target that is left
// non-empty is cut at the engine's windows of 2048 positions into pieces (target, a, b): the positions
// [w * 2048 + a, w * 2048 + b) of window w, 0 <= a < b <= 2048.  The pieces are counting-sorted by window (within a
// window in the order of the targets), eight bytes each, with first[n_win + 1]: window w holds pieces
// [first[w], first[w + 1]).  The count comes first and on its own, so that a caller can refuse a list beyond its cap
// before a byte of it is allocated.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace clk {

constexpr uint32_t kPieceWindow = 2048;                    // (CL_WINDOW)

struct TargetPiece {
    uint32_t target;
    uint32_t ab;                                           // a | b << 16
};
static_assert(sizeof(TargetPiece) == 8, "eight bytes a piece");

struct ClippedTarget { uint32_t s, e; };
inline ClippedTarget clip_target(uint32_t start, uint32_t end, uint32_t extent)
{
    const uint32_t e = end < extent ? end : extent;
    return ClippedTarget{start < e ? start : e, e};
}

// How many pieces the targets have (nothing is allocated).
inline uint64_t target_piece_count(const uint32_t *starts, const uint32_t *ends, size_t n, uint32_t extent)
{
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        const ClippedTarget t = clip_target(starts[i], ends[i], extent);
        if (t.s < t.e) total += (uint64_t)((t.e - 1u) / kPieceWindow - t.s / kPieceWindow) + 1u;
    }
    return total;
}

// The pieces and the windows' ranges of them; n_win * 2048 >= extent.  Returns false, with nothing usable in the two
// vectors, where a piece would lie beyond window n_win - 1 (an extent the windows do not cover) or the pieces do not
// fit 32 bits.  Allocations throw std::bad_alloc as a vector does.
inline bool target_pieces_build(const uint32_t *starts, const uint32_t *ends, size_t n, uint32_t extent, uint32_t n_win,
                                std::vector<TargetPiece> &pieces, std::vector<uint32_t> &first)
{
    pieces.clear();
    first.assign((size_t)n_win + 1u, 0u);
    if ((uint64_t)n_win * kPieceWindow < extent || n > 0xFFFFFFFFull) return false;
    const uint64_t total = target_piece_count(starts, ends, n, extent);
    if (total > 0xFFFFFFFFull) return false;
    // the windows' counts (at first[w + 1]), then their running sums
    for (size_t i = 0; i < n; ++i) {
        const ClippedTarget t = clip_target(starts[i], ends[i], extent);
        if (t.s >= t.e) continue;
        for (uint32_t w = t.s / kPieceWindow, wl = (t.e - 1u) / kPieceWindow; w <= wl; ++w) ++first[(size_t)w + 1u];
    }
    for (uint32_t w = 0; w < n_win; ++w) first[(size_t)w + 1u] += first[w];
    pieces.resize((size_t)total);
    std::vector<uint32_t> at(first.begin(), first.end() - 1);
    for (size_t i = 0; i < n; ++i) {
        const ClippedTarget t = clip_target(starts[i], ends[i], extent);
        if (t.s >= t.e) continue;
        for (uint32_t w = t.s / kPieceWindow, wl = (t.e - 1u) / kPieceWindow; w <= wl; ++w) {
            const uint64_t W = (uint64_t)w * kPieceWindow;
            const uint32_t a = t.s > W ? (uint32_t)(t.s - W) : 0u;
            const uint32_t b = t.e - W < kPieceWindow ? (uint32_t)(t.e - W) : kPieceWindow;
            pieces[at[w]++] = TargetPiece{(uint32_t)i, a | (b << 16)};
        }
    }
    return true;
}

} // namespace clk
