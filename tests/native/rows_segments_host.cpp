// rows_segments_host.cpp -- the two row builders of pass_rows.h side by side, as a program of its own for the sanitizers
// (plain C++, no device, nothing else of the library):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I decodingustools_amd/csrc
//       tests/native/rows_segments_host.cpp -o rows_segments_host && ./rows_segments_host
// rows_window_segments (a row stack per segment of 256 positions: what the device holds) is held against rows_window
// (one stack per window) on hand-made and random windows, every buffer of exactly the size the builder is told:
//   * the column sum of every position is the same in both layouts
//   * without sparse reads a segment is as high as its deepest column asks for, ceil(depth / 4) units
//   * no segment is higher than the window's one stack, and the units beyond a capacity are never touched
//   * the equal-heights form (asked for, or forced by a segment of more than 255 units) holds the same sums
//   * both builders leave the same cursors for the next window
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "pass_rows.h"

namespace {

constexpr uint32_t T = 2048, S = 256, NW = 4;

struct Reads {
    std::vector<int32_t> pos; std::vector<uint32_t> end; std::vector<uint8_t> mapq;
    std::vector<unsigned long long> off{0ull}; std::vector<uint64_t> bits;
    std::vector<uint32_t> sc_off{0u}, sc;
    bool any_sparse = false;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    uint64_t rnd(uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; }
    // a read [p, p + span) with random pass bits in reference order
    void plain(uint32_t p, uint32_t span, uint8_t mq = 60)
    {
        pos.push_back((int32_t)p); end.push_back(p + span); mapq.push_back(mq);
        for (uint32_t k = 0; k < span; k += 64) {
            uint64_t w = rnd(1ull << 62) | (rnd(4) << 62);
            if (span - k < 64) w &= (1ull << (span - k)) - 1ull;
            bits.push_back(w);
        }
        off.push_back(bits.size()); sc_off.push_back((uint32_t)sc.size());
    }
    // a gapped read: a M, gap N, b M, its bits in query order
    void sparse(uint32_t p, uint32_t a, uint32_t gap, uint32_t b)
    {
        pos.push_back((int32_t)p); end.push_back(p + a + gap + b); mapq.push_back(60);
        off.back() |= dut::kRowSparse;
        for (uint32_t k = 0; k < a + b; k += 64) {
            uint64_t w = rnd(1ull << 62) | (rnd(4) << 62);
            if (a + b - k < 64) w &= (1ull << (a + b - k)) - 1ull;
            bits.push_back(w);
        }
        sc.push_back(a << 4); sc.push_back((gap << 4) | 3u); sc.push_back(b << 4);
        off.push_back(bits.size()); sc_off.push_back((uint32_t)sc.size());
        any_sparse = true;
    }
};

int check(Reads &R, const char *what)
{
    int bad = 0;
    R.bits.push_back(0ull); R.bits.push_back(0ull);             // the words deposit_bits may read behind the last string
    if (R.sc.empty()) R.sc.push_back(0u);
    dut::RowReads H;
    H.pos = R.pos.data(); H.end = R.end.data(); H.mapq = R.mapq.data(); H.off = R.off.data(); H.bits = R.bits.data();
    H.sc_off = R.sc_off.data(); H.sc = R.sc.data(); H.min_mapq = 10;
    const uint32_t n = (uint32_t)R.pos.size();
    // the deepest column per segment among the reads that get a row
    std::vector<uint32_t> depth(NW * T + 1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (R.mapq[i] < 10 || R.end[i] <= (uint32_t)R.pos[i]) continue;
        for (uint32_t x = (uint32_t)R.pos[i]; x < R.end[i] && x < NW * T; ++x) depth[x] += 1;
    }
    for (int uniform = 0; uniform < 2; ++uniform) {
        std::vector<dut::RowCur> act, act_s;
        dut::RowScratch scr;
        dut::SegScratch seg;
        uint32_t next = 0;
        for (uint32_t w = 0; w < NW; ++w) {
            const uint32_t W = w * T;
            while (next < n && (uint32_t)R.pos[next] < W + T) { dut::rows_enter(act, H, next, W); dut::rows_enter(act_s, H, next, W); ++next; }
            size_t cap = 2, ng;
            const std::vector<dut::RowCur> start = act;
            std::vector<uint32_t> buf;
            for (;;) { buf.assign(cap * dut::kRowGroupWords, 0xFFFFFFFFu); act = start; ng = dut::rows_window<T>(act, H, W, buf.data(), cap, scr); if (ng != SIZE_MAX) break; cap *= 2; }
            // the segments: first the size is asked for with no room at all, then exactly that much is given
            const std::vector<dut::RowCur> start_s = act_s;
            uint32_t none[1] = {0xFFFFFFFFu};
            size_t units = dut::rows_window_segments<T>(act_s, H, W, none, 0, seg, uniform != 0);
            size_t total = 0;
            for (uint32_t g = 0; g < dut::kRowSegments; ++g) total += seg.h[g];
            if (total == 0) { if (units != 0) ++bad; }
            else {
                if (units != SIZE_MAX) ++bad;
                act_s = start_s;
                std::vector<uint32_t> one_short((total - 1) * dut::kRowUnitWords, 0xFFFFFFFFu);
                if (dut::rows_window_segments<T>(act_s, H, W, one_short.data(), total - 1, seg, uniform != 0) != SIZE_MAX) ++bad;
                for (uint32_t v : one_short) if (v != 0xFFFFFFFFu) { ++bad; break; }
                act_s = start_s;
            }
            std::vector<uint32_t> ub(total * dut::kRowUnitWords, 0xFFFFFFFFu);
            units = dut::rows_window_segments<T>(act_s, H, W, ub.data(), total, seg, uniform != 0);
            if (units != total || dut::rows_window_units(seg.most, seg.word) != total) { ++bad; continue; }
            // the record's two fields say what the scratch says
            uint32_t most = 0;
            for (uint32_t g = 0; g < dut::kRowSegments; ++g) {
                most = seg.h[g] > most ? seg.h[g] : most;
                if (seg.word && ((seg.word >> (8 * g)) & 0xFFu) != seg.h[g]) ++bad;
                if (!seg.word && seg.h[g] != seg.most) ++bad;
            }
            if (most != seg.most || most > ng || (uniform && seg.word)) ++bad;
            if ((seg.word == 0) != (uniform || most > 255u || most == 0)) ++bad;
            // heights by the deepest column
            uint32_t deepest_all = 0;
            for (uint32_t g = 0; g < dut::kRowSegments; ++g) {
                uint32_t deepest = 0;
                for (uint32_t x = 0; x < S; ++x) deepest = depth[W + g * S + x] > deepest ? depth[W + g * S + x] : deepest;
                deepest_all = deepest > deepest_all ? deepest : deepest_all;
                if (!R.any_sparse && seg.word && seg.h[g] != (deepest + 3) / 4) ++bad;
            }
            if (!R.any_sparse && most != (deepest_all + 3) / 4) ++bad;
            // column sums
            size_t first = 0;
            for (uint32_t g = 0; g < dut::kRowSegments; ++g) {
                const uint32_t *u = ub.data() + first * dut::kRowUnitWords;
                for (uint32_t x = g * S; x < (g + 1) * S; ++x) {
                    uint32_t a = 0, b = 0;
                    for (size_t r = 0; r < 4 * ng; ++r) a += (buf[(r >> 2) * dut::kRowGroupWords + ((x >> 5) << 2) + (r & 3)] >> (x & 31u)) & 1u;
                    for (size_t r = 0; r < 4 * (size_t)seg.h[g]; ++r) b += (u[(r >> 2) * dut::kRowUnitWords + (((x >> 5) & 7u) << 2) + (r & 3)] >> (x & 31u)) & 1u;
                    if (a != b) ++bad;
                }
                first += seg.h[g];
            }
            // the cursors that go on
            if (act.size() != act_s.size()) ++bad;
            else for (size_t i = 0; i < act.size(); ++i) {
                const dut::RowCur &p = act[i], &q = act_s[i];
                if (p.k != q.k || p.x != q.x || p.y != q.y || p.pos != q.pos || p.end != q.end || p.o != q.o) ++bad;
            }
        }
    }
    printf("%-28s %d mismatch(es)\n", what, bad);
    return bad;
}

} // namespace

int main()
{
    int bad = 0;
    { Reads R; for (int i = 0; i < 9; ++i) R.plain(10 + i, 100); bad += check(R, "segment 0 only"); }
    { Reads R; for (int i = 0; i < 5; ++i) R.plain(T + 7 * S + 3 * i, 60); bad += check(R, "last segment, empty window"); }
    {   // ends exactly on a segment seam and on a window seam, starts exactly on them, and reads across both
        Reads R;
        R.plain(S - 100, 100); R.plain(S - 50, 100); R.plain(S, 40); R.plain(T - 150, 150); R.plain(T - 70, 150); R.plain(T, 30);
        R.plain(T + 2 * S - 1, 2);
        bad += check(R, "seams");
    }
    {   // 4 k and 4 k + 1 rows in neighbouring segments
        Reads R;
        for (int i = 0; i < 8; ++i) R.plain(2 * S + 10, 100);
        for (int i = 0; i < 9; ++i) R.plain(3 * S + 10, 100);
        bad += check(R, "8 and 9 rows");
    }
    {   // 1020 reads on one stretch: 255 units, still a byte; 1021: the equal-heights form
        Reads R; for (int i = 0; i < 1020; ++i) R.plain(5 * S + 20, 64); R.plain(6 * S + 1, 10); bad += check(R, "255 units");
        Reads Q; for (int i = 0; i < 1021; ++i) Q.plain(5 * S + 20, 64); Q.plain(6 * S + 1, 10); bad += check(Q, "256 units");
    }
    {   // a long read over three windows, low-mapq reads that get no row, a gapped read
        Reads R;
        R.plain(100, 3 * T); R.plain(120, 300, 3); R.plain(400, 700); R.sparse(500, 90, 3000, 120); R.plain(900, 50); R.sparse(T + 10, 40, 5000, 40);
        bad += check(R, "long and gapped reads");
    }
    for (int round = 0; round < 40; ++round) {
        Reads R;
        R.state += (uint64_t)round * 0x2545F4914F6CDD1Dull;
        const uint32_t n = 40 + (uint32_t)R.rnd(400), step = 1 + (uint32_t)R.rnd(60);
        uint32_t p = (uint32_t)R.rnd(3000);
        for (uint32_t i = 0; i < n; ++i) {
            p += (uint32_t)R.rnd(step);
            const uint64_t kind = R.rnd(12);
            if (kind == 0 && round % 2) R.sparse(p, 1 + (uint32_t)R.rnd(200), 1500 + (uint32_t)R.rnd(3000), 1 + (uint32_t)R.rnd(200));
            else if (kind == 1) R.plain(p, 1 + (uint32_t)R.rnd(5000));
            else R.plain(p, 1 + (uint32_t)R.rnd(300), (uint8_t)(R.rnd(6) == 0 ? 3 : 60));
        }
        char name[32];
        snprintf(name, sizeof(name), "random %d%s", round, R.any_sparse ? " (gapped)" : "");
        bad += check(R, name);
    }
    printf("rows_segments_host: %d mismatch(es)\n", bad);
    return bad ? 1 : 0;
}
