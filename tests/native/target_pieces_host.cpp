// target_pieces_host.cpp -- the piece list of cl_contig_target_order (decodingustools_amd/csrc/target_pieces.h) under the
// sanitizers, no device: seeded target sets against a brute-force cut, position by position.  Built and run by
// tests/test_target_order_host.py (g++ -fsanitize=address,undefined); exits 0 and prints "ok <cases>" when every check holds.
#include "../../decodingustools_amd/csrc/target_pieces.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <new>
#include <random>

using namespace clk;

// every allocation of the program is counted: the over-cap count must make none
static size_t g_allocs = 0;
void *operator new(size_t n) { ++g_allocs; void *p = malloc(n ? n : 1); if (!p) throw std::bad_alloc(); return p; }
void operator delete(void *p) noexcept { free(p); }
void operator delete(void *p, size_t) noexcept { free(p); }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s (case %d)\n", __LINE__, #cond, g_case); return 1; } } while (0)
static int g_case = 0;

static int one_case(const std::vector<uint32_t> &s, const std::vector<uint32_t> &e, uint32_t extent, uint32_t n_win)
{
    ++g_case;
    const size_t n = s.size();
    std::vector<TargetPiece> pc;
    std::vector<uint32_t> first;
    CHECK(target_pieces_build(s.data(), e.data(), n, extent, n_win, pc, first));
    CHECK(first.size() == (size_t)n_win + 1 && first[0] == 0 && first[n_win] == pc.size());
    CHECK(target_piece_count(s.data(), e.data(), n, extent) == pc.size());
    // brute force: per target and window the positions of the clipped target inside it
    std::map<std::pair<uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> want;   // (window, target) -> (first, last + 1) in-window
    std::vector<uint64_t> covered(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t ee = e[i] < extent ? e[i] : extent, ss = s[i] < ee ? s[i] : ee;
        for (uint32_t p = ss; p < ee; ++p) {
            auto it = want.find({p / 2048, (uint32_t)i});
            if (it == want.end()) want[{p / 2048, (uint32_t)i}] = {p % 2048, p % 2048 + 1};
            else { CHECK(it->second.second == p % 2048); it->second.second = p % 2048 + 1; }
        }
    }
    CHECK(want.size() == pc.size());
    // sorted by window, inside a window by target; every piece is the brute-force cut
    size_t j = 0;
    for (uint32_t w = 0; w < n_win; ++w) {
        CHECK(first[w] <= first[w + 1] && first[w + 1] <= pc.size());
        for (uint32_t k = first[w]; k < first[w + 1]; ++k, ++j) {
            const uint32_t a = pc[k].ab & 0xFFFFu, b = pc[k].ab >> 16;
            CHECK(pc[k].target < n && a < b && b <= 2048);
            CHECK(k == first[w] || pc[k - 1].target < pc[k].target);
            const auto it = want.find({w, pc[k].target});
            CHECK(it != want.end() && it->second.first == a && it->second.second == b);
            CHECK((uint64_t)w * 2048 + b <= extent);
            covered[pc[k].target] += b - a;
        }
    }
    CHECK(j == pc.size());
    // the pieces tile every target exactly
    for (size_t i = 0; i < n; ++i) {
        const uint32_t ee = e[i] < extent ? e[i] : extent, ss = s[i] < ee ? s[i] : ee;
        CHECK(covered[i] == ee - ss);
    }
    return 0;
}

int main()
{
    std::mt19937_64 rng(20240611);
    auto rnd = [&](uint64_t n) { return (uint32_t)(rng() % n); };
    // the edges by hand: empty, one position, a seam, a whole window, the extent inside a window and on a seam, beyond it
    for (uint32_t extent : {0u, 1u, 2047u, 2048u, 2049u, 4096u, 6143u, 10000u}) {
        const uint32_t n_win = (extent + 2047) / 2048;
        std::vector<uint32_t> s = {0, 0, 0, 2047, 2048, 2047, 5, extent, extent > 0 ? extent - 1 : 0, 4000, 4000, 0xFFFFFFFFu, 0};
        std::vector<uint32_t> e = {0, 1, extent, 2049, 4096, 2048, 5, extent + 9, extent, 4001, 4000, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (one_case(s, e, extent, n_win)) return 1;
        if (one_case(s, e, extent, n_win + 3)) return 1;                   // (more windows than the extent needs)
        if (one_case({}, {}, extent, n_win)) return 1;
    }
    // seeded sets: short, long, nested, repeated, shuffled by construction
    for (int c = 0; c < 60; ++c) {
        const uint32_t extent = 1 + rnd(c % 3 == 0 ? 3000 : 30000), n_win = (extent + 2047) / 2048;
        const size_t n = rnd(200);
        std::vector<uint32_t> s(n), e(n);
        for (size_t i = 0; i < n; ++i) {
            s[i] = rnd(extent + 60);
            e[i] = s[i] + (rnd(4) ? rnd(400) : rnd(extent + 60));
            if (i && rnd(8) == 0) { s[i] = s[i - 1]; e[i] = e[i - 1]; }
        }
        if (one_case(s, e, extent, n_win)) return 1;
    }
    // windows that do not cover the extent: refused
    {
        ++g_case;
        std::vector<TargetPiece> pc;
        std::vector<uint32_t> first;
        const uint32_t s = 0, e = 5000;
        CHECK(!target_pieces_build(&s, &e, 1, 5000, 2, pc, first));
    }
    // beyond the cap of cl_contig_target_order: 2^24 whole-contig targets over five windows, counted without an allocation
    {
        ++g_case;
        const size_t n = (size_t)1 << 24;
        const uint32_t extent = 5 * 2048 - 7;
        uint32_t *s = (uint32_t *)calloc(n, sizeof(uint32_t)), *e = (uint32_t *)malloc(n * sizeof(uint32_t));
        CHECK(s && e);
        for (size_t i = 0; i < n; ++i) e[i] = 0xFFFFFFFFu;
        const size_t before = g_allocs;
        const uint64_t total = target_piece_count(s, e, n, extent);
        CHECK(g_allocs == before);
        CHECK(total == 5ull * n && total > (1ull << 26));
        free(s); free(e);
    }
    printf("ok %d\n", g_case);
    return 0;
}
