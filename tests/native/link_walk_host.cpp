// link_walk_host.cpp -- the read walk of the linked sites (csrc/link_walk.h) and its host route (dut_link_measure,
// csrc/variants.cpp) as a program of their own, for AddressSanitizer + UBSan on the CPU (tests/test_link_host.py builds and
// runs it; nothing here touches a device).  It reads a case file -- reads, sites and configurations, written by the test
// from its planted cases and seeded random CIGARs -- and prints FNV-1a checksums the test recomputes from
// tests/link_ref.py:
//
//   walk <hex>       over every read that starts inside the contig and has a reference span, in order, and every site it
//                    covers as an anchor, by link_observe_read itself over exact-size copies of the read's CIGAR words,
//                    bases and quality values and of the anchor's sites under the first configuration: the two halves of
//                    the packed observations, low first
//   measure i <hex>  per configuration i, by dut_link_measure: the words of first, then tables, then site_counts
//
// The case file, whitespace separated: contig_len n_reads n_sites n_configs; per read pos flag mapq, n_ops and its CIGAR
// words, n_bases and its 4-bit codes, n_quals and its values; the sites; per configuration max_dist max_partners
// min_quality filtered exclude_flags has_min_base_quality min_base_quality.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/dut_variants.h"
#include "../../decodingustools_amd/csrc/link_walk.h"

static uint64_t fnv(uint64_t h, uint32_t w)
{
    for (int k = 0; k < 4; ++k) { h ^= (w >> (8 * k)) & 255u; h *= 1099511628211ull; }
    return h;
}

static bool next(FILE *f, long long &v) { return fscanf(f, "%lld", &v) == 1; }

// one read's bases and quality values, each in a vector of exactly its size
struct Own {
    std::vector<uint8_t> codes, quals;
    bool use_bq;
    uint8_t thr;
    uint32_t code(uint32_t q) const { return codes.at(q); }
    bool passes(uint32_t q) const { return !use_bq || q >= quals.size() || quals[q] >= thr; }
};

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: link_walk_host <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    long long L, n_reads, n_sites, n_cfg, v, n;
    if (!next(f, L) || !next(f, n_reads) || !next(f, n_sites) || !next(f, n_cfg)) return 2;
    std::vector<int32_t> pos(n_reads);
    std::vector<uint16_t> flag(n_reads);
    std::vector<uint8_t> mapq(n_reads), qual, codes;
    std::vector<uint32_t> coff(n_reads + 1, 0), cigar;
    std::vector<uint64_t> soff(n_reads + 1, 0), qoff(n_reads + 1, 0);
    for (long long r = 0; r < n_reads; ++r) {
        if (!next(f, v)) return 2;
        pos[r] = (int32_t)v;
        if (!next(f, v)) return 2;
        flag[r] = (uint16_t)v;
        if (!next(f, v)) return 2;
        mapq[r] = (uint8_t)v;
        if (!next(f, n)) return 2;
        for (long long k = 0; k < n; ++k) { if (!next(f, v)) return 2; cigar.push_back((uint32_t)v); }
        coff[r + 1] = (uint32_t)cigar.size();
        if (!next(f, n)) return 2;
        for (long long k = 0; k < n; ++k) { if (!next(f, v)) return 2; codes.push_back((uint8_t)v); }
        soff[r + 1] = codes.size();
        if (!next(f, n)) return 2;
        for (long long k = 0; k < n; ++k) { if (!next(f, v)) return 2; qual.push_back((uint8_t)v); }
        qoff[r + 1] = qual.size();
    }
    std::vector<uint32_t> sites(n_sites);
    for (auto &s : sites) { if (!next(f, v)) return 2; s = (uint32_t)v; }
    struct Cfg { uint32_t D, K, mq, filtered, exclude, has_bq, bq; };
    std::vector<Cfg> cfg(n_cfg);
    for (auto &c : cfg) {
        long long q[7];
        for (auto &x : q) if (!next(f, x)) return 2;
        c = {(uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3], (uint32_t)q[4], (uint32_t)q[5], (uint32_t)q[6]};
    }
    fclose(f);
    if (cfg.empty()) return 2;
    std::vector<uint8_t> seq4((codes.size() + 1) / 2, 0);                   // exactly the bytes the bases need
    for (size_t i = 0; i < codes.size(); ++i) seq4[i >> 1] |= (uint8_t)((codes[i] & 15u) << ((i & 1) ? 0 : 4));
    uint64_t h_walk = 14695981039346656037ull;
    for (long long r = 0; r < n_reads; ++r) {
        if (pos[r] < 0 || pos[r] >= L) continue;
        const std::vector<uint32_t> own(cigar.begin() + coff[r], cigar.begin() + coff[r + 1]);
        uint64_t span = 0;
        for (uint32_t c : own) span += ((0x18Du >> (c & 15u)) & 1u) ? (c >> 4) : 0u;
        if (!span) continue;
        const Own src{std::vector<uint8_t>(codes.begin() + soff[r], codes.begin() + soff[r + 1]), std::vector<uint8_t>(qual.begin() + qoff[r], qual.begin() + qoff[r + 1]),
                      cfg[0].filtered && cfg[0].has_bq, (uint8_t)cfg[0].bq};
        for (size_t i = 0; i < sites.size(); ++i) {
            if (sites[i] < (uint32_t)pos[r] || (uint64_t)sites[i] >= (uint64_t)pos[r] + span) continue;
            const uint32_t m = 1u + dut::link_partner_count(sites.data(), sites.size(), i, cfg[0].D, cfg[0].K);
            const std::vector<uint32_t> mine(sites.begin() + i, sites.begin() + i + m);
            const uint64_t obs = dut::link_observe_read((uint32_t)pos[r], own.data(), (uint32_t)own.size(), (uint32_t)src.codes.size(), mine.data(), m, src);
            h_walk = fnv(fnv(h_walk, (uint32_t)obs), (uint32_t)(obs >> 32));
        }
    }
    printf("walk %016llx\n", (unsigned long long)h_walk);
    const dut_ep_reads reads = {(uint64_t)n_reads, pos.data(), flag.data(), mapq.data(), coff.data(), cigar.data(), soff.data(), seq4.data(), qoff.data(), qual.data()};
    for (size_t i = 0; i < cfg.size(); ++i) {
        const Cfg &c = cfg[i];
        const dut_link_options opt = {1, (uint8_t)c.mq, (int)c.filtered, (uint16_t)c.exclude, (int)c.has_bq, (uint8_t)c.bq, c.D, c.K, 1, 0};
        uint64_t n_pairs = 0;
        if (dut_link_pair_offsets(sites.data(), sites.size(), c.D, c.K, nullptr, &n_pairs) != 0) { fprintf(stderr, "dut_link_pair_offsets refused\n"); return 1; }
        std::vector<uint32_t> first(sites.size() + 1, 0xDEADBEEFu), tables((size_t)n_pairs * 36, 0xDEADBEEFu), counts(sites.size() * 6, 0xDEADBEEFu);
        const int rc = dut_link_measure(&reads, (uint32_t)L, &opt, sites.data(), sites.size(), first.data(), tables.data(), counts.data());
        if (rc != 0) { fprintf(stderr, "dut_link_measure: %d\n", rc); return 1; }
        uint64_t h = 14695981039346656037ull;
        for (uint32_t w : first) h = fnv(h, w);
        for (uint32_t w : tables) h = fnv(h, w);
        for (uint32_t w : counts) h = fnv(h, w);
        printf("measure %zu %016llx\n", i, (unsigned long long)h);
    }
    return 0;
}
