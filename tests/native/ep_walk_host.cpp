// ep_walk_host.cpp -- the read walk of the error profile (csrc/ep_walk.h) and its host route (dut_error_profile_measure,
// csrc/variants.cpp) as a program of their own, for AddressSanitizer + UBSan on the CPU (tests/test_ep_host.py builds and
// runs it; nothing here touches a device).  It reads a case file -- reference, reads and configurations, written by the
// test from its planted cases and seeded random CIGARs -- and prints FNV-1a checksums the test recomputes from
// tests/ep_ref.py:
//
//   walk <hex>       over every read in order, by ep_walk_read itself over the first configuration's range cut at ref_len,
//                    one caller: the words n_bases, sum of p, sum of q, n_ins, sum of (p + q + l) over the insertions, n_del,
//                    sum of (p + q + l) over the deletions (sums modulo 2^32)
//   split <hex>      the same words, from walks over the two halves of that range by three callers each: every base and
//                    every event is reported once, whichever way a range is cut and dealt
//   measure i <hex>  per configuration i, by dut_error_profile_measure: the scalars n_reads, n_bases, n_uncomparable, n_ins,
//                    ins_bases, n_del, del_bases, then total, from5, from3, ins5, ins3, del5, del3, low word first
//
// The case file, whitespace separated: contig_len ref_len n_reads n_configs; the reference as ref_len numbers; per read
// pos flag mapq, n_ops and its CIGAR words, n_bases and its 4-bit codes, n_quals and its values; per configuration
// start end n_cycles min_quality filtered exclude_flags has_min_base_quality min_base_quality.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/dut_variants.h"
#include "../../decodingustools_amd/csrc/ep_walk.h"

static uint64_t fnv(uint64_t h, uint32_t w)
{
    for (int k = 0; k < 4; ++k) { h ^= (w >> (8 * k)) & 255u; h *= 1099511628211ull; }
    return h;
}
static uint64_t fnv64(uint64_t h, uint64_t w) { return fnv(fnv(h, (uint32_t)w), (uint32_t)(w >> 32)); }

static bool next(FILE *f, long long &v) { return fscanf(f, "%lld", &v) == 1; }

struct Sums {
    uint32_t w[7] = {0, 0, 0, 0, 0, 0, 0};
    void base(uint32_t p, uint32_t q) { w[0] += 1; w[1] += p; w[2] += q; }
    void ins(uint32_t p, uint32_t q, uint32_t l) { w[3] += 1; w[4] += p + q + l; }
    void del(uint32_t p, uint32_t q, uint32_t l) { w[5] += 1; w[6] += p + q + l; }
};

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: ep_walk_host <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    long long L, ref_len, n_reads, n_cfg, v, n;
    if (!next(f, L) || !next(f, ref_len) || !next(f, n_reads) || !next(f, n_cfg)) return 2;
    std::vector<uint8_t> ref(ref_len);
    for (auto &b : ref) { if (!next(f, v)) return 2; b = (uint8_t)v; }
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
    std::vector<uint8_t> seq4((codes.size() + 1) / 2, 0);                   // exactly the bytes the bases need
    for (size_t i = 0; i < codes.size(); ++i) seq4[i >> 1] |= (uint8_t)((codes[i] & 15u) << ((i & 1) ? 0 : 4));
    struct Cfg { uint32_t start, end, C, mq, filtered, exclude, has_bq, bq; };
    std::vector<Cfg> cfg(n_cfg);
    for (auto &c : cfg) {
        long long q[8];
        for (auto &x : q) if (!next(f, x)) return 2;
        c = {(uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3], (uint32_t)q[4], (uint32_t)q[5], (uint32_t)q[6], (uint32_t)q[7]};
    }
    fclose(f);
    if (cfg.empty()) return 2;
    // an exact-size copy of every read's words: a walk that reads one word too many is then an out-of-bounds read
    const uint32_t lo = cfg[0].start, hi = (uint32_t)(cfg[0].end < (uint64_t)ref_len ? cfg[0].end : (uint64_t)ref_len), mid = lo + (hi > lo ? (hi - lo) / 2 : 0);
    uint64_t h_walk = 14695981039346656037ull, h_split = h_walk;
    for (long long r = 0; r < n_reads; ++r) {
        const std::vector<uint32_t> own(cigar.begin() + coff[r], cigar.begin() + coff[r + 1]);
        const uint32_t len = (uint32_t)(soff[r + 1] - soff[r]);
        Sums one, cut;
        if (lo < hi) {
            dut::ep_walk_read((uint32_t)pos[r], own.data(), (uint32_t)own.size(), len, lo, hi, 0, 1, one);
            for (uint32_t lane = 0; lane < 3; ++lane) {
                if (lo < mid) dut::ep_walk_read((uint32_t)pos[r], own.data(), (uint32_t)own.size(), len, lo, mid, lane, 3, cut);
                dut::ep_walk_read((uint32_t)pos[r], own.data(), (uint32_t)own.size(), len, mid, hi, lane, 3, cut);
            }
        }
        for (uint32_t w : one.w) h_walk = fnv(h_walk, w);
        for (uint32_t w : cut.w) h_split = fnv(h_split, w);
    }
    printf("walk %016llx\nsplit %016llx\n", (unsigned long long)h_walk, (unsigned long long)h_split);
    const dut_ep_reads reads = {(uint64_t)n_reads, pos.data(), flag.data(), mapq.data(), coff.data(), cigar.data(), soff.data(), seq4.data(), qoff.data(), qual.data()};
    for (size_t i = 0; i < cfg.size(); ++i) {
        const Cfg &c = cfg[i];
        const dut_ep_options opt = {(uint8_t)c.mq, (int)c.filtered, (uint16_t)c.exclude, (int)c.has_bq, (uint8_t)c.bq, c.C};
        std::vector<uint64_t> tables((size_t)36 * c.C, 0xDEADBEEFDEADBEEFull);
        cl_ep_result res;
        const int rc = dut_error_profile_measure(&reads, (uint32_t)L, ref.data(), (uint64_t)ref_len, c.start, c.end, &opt, tables.data(), &res);
        if (rc != 0) { fprintf(stderr, "dut_error_profile_measure: %d\n", rc); return 1; }
        uint64_t h = 14695981039346656037ull;
        for (uint64_t w : {res.n_reads, res.n_bases, res.n_uncomparable, res.n_ins, res.ins_bases, res.n_del, res.del_bases}) h = fnv64(h, w);
        for (uint64_t w : res.total) h = fnv64(h, w);
        for (uint64_t w : tables) h = fnv64(h, w);
        printf("measure %zu %016llx\n", i, (unsigned long long)h);
    }
    return 0;
}
