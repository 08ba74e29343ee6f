// str_walk_host.cpp -- the read walk of the short-tandem-repeat mode (csrc/str_walk.h) and its host route (dut_str_measure,
// csrc/variants.cpp) as a program of their own, for AddressSanitizer + UBSan on the CPU (tests/test_str_host.py builds and
// runs it; nothing here touches a device).  It reads a case file -- reads, loci and configurations, written by the test from
// its planted cases and seeded random CIGARs -- and prints FNV-1a checksums the test recomputes from tests/str_ref.py:
//
//   walk <hex>       over every (locus, read) pair in that order, by str_measure_read itself with the first
//                    configuration's flank: the words (spanning, spanning ? delta : 0)
//   measure i <hex>  per configuration i, by dut_str_measure: the words of hist, then those of partial
//
// The case file, whitespace separated: contig_len n_reads n_loci n_configs; per read pos flag mapq n_ops and its CIGAR
// words; per locus start end; per configuration flank min_quality strands exclude_flags.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/dut_variants.h"
#include "../../decodingustools_amd/csrc/str_walk.h"

static uint64_t fnv(uint64_t h, uint32_t w)
{
    for (int k = 0; k < 4; ++k) { h ^= (w >> (8 * k)) & 255u; h *= 1099511628211ull; }
    return h;
}

static bool next(FILE *f, long long &v) { return fscanf(f, "%lld", &v) == 1; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: str_walk_host <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    long long L, n_reads, n_loci, n_cfg, v;
    if (!next(f, L) || !next(f, n_reads) || !next(f, n_loci) || !next(f, n_cfg)) return 2;
    std::vector<int32_t> pos(n_reads);
    std::vector<uint16_t> flag(n_reads);
    std::vector<uint8_t> mapq(n_reads);
    std::vector<uint32_t> coff(n_reads + 1, 0), cigar;
    for (long long r = 0; r < n_reads; ++r) {
        long long n_ops;
        if (!next(f, v)) return 2;
        pos[r] = (int32_t)v;
        if (!next(f, v)) return 2;
        flag[r] = (uint16_t)v;
        if (!next(f, v)) return 2;
        mapq[r] = (uint8_t)v;
        if (!next(f, n_ops)) return 2;
        for (long long k = 0; k < n_ops; ++k) { if (!next(f, v)) return 2; cigar.push_back((uint32_t)v); }
        coff[r + 1] = (uint32_t)cigar.size();
    }
    std::vector<cl_str_locus> loci(n_loci);
    for (auto &l : loci) { if (!next(f, v)) return 2; l.start = (uint32_t)v; if (!next(f, v)) return 2; l.end = (uint32_t)v; }
    struct Cfg { uint32_t flank, min_quality, strands, exclude; };
    std::vector<Cfg> cfg(n_cfg);
    for (auto &c : cfg) {
        long long q[4];
        for (auto &x : q) if (!next(f, x)) return 2;
        c = {(uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3]};
    }
    fclose(f);
    if (cfg.empty()) return 2;
    // an exact-size copy of every read's words: a walk that reads one word too many is then an out-of-bounds read
    uint64_t h = 14695981039346656037ull;
    for (const cl_str_locus &l : loci)
        for (long long r = 0; r < n_reads; ++r) {
            const std::vector<uint32_t> own(cigar.begin() + coff[r], cigar.begin() + coff[r + 1]);
            const dut::StrMeasure m = dut::str_measure_read((uint32_t)pos[r], own.data(), (uint32_t)own.size(), l.start, l.end, cfg[0].flank);
            h = fnv(h, m.spanning ? 1u : 0u);
            h = fnv(h, m.spanning ? (uint32_t)(int32_t)m.delta : 0u);
        }
    printf("walk %016llx\n", (unsigned long long)h);
    for (size_t i = 0; i < cfg.size(); ++i) {
        const Cfg &c = cfg[i];
        std::vector<uint32_t> hist((size_t)n_loci * c.strands * CL_STR_BINS, 0xDEADBEEFu), partial((size_t)n_loci, 0xDEADBEEFu);
        const int rc = dut_str_measure(pos.data(), c.strands == 2 ? flag.data() : nullptr, mapq.data(), coff.data(), cigar.data(), (uint64_t)n_reads, (uint32_t)L,
                                       (uint8_t)c.min_quality, (uint16_t)c.exclude, c.flank, loci.data(), loci.size(), hist.data(), partial.data(), c.strands);
        if (rc != 0) { fprintf(stderr, "dut_str_measure: %d\n", rc); return 1; }
        h = 14695981039346656037ull;
        for (uint32_t w : hist) h = fnv(h, w);
        for (uint32_t w : partial) h = fnv(h, w);
        printf("measure %zu %016llx\n", i, (unsigned long long)h);
    }
    return 0;
}
