// fp_compare_host.cpp -- csrc/fp_compare.h in a program of its own, for AddressSanitizer + UBSan: the two-pointer merge and
// the file parser over heap buffers of exactly the size they are given.
//   fp_compare_host merge <file>   the file: u64 n_sketches, then per sketch u64 scaled, u64 n, n u64 hashes, n u32 counts;
//                                  prints "i j n_a n_b n_common sum_a sum_b sum_min" for every ordered pair
//   fp_compare_host parse <file>   prints "ok ksize scaled n sum_of_hashes sum_of_counts region max_frequency|-" or "error <message>"
#include "../../decodingustools_amd/csrc/fp_compare.h"

#include <cinttypes>
#include <memory>

struct Sk {
    uint64_t scaled = 0, n = 0;
    std::unique_ptr<uint64_t[]> h;               // exactly n elements each: one read past either end is reported
    std::unique_ptr<uint32_t[]> c;
};

static bool read_exact(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static int run_merge(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    uint64_t ns = 0;
    if (!read_exact(f, &ns, 8)) return 2;
    std::vector<Sk> sk(ns);
    for (Sk &s : sk) {
        if (!read_exact(f, &s.scaled, 8) || !read_exact(f, &s.n, 8)) return 2;
        s.h.reset(new uint64_t[s.n]);
        s.c.reset(new uint32_t[s.n]);
        if (!read_exact(f, s.h.get(), 8 * s.n) || !read_exact(f, s.c.get(), 4 * s.n)) return 2;
        const std::string bad = fpc::validate(31, s.scaled, s.h.get(), s.c.get(), s.n);
        if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 2; }
    }
    fclose(f);
    for (size_t i = 0; i < sk.size(); ++i)
        for (size_t j = 0; j < sk.size(); ++j) {
            const uint64_t cut = std::min(fpc::max_hash(sk[i].scaled), fpc::max_hash(sk[j].scaled));
            const dut_fpc_record r = fpc::merge_pair(sk[i].h.get(), sk[i].c.get(), sk[i].n, sk[j].h.get(), sk[j].c.get(), sk[j].n, cut);
            printf("%zu %zu %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", i, j, r.n_a, r.n_b, r.n_common,
                   r.sum_a, r.sum_b, r.sum_min);
        }
    return 0;
}

static int run_parse(const char *path)
{
    // the text in a heap block of exactly its size, as parse_file holds it
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::unique_ptr<char[]> text(new char[(size_t)len]);
    if (!read_exact(f, text.get(), (size_t)len)) return 2;
    fclose(f);
    fpc::SketchFile s;
    const std::string bad = fpc::parse_text(text.get(), (size_t)len, s);
    fpc::SketchFile s2;
    const std::string bad2 = fpc::parse_file(path, s2);
    if (bad.empty() != bad2.empty() || s.hashes != s2.hashes || s.counts != s2.counts) { fprintf(stderr, "parse_text and parse_file differ\n"); return 2; }
    if (!bad.empty()) { printf("error %s\n", bad.c_str()); return 0; }
    uint64_t sh = 0, sc = 0;
    for (uint64_t h : s.hashes) sh += h;
    for (uint32_t c : s.counts) sc += c;
    printf("ok %u %" PRIu64 " %zu %" PRIu64 " %" PRIu64 " %s %s\n", s.ksize, s.scaled, s.hashes.size(), sh, sc,
           s.region.empty() ? "-" : s.region.c_str(), s.has_max_frequency ? std::to_string(s.max_frequency).c_str() : "-");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: fp_compare_host merge|parse <file>\n"); return 2; }
    if (!strcmp(argv[1], "merge")) return run_merge(argv[2]);
    if (!strcmp(argv[1], "parse")) return run_parse(argv[2]);
    return 2;
}
