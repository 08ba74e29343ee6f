// fp_compare.h -- the host side of fingerprint-compare that needs no HIP: max_hash, the validation of a sketch, the
// two-pointer merge that is the yardstick of the device kernel (dut_fpc_compare_host), and the reader of the files
// `fingerprint -o` writes.  tests/native/fp_compare_host.cpp compiles this text under the sanitizers.
#pragma once
#include "../../include/dut_fingerprint.h"

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace fpc {

// ((u64::MAX as f64) / scaled as f64) as u64, with Rust's saturating cast (scaled 0 and 1: u64::MAX)
inline uint64_t max_hash(uint64_t scaled)
{
    const double two64 = 18446744073709551616.0;
    const double d = two64 / (double)scaled;
    if (!(d < two64)) return ~0ull;
    return (uint64_t)d;
}

// "" when the sketch is valid, else what is wrong and where
inline std::string validate(uint32_t ksize, uint64_t scaled, const uint64_t *h, const uint32_t *c, uint64_t n)
{
    if (ksize < 1 || ksize > 64) return "ksize " + std::to_string(ksize) + " is outside 1..64";
    if (n && (!h || !c)) return "null hashes or counts";
    for (uint64_t i = 0; i < n; ++i) {
        if (c[i] == 0) return "a count of 0 at index " + std::to_string(i);
        if (i && h[i] <= h[i - 1]) return "hashes are not strictly ascending at index " + std::to_string(i);
    }
    if (n && h[n - 1] > max_hash(scaled))
        return "the hash at index " + std::to_string(n - 1) + " is above max_hash of scaled " + std::to_string(scaled);
    return "";
}

// entries with hash <= cut (a prefix: the hashes ascend)
inline uint64_t prefix_len(const uint64_t *h, uint64_t n, uint64_t cut)
{
    return (uint64_t)(std::upper_bound(h, h + n, cut) - h);
}

// one pair by a two-pointer merge over the prefixes within the cut
inline dut_fpc_record merge_pair(const uint64_t *ha, const uint32_t *ca, uint64_t na, const uint64_t *hb,
                                 const uint32_t *cb, uint64_t nb, uint64_t cut)
{
    dut_fpc_record r{};
    r.n_a = prefix_len(ha, na, cut);
    r.n_b = prefix_len(hb, nb, cut);
    uint64_t i = 0, j = 0;
    while (i < r.n_a && j < r.n_b) {
        const uint64_t x = ha[i], y = hb[j];
        if (x == y) {
            r.n_common += 1;
            r.sum_min += std::min(ca[i], cb[j]);
            r.sum_a += ca[i++];
            r.sum_b += cb[j++];
        } else if (x < y) r.sum_a += ca[i++];
        else r.sum_b += cb[j++];
    }
    for (; i < r.n_a; ++i) r.sum_a += ca[i];
    for (; j < r.n_b; ++j) r.sum_b += cb[j];
    return r;
}

// what dut_fp_file_read keeps behind dut_fpc_sketch::owner
struct SketchFile {
    uint32_t ksize = 0;
    uint64_t scaled = 0;
    std::string region;
    uint32_t max_frequency = 0;
    bool has_max_frequency = false;
    std::vector<uint64_t> hashes;
    std::vector<uint32_t> counts;
};

// the decimal number of [p, e) (digits only, at least one); false when malformed or above `most`
inline bool parse_u64(const char *p, const char *e, uint64_t most, uint64_t *out)
{
    if (p == e) return false;
    uint64_t v = 0;
    for (; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        const uint64_t d = (uint64_t)(*p - '0');
        if (v > (most - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

// the whole text of a file: "" or "<line>: <what>" (line 0: before any line)
inline std::string parse_text(const char *text, size_t len, SketchFile &s)
{
    bool has_k = false, has_s = false, in_entries = false;
    uint64_t mh = 0, line_no = 0;
    const char *p = text, *end = text + len;
    auto at = [&](const std::string &what) { return std::to_string(line_no) + ": " + what; };
    auto missing = [&]() { return at(std::string("missing #") + (has_k ? "scaled" : "ksize") + "= in the header"); };
    while (p < end) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *e = nl ? nl : end;
        const char *next = nl ? nl + 1 : end;
        if (e > p && e[-1] == '\r') --e;
        ++line_no;
        if (!in_entries && e > p && *p == '#') {
            const char *eq = (const char *)memchr(p, '=', (size_t)(e - p));
            if (eq) {
                const std::string key(p + 1, eq), val(eq + 1, e);
                uint64_t v = 0;
                if (key == "ksize") {
                    if (!parse_u64(eq + 1, e, 64, &v) || v < 1) return at("malformed ksize '" + val + "' (1..64)");
                    s.ksize = (uint32_t)v; has_k = true;
                } else if (key == "scaled") {
                    if (!parse_u64(eq + 1, e, ~0ull, &v)) return at("malformed scaled '" + val + "'");
                    s.scaled = v; has_s = true;
                } else if (key == "max_frequency") {
                    if (!parse_u64(eq + 1, e, 0xFFFFFFFFull, &v)) return at("malformed max_frequency '" + val + "'");
                    s.max_frequency = (uint32_t)v; s.has_max_frequency = true;
                } else if (key == "region") s.region = val;
            }
            p = next;
            continue;
        }
        if (e == p && next == end) break;                      // an empty last line
        if (!in_entries) {
            if (!has_k || !has_s) return missing();
            in_entries = true;
            mh = max_hash(s.scaled);
        }
        const char *tab = (const char *)memchr(p, '\t', (size_t)(e - p));
        uint64_t h = 0, c = 0;
        if (!tab) return at("expected hash<TAB>count");
        if (!parse_u64(p, tab, ~0ull, &h)) return at("malformed or overflowing hash '" + std::string(p, tab) + "'");
        if (!parse_u64(tab + 1, e, 0xFFFFFFFFull, &c)) return at("malformed or overflowing count '" + std::string(tab + 1, e) + "'");
        if (c == 0) return at("a count of 0");
        if (!s.hashes.empty() && h <= s.hashes.back()) return at("hashes are not strictly ascending");
        if (h > mh) return at("hash " + std::to_string(h) + " is above max_hash " + std::to_string(mh) + " of scaled " + std::to_string(s.scaled));
        s.hashes.push_back(h);
        s.counts.push_back((uint32_t)c);
        p = next;
    }
    if (!has_k || !has_s) { ++line_no; return missing(); }
    return "";
}

// "" or "<path>:<line>: <what>" / "<path>: <what>"
inline std::string parse_file(const char *path, SketchFile &s)
{
    FILE *f = fopen(path, "rb");
    if (!f) return std::string(path) + ": cannot open: " + strerror(errno);
    std::vector<char> buf;
    char tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return std::string(path) + ": read failed";
    const std::string e = parse_text(buf.data(), buf.size(), s);
    return e.empty() ? e : std::string(path) + ":" + e;
}

} // namespace fpc
