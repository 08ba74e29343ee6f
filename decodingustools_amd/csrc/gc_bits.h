// gc_bits.h -- host helper of the GC-bias profile (cl_contig_gc_bias, include/callable_loci.h): the reference bytes as
// two bit planes, one bit per base each, taken where the bytes pass through the host's hands on their way to the staging
// ring (as ref_n_words of qual_pack.h takes the 'N' bit):
//   gc     the byte is one of G C g c
//   valid  the byte is one of A C G T a c g t
// Every other byte (N, n, the IUPAC codes, S among them, anything else) and every position beyond the bases given has
// both bits 0.  Plain C++ and no HIP, everything inline: a stand-alone program can include it.  AVX2 when the CPU has
// it, SSE2 (x86-64 baseline) otherwise; both are checked against the scalar form by tests/test_gc_bias_host.py.
#pragma once
#include <immintrin.h>
#include <stdint.h>

namespace dut {

// 0 scalar, 1 SSE2, 2 AVX2: what this CPU runs (the `level` argument below lets a test pin a lower one)
inline int gc_bits_level()
{
    static const int v = __builtin_cpu_supports("avx2") ? 2 : 1;
    return v;
}

namespace gc_detail {

inline void word_scalar(const uint8_t *r, uint32_t n, uint64_t &gc, uint64_t &valid)
{
    uint64_t g = 0, v = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t b = (uint8_t)(r[i] | 0x20u);
        const uint64_t is_gc = b == 'g' || b == 'c', is_at = b == 'a' || b == 't';
        g |= is_gc << i;
        v |= (is_gc | is_at) << i;
    }
    gc = g; valid = v;
}

inline void word_sse2(const uint8_t *r, uint64_t &gc, uint64_t &valid)
{
    const __m128i lc = _mm_set1_epi8(0x20), ca = _mm_set1_epi8('a'), cc = _mm_set1_epi8('c'), cg = _mm_set1_epi8('g'), ct = _mm_set1_epi8('t');
    uint64_t g = 0, v = 0;
    for (int k = 0; k < 4; ++k) {
        const __m128i b = _mm_or_si128(_mm_loadu_si128(reinterpret_cast<const __m128i *>(r + 16 * k)), lc);
        const __m128i is_gc = _mm_or_si128(_mm_cmpeq_epi8(b, cg), _mm_cmpeq_epi8(b, cc));
        const __m128i is_at = _mm_or_si128(_mm_cmpeq_epi8(b, ca), _mm_cmpeq_epi8(b, ct));
        g |= (uint64_t)(uint32_t)_mm_movemask_epi8(is_gc) << (16 * k);
        v |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_or_si128(is_gc, is_at)) << (16 * k);
    }
    gc = g; valid = v;
}

__attribute__((target("avx2"))) inline void word_avx2(const uint8_t *r, uint64_t &gc, uint64_t &valid)
{
    const __m256i lc = _mm256_set1_epi8(0x20), ca = _mm256_set1_epi8('a'), cc = _mm256_set1_epi8('c'), cg = _mm256_set1_epi8('g'),
                  ct = _mm256_set1_epi8('t');
    uint64_t g = 0, v = 0;
    for (int k = 0; k < 2; ++k) {
        const __m256i b = _mm256_or_si256(_mm256_loadu_si256(reinterpret_cast<const __m256i *>(r + 32 * k)), lc);
        const __m256i is_gc = _mm256_or_si256(_mm256_cmpeq_epi8(b, cg), _mm256_cmpeq_epi8(b, cc));
        const __m256i is_at = _mm256_or_si256(_mm256_cmpeq_epi8(b, ca), _mm256_cmpeq_epi8(b, ct));
        g |= (uint64_t)(uint32_t)_mm256_movemask_epi8(is_gc) << (32 * k);
        v |= (uint64_t)(uint32_t)_mm256_movemask_epi8(_mm256_or_si256(is_gc, is_at)) << (32 * k);
    }
    gc = g; valid = v;
}

__attribute__((target("avx2"))) inline void words_avx2(const uint8_t *r, uint64_t n_words, uint64_t *gc, uint64_t *valid, uint64_t stride)
{
    for (uint64_t w = 0; w < n_words; ++w) word_avx2(r + 64 * w, gc[w * stride], valid[w * stride]);
}

} // namespace gc_detail

// bit i of gc[w * stride] and of valid[w * stride] = the class bits of ref[64 w + i] for the n_bases bases at `ref`, 0
// for every position beyond them; n_words words are written to either plane (stride 1: two arrays; stride 2 with
// valid = gc + 1: the interleaved pairs the device reads).  ref may be null when n_bases is 0.
inline void gc_bit_words(const uint8_t *ref, uint64_t n_bases, uint64_t n_words, uint64_t *gc, uint64_t *valid, uint64_t stride = 1, int level = 2)
{
    const uint64_t whole = (n_bases >> 6) < n_words ? (n_bases >> 6) : n_words;
    if (level == 0) { for (uint64_t w = 0; w < whole; ++w) gc_detail::word_scalar(ref + 64 * w, 64, gc[w * stride], valid[w * stride]); }
    else if (level >= 2 && gc_bits_level() >= 2) gc_detail::words_avx2(ref, whole, gc, valid, stride);
    else for (uint64_t w = 0; w < whole; ++w) gc_detail::word_sse2(ref + 64 * w, gc[w * stride], valid[w * stride]);
    for (uint64_t w = whole; w < n_words; ++w) {
        const uint64_t have = n_bases > 64 * w ? (n_bases - 64 * w < 64 ? n_bases - 64 * w : 64) : 0;
        uint64_t g = 0, v = 0;
        if (have) gc_detail::word_scalar(ref + 64 * w, (uint32_t)have, g, v);
        gc[w * stride] = g; valid[w * stride] = v;                 // beyond the reference: invalid
    }
}

} // namespace dut
