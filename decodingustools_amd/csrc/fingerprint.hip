// fingerprint.hip -- the `fingerprint` engine (include/dut_fingerprint.h): k-mer hashing, survivor compaction
// and the sorted (hash, count) table on the device; SHA-256 digest, file readers' driver and the CLI's file level
// on the host.
//
// Contract (collectors/fingerprint/processor.rs:117-140, utils.rs:11-34): for every window of k bytes without an
// uppercase 'N', canonical = min(window, revcomp(window)) in byte order, where revcomp maps A<->T, C<->G and every
// other byte to 'N'; h = SeaHash(canonical) (seahash 4.1, one write, no length prefix); h <= max_hash is counted.
//
// Device layout of a batch: sequences cut into strips of kStrip consecutive window starts, one strip per thread.
// A thread keeps rolling 2-bit forward / reverse-complement words (one u64 for k <= 32, two for 33..64) and the
// last positions of an 'N' and of any other non-ACGT byte; a window of ACGT only is hashed from the 2-bit words
// (A<C<G<T in ASCII, so integer order is byte order), any other window by the exact byte path.  Survivors are
// compacted with one ballot and one atomic per wave, then sorted, run-length reduced and merged into the resident
// table with rocPRIM (header-only, compiled into this library).
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

#include "../../include/dut_bam.h"
#include "../../include/dut_fingerprint.h"
#include "fp_compare.h"
#include "host_parallel.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#define FP_HD __host__ __device__ __forceinline__

namespace fp {

constexpr uint32_t kStrip = 64;                  // window starts per thread
constexpr uint32_t kBlock = 256;
constexpr uint64_t kDefaultBatchBases = 32ull << 20;
constexpr uint64_t kMaxBatchBases = 1ull << 30;  // survivors are counted in 32 bits

// ---- SeaHash (seahash 4.1, one-shot write) ----
FP_HD uint64_t sea_diffuse(uint64_t x)
{
    x *= 0x6eed0e9da4d94a4full;
    x ^= (x >> 32) >> (x >> 60);
    x *= 0x6eed0e9da4d94a4full;
    return x;
}

// word i goes to lane i % 4; the lanes rotate instead of being indexed (the final XOR does not see the order)
struct Sea {
    uint64_t a = 0x16f11fe89b0d677cull, b = 0xb480a793d8e6c86cull, c = 0x6fe2e5aaf078ebc9ull, d = 0x14f994a4c5259381ull;
    FP_HD void push(uint64_t w)
    {
        const uint64_t t = sea_diffuse(a ^ w);
        a = b; b = c; c = d; d = t;
    }
    FP_HD uint64_t finish(uint64_t len) const { return sea_diffuse(a ^ b ^ c ^ d ^ len); }
};

FP_HD uint8_t comp_byte(uint8_t x)
{
    return x == 'A' ? 'T' : x == 'T' ? 'A' : x == 'C' ? 'G' : x == 'G' ? 'C' : 'N';
}

// BAM's 4-bit code -> its byte (=ACMGRSVTWYHKDBN), from two constants instead of a table in memory
FP_HD uint8_t seq4_byte(uint32_t nib)
{
    const uint64_t lo = 0x565352474d43413dull;   // "=ACMGRSV" little-endian
    const uint64_t hi = 0x4e42444b48595754ull;   // "TWYHKDBN"
    return (uint8_t)((nib < 8 ? lo >> (8 * nib) : hi >> (8 * (nib - 8))) & 0xFFu);
}

// the two input forms: byte(p) is the base at absolute position p; cls(p) 0..3 = A,C,G,T, 4 = 'N', 5 = other
struct SrcBytes {
    const uint8_t *p;
    FP_HD uint8_t byte(uint64_t i) const { return p[i]; }
    FP_HD uint32_t cls(uint64_t i) const
    {
        const uint32_t b = p[i];
        if (b == 'A' || b == 'C' || b == 'G' || b == 'T') return ((b >> 1) ^ (b >> 2)) & 3u;
        return b == 'N' ? 4u : 5u;
    }
};
struct SrcSeq4 {
    const uint8_t *p;
    FP_HD uint32_t nib(uint64_t i) const { return (p[i >> 1] >> ((~i & 1u) * 4u)) & 15u; }
    FP_HD uint8_t byte(uint64_t i) const { return seq4_byte(nib(i)); }
    FP_HD uint32_t cls(uint64_t i) const
    {
        const uint32_t n = nib(i);
        if (n == 1u) return 0u;
        if (n == 2u) return 1u;
        if (n == 4u) return 2u;
        if (n == 8u) return 3u;
        return n == 15u ? 4u : 5u;
    }
};

// exact byte path: the window [s, s + k) of any bytes without 'N'
template <class Src>
FP_HD uint64_t hash_window_bytes(const Src &src, uint64_t s, uint32_t k)
{
    bool use_rc = false;
    for (uint32_t j = 0; j < k; ++j) {
        const uint8_t f = src.byte(s + j), r = comp_byte(src.byte(s + k - 1 - j));
        if (f != r) { use_rc = r < f; break; }
    }
    Sea h;
    for (uint32_t m = 0; m < k; m += 8) {
        uint64_t w = 0;
        for (uint32_t b = 0; b < 8 && m + b < k; ++b) {
            const uint32_t j = m + b;
            const uint8_t c = use_rc ? comp_byte(src.byte(s + k - 1 - j)) : src.byte(s + j);
            w |= (uint64_t)c << (8 * b);
        }
        h.push(w);
    }
    return h.finish(k);
}

// fast path: the canonical window as 2-bit codes, base j at bit 2(k-1-j) of the 128-bit (hi, lo)
FP_HD uint64_t hash_window_codes(uint64_t hi, uint64_t lo, uint32_t k)
{
    const uint32_t ascii = 0x54474341u;          // "ACGT"
    Sea h;
    for (uint32_t m = 0; m < k; m += 8) {
        uint64_t w = 0;
        for (uint32_t b = 0; b < 8 && m + b < k; ++b) {
            const uint32_t pos = 2 * (k - 1 - (m + b));
            const uint32_t c = (uint32_t)((pos >= 64 ? hi >> (pos - 64) : lo >> pos) & 3u);
            w |= (uint64_t)((ascii >> (8 * c)) & 0xFFu) << (8 * b);
        }
        h.push(w);
    }
    return h.finish(k);
}

// One strip: the windows w0 .. w0 + nwin - 1 (absolute base positions of their first base), k - 1 bases of
// priming first.  `iters` >= k - 1 + nwin is the loop count (uniform over a wave on the device; the extra steps
// read nothing).  emit(in_range, has_n, h, window_index_in_strip) is called once per step from k - 1 on.
template <bool WIDE, class Src, class Emit>
FP_HD void strip_walk(const Src &src, uint64_t w0, uint32_t nwin, uint32_t k, uint32_t iters, Emit &emit)
{
    const uint32_t need = nwin ? k - 1 + nwin : 0;  // a lane without windows reads nothing
    uint64_t fh = 0, fl = 0, rh = 0, rl = 0;
    const uint64_t mask_lo = (!WIDE && k < 32) ? ((1ull << (2 * k)) - 1) : ~0ull;
    const uint64_t mask_hi = (WIDE && k < 64) ? ((1ull << (2 * k - 64)) - 1) : ~0ull;
    uint32_t last_n1 = 0, last_o1 = 0;           // 1 + step of the last 'N' / other byte, 0 = none
    for (uint32_t t = 0; t < iters; ++t) {
        const bool live = t < need;
        const uint32_t cl = live ? src.cls(w0 + t) : 0u;
        if (cl == 4u) last_n1 = t + 1;
        if (cl == 5u) last_o1 = t + 1;
        const uint64_t c = cl & 3u;              // N / other: any code (such a window never takes the fast path)
        if (!WIDE) {
            fl = ((fl << 2) | c) & mask_lo;
            rl = (rl >> 2) | ((3u - c) << (2 * k - 2));
        } else {
            fh = ((fh << 2) | (fl >> 62)) & mask_hi;
            fl = (fl << 2) | c;
            rl = (rl >> 2) | (rh << 62);
            rh = (rh >> 2) | ((3u - c) << (2 * k - 66));
        }
        if (t + 1 < k) continue;
        const uint32_t wi = t + 1 - k;
        const bool in_range = wi < nwin;
        const bool has_n = last_n1 + k - 1 > t;
        uint64_t h = 0;
        if (in_range && !has_n) {
            if (last_o1 + k - 1 > t) h = hash_window_bytes(src, w0 + wi, k);
            else if (!WIDE) h = hash_window_codes(0, fl < rl ? fl : rl, k);
            else {
                const bool f_lt = fh < rh || (fh == rh && fl < rl);
                h = f_lt ? hash_window_codes(fh, fl, k) : hash_window_codes(rh, rl, k);
            }
        }
        emit(in_range, has_n, h, wi);
    }
}

inline uint64_t max_hash(uint64_t scaled) { return fpc::max_hash(scaled); }   // (fp_compare.h: the file reader checks against it too)

// ---- SHA-256 (FIPS 180-4) ----
struct Sha256 {
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    uint8_t blk[64];
    size_t nb = 0;
    uint64_t total = 0;
    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void compress(const uint8_t *p)
    {
        static const uint32_t K[64] = {
            0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
            0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
            0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
            0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
            0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
            0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
            0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
            0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
        uint32_t w[64];
        for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void update(const uint8_t *p, size_t n)
    {
        total += n;
        while (n) {
            const size_t take = std::min(n, 64 - nb);
            memcpy(blk + nb, p, take);
            nb += take; p += take; n -= take;
            if (nb == 64) { compress(blk); nb = 0; }
        }
    }
    void final(uint8_t out[32])
    {
        const uint64_t bits = total * 8;
        const uint8_t one = 0x80, zero = 0;
        update(&one, 1);
        while (nb != 56) update(&zero, 1);
        uint8_t len[8];
        for (int i = 0; i < 8; ++i) len[i] = (uint8_t)(bits >> (56 - 8 * i));
        update(len, 8);
        for (int i = 0; i < 8; ++i) { out[4 * i] = (uint8_t)(h[i] >> 24); out[4 * i + 1] = (uint8_t)(h[i] >> 16); out[4 * i + 2] = (uint8_t)(h[i] >> 8); out[4 * i + 3] = (uint8_t)h[i]; }
    }
};

void hexdigest(const std::vector<uint64_t> &hs, const std::vector<uint32_t> &cs, char out[65])
{
    Sha256 s;
    uint8_t rec[12];
    for (size_t i = 0; i < hs.size(); ++i) {
        for (int b = 0; b < 8; ++b) rec[b] = (uint8_t)(hs[i] >> (8 * b));
        for (int b = 0; b < 4; ++b) rec[8 + b] = (uint8_t)(cs[i] >> (8 * b));
        s.update(rec, 12);
    }
    uint8_t d[32];
    s.final(d);
    for (int i = 0; i < 32; ++i) snprintf(out + 2 * i, 3, "%02x", d[i]);
    out[64] = 0;
}

// ---- the hash kernel ----
// strip t -> sequence strip_seq[t]; its strips begin at strip_first[seq]; bases [off[seq], off[seq + 1]).
template <bool SEQ4, bool WIDE>
__global__ __launch_bounds__(kBlock) void k_fp_hash(const uint8_t *__restrict__ data, const uint64_t *__restrict__ off,
                                                     const uint32_t *__restrict__ strip_first, const uint32_t *__restrict__ strip_seq,
                                                     uint32_t n_strips, uint32_t k, uint64_t max_hash, uint64_t *__restrict__ surv,
                                                     uint32_t *__restrict__ n_surv)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const bool in = t < n_strips;                 // lanes past the end walk nothing but join every ballot
    uint64_t w0 = 0;
    uint32_t nwin = 0;
    if (in) {
        const uint32_t s = strip_seq[t];
        const uint64_t b = off[s], len = off[s + 1] - b;
        const uint64_t j = (uint64_t)(t - strip_first[s]) * kStrip;
        w0 = b + j;
        nwin = (uint32_t)std::min<uint64_t>(kStrip, len - k + 1 - j);
    }
    const uint32_t lane = threadIdx.x & 63u;
    auto emit = [&](bool in_range, bool has_n, uint64_t h, uint32_t) {
        const bool keep = in_range && !has_n && h <= max_hash;
        const uint64_t m = __ballot(keep);
        if (m == 0) return;                       // uniform over the wave
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(n_surv, (uint32_t)__popcll(m));
        base = __shfl(base, 0);
        if (keep) surv[base + __popcll(m & ((1ull << lane) - 1ull))] = h;
    };
    if (SEQ4) strip_walk<WIDE>(SrcSeq4{data}, w0, nwin, k, k - 1 + kStrip, emit);
    else strip_walk<WIDE>(SrcBytes{data}, w0, nwin, k, k - 1 + kStrip, emit);
}

struct SumU32 {
    __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }   // u32 wraps as the reference's
};

} // namespace fp

struct dut_fp_ctx {
    dut_fp_options opt{};
    uint64_t max_hash = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    uint64_t batch_bases = fp::kDefaultBatchBases;
    uint64_t processed = 0;
    // device buffers (grow-only) and their capacities in elements
    uint8_t *d_data = nullptr; size_t cap_data = 0;
    uint64_t *d_off = nullptr; size_t cap_off = 0;
    uint32_t *d_sfirst = nullptr; size_t cap_sfirst = 0;
    uint32_t *d_sseq = nullptr; size_t cap_sseq = 0;
    uint64_t *d_surv = nullptr, *d_sorted = nullptr, *d_uniq = nullptr; size_t cap_surv = 0;
    uint32_t *d_runc = nullptr; size_t cap_runc = 0;
    uint32_t *d_scal = nullptr;                                   // [0] survivors, [1] runs, [2] merged distinct
    void *d_tmp = nullptr; size_t cap_tmp = 0;
    uint64_t *d_tk = nullptr, *d_mk = nullptr, *d_nk = nullptr;   // table, merged, next table
    uint32_t *d_tc = nullptr, *d_mc = nullptr, *d_nc = nullptr;
    size_t cap_table = 0;
    uint64_t n_table = 0;
    // pinned staging
    uint8_t *h_stage = nullptr; size_t cap_stage = 0;
    uint32_t *h_scal = nullptr;
    hipEvent_t ev[4] = {};
    // DUT_TIMING / dut_fp_stats
    double hash_ms = 0, reduce_ms = 0, h2d_ms = 0;
    uint64_t n_windows = 0, n_batches = 0;
    // the last result
    std::vector<uint64_t> out_h;
    std::vector<uint32_t> out_c;
};

namespace fp {

int dev_fail(dut_fp_ctx *c, hipError_t e, const char *what)
{
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? CL_ERR_NOMEM : CL_ERR_DEVICE;
}
#define FP_CK(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fp::dev_fail(c, e_, what); } while (0)

template <class T>
int grow(dut_fp_ctx *c, T *&p, size_t &cap, size_t need, const char *what)
{
    if (need <= cap) return CL_OK;
    size_t n = std::max(need, cap + cap / 2);
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
    if (e != hipSuccess && n > need) { (void)hipGetLastError(); n = need; e = hipMalloc((void **)&p, n * sizeof(T)); }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        c->err = std::string("device memory exhausted: ") + what + " of " + std::to_string(need) + " entries does not fit";
        return CL_ERR_NOMEM;
    }
    cap = n;
    return CL_OK;
}
#define FP_GROW(p, cap, need, what) do { const int r_ = fp::grow(c, p, cap, (size_t)(need), what); if (r_ != CL_OK) return r_; } while (0)

int tmp_need(dut_fp_ctx *c, size_t bytes)
{
    if (bytes <= c->cap_tmp) return CL_OK;
    return grow(c, *(uint8_t **)&c->d_tmp, c->cap_tmp, bytes, "sort scratch");
}

// the survivors of one batch (on the device) into the table: sort, run-length reduce, merge, reduce equal keys
int reduce_batch(dut_fp_ctx *c, uint32_t n)
{
    size_t tb = 0;
    FP_CK(rocprim::radix_sort_keys(nullptr, tb, c->d_surv, c->d_sorted, n, 0, 64, c->stream), "radix_sort_keys");
    if (int r = tmp_need(c, tb)) return r;
    FP_CK(rocprim::radix_sort_keys(c->d_tmp, tb, c->d_surv, c->d_sorted, n, 0, 64, c->stream), "radix_sort_keys");
    FP_GROW(c->d_runc, c->cap_runc, n, "run counts");
    tb = 0;
    FP_CK(rocprim::run_length_encode(nullptr, tb, c->d_sorted, n, c->d_uniq, c->d_runc, c->d_scal + 1, c->stream), "run_length_encode");
    if (int r = tmp_need(c, tb)) return r;
    FP_CK(rocprim::run_length_encode(c->d_tmp, tb, c->d_sorted, n, c->d_uniq, c->d_runc, c->d_scal + 1, c->stream), "run_length_encode");
    FP_CK(hipMemcpyAsync(c->h_scal + 1, c->d_scal + 1, 4, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
    FP_CK(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    const uint64_t runs = c->h_scal[1];
    const uint64_t T = c->n_table, M = T + runs;
    if (M > c->cap_table) {
        // the table's three buffers grow together; the live table is carried over
        size_t cap = std::max<size_t>(M, c->cap_table + c->cap_table / 2);
        uint64_t *tk = nullptr; uint32_t *tc = nullptr; size_t ck = 0, cc = 0;
        if (int r = grow(c, tk, ck, cap, "fingerprint table")) return r;
        if (int r = grow(c, tc, cc, cap, "fingerprint table")) { (void)hipFree(tk); return r; }
        if (T) {
            FP_CK(hipMemcpyAsync(tk, c->d_tk, T * 8, hipMemcpyDeviceToDevice, c->stream), "hipMemcpyAsync");
            FP_CK(hipMemcpyAsync(tc, c->d_tc, T * 4, hipMemcpyDeviceToDevice, c->stream), "hipMemcpyAsync");
            FP_CK(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        }
        (void)hipFree(c->d_tk); (void)hipFree(c->d_tc); (void)hipFree(c->d_mk); (void)hipFree(c->d_mc);
        (void)hipFree(c->d_nk); (void)hipFree(c->d_nc);
        c->d_mk = nullptr; c->d_mc = nullptr; c->d_nk = nullptr; c->d_nc = nullptr;
        c->d_tk = tk; c->d_tc = tc; c->cap_table = std::min(ck, cc);
        size_t c1 = 0, c2 = 0, c3 = 0, c4 = 0;
        if (int r = grow(c, c->d_mk, c1, c->cap_table, "fingerprint table")) return r;
        if (int r = grow(c, c->d_mc, c2, c->cap_table, "fingerprint table")) return r;
        if (int r = grow(c, c->d_nk, c3, c->cap_table, "fingerprint table")) return r;
        if (int r = grow(c, c->d_nc, c4, c->cap_table, "fingerprint table")) return r;
    }
    if (T == 0) {
        FP_CK(hipMemcpyAsync(c->d_tk, c->d_uniq, runs * 8, hipMemcpyDeviceToDevice, c->stream), "hipMemcpyAsync");
        FP_CK(hipMemcpyAsync(c->d_tc, c->d_runc, runs * 4, hipMemcpyDeviceToDevice, c->stream), "hipMemcpyAsync");
        c->n_table = runs;
        return CL_OK;
    }
    tb = 0;
    FP_CK(rocprim::merge(nullptr, tb, c->d_tk, c->d_uniq, c->d_mk, c->d_tc, c->d_runc, c->d_mc, (size_t)T, (size_t)runs,
                         rocprim::less<uint64_t>(), c->stream), "merge");
    if (int r = tmp_need(c, tb)) return r;
    FP_CK(rocprim::merge(c->d_tmp, tb, c->d_tk, c->d_uniq, c->d_mk, c->d_tc, c->d_runc, c->d_mc, (size_t)T, (size_t)runs,
                         rocprim::less<uint64_t>(), c->stream), "merge");
    tb = 0;
    FP_CK(rocprim::reduce_by_key(nullptr, tb, c->d_mk, c->d_mc, (size_t)M, c->d_nk, c->d_nc, c->d_scal + 2, SumU32(),
                                 rocprim::equal_to<uint64_t>(), c->stream), "reduce_by_key");
    if (int r = tmp_need(c, tb)) return r;
    FP_CK(rocprim::reduce_by_key(c->d_tmp, tb, c->d_mk, c->d_mc, (size_t)M, c->d_nk, c->d_nc, c->d_scal + 2, SumU32(),
                                 rocprim::equal_to<uint64_t>(), c->stream), "reduce_by_key");
    FP_CK(hipMemcpyAsync(c->h_scal + 2, c->d_scal + 2, 4, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
    FP_CK(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    std::swap(c->d_tk, c->d_nk); std::swap(c->d_tc, c->d_nc);
    c->n_table = c->h_scal[2];
    return CL_OK;
}

// one batch: sequences [i0, i1) of the caller's arrays; SEQ4: nibble codes, else bytes
int push_batch(dut_fp_ctx *c, bool seq4, const uint8_t *data, const uint64_t *off, uint64_t i0, uint64_t i1)
{
    const uint32_t k = c->opt.ksize;
    const uint64_t n = i1 - i0;
    const uint64_t b0 = seq4 ? (off[i0] & ~1ull) : off[i0];      // first base of the upload (a whole byte for seq4)
    const uint64_t bases = off[i1] - b0;
    const size_t data_bytes = seq4 ? (size_t)((bases + 1) / 2) : (size_t)bases;
    // strips per sequence
    uint64_t n_strips = 0, n_win = 0;
    for (uint64_t i = i0; i < i1; ++i) {
        const uint64_t len = off[i + 1] - off[i];
        if (len < k) continue;
        c->processed += 1;
        n_win += len - k + 1;
        n_strips += (len - k + 1 + kStrip - 1) / kStrip;
    }
    if (n_strips == 0) return CL_OK;
    if (n_win > 0xFFFFFFFFull || n_strips > 0xFFFFFFFFull) { c->err = "batch too large"; return CL_ERR_RANGE; }
    // staging: data | off (n + 1, relative to b0) | strip_first (n + 1) | strip_seq (n_strips)
    const size_t o_off = (data_bytes + 7) & ~(size_t)7, o_sf = o_off + 8 * (n + 1), o_ss = o_sf + 4 * (n + 1);
    const size_t stage = o_ss + 4 * n_strips;
    if (stage > c->cap_stage) {
        if (c->h_stage) (void)hipHostFree(c->h_stage);
        c->h_stage = nullptr; c->cap_stage = 0;
        const size_t cap = std::max(stage, c->cap_stage + c->cap_stage / 2);
        FP_CK(hipHostMalloc((void **)&c->h_stage, cap, hipHostMallocDefault), "hipHostMalloc");
        c->cap_stage = cap;
    }
    uint8_t *st = c->h_stage;
    memcpy(st, data + (seq4 ? b0 / 2 : b0), data_bytes);
    uint64_t *h_off = (uint64_t *)(st + o_off);
    uint32_t *h_sf = (uint32_t *)(st + o_sf), *h_ss = (uint32_t *)(st + o_ss);
    uint32_t s_at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        h_off[i] = off[i0 + i] - b0;
        h_sf[i] = s_at;
        const uint64_t len = off[i0 + i + 1] - off[i0 + i];
        if (len >= k) {
            const uint32_t ns = (uint32_t)((len - k + 1 + kStrip - 1) / kStrip);
            for (uint32_t q = 0; q < ns; ++q) h_ss[s_at + q] = (uint32_t)i;
            s_at += ns;
        }
    }
    h_off[n] = off[i1] - b0;
    h_sf[n] = s_at;
    FP_GROW(c->d_data, c->cap_data, data_bytes + 8, "batch bases");
    FP_GROW(c->d_off, c->cap_off, n + 1, "batch offsets");
    FP_GROW(c->d_sfirst, c->cap_sfirst, n + 1, "batch strips");
    FP_GROW(c->d_sseq, c->cap_sseq, n_strips, "batch strips");
    if (n_win > c->cap_surv) {
        size_t c1 = c->cap_surv, c2 = c->cap_surv, c3 = c->cap_surv;
        FP_GROW(c->d_surv, c1, n_win, "batch survivors");
        FP_GROW(c->d_sorted, c2, n_win, "batch survivors");
        FP_GROW(c->d_uniq, c3, n_win, "batch survivors");
        c->cap_surv = std::min(c1, std::min(c2, c3));
    }
    FP_CK(hipEventRecord(c->ev[0], c->stream), "hipEventRecord");
    FP_CK(hipMemcpyAsync(c->d_data, st, data_bytes, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
    FP_CK(hipMemcpyAsync(c->d_off, h_off, 8 * (n + 1), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
    FP_CK(hipMemcpyAsync(c->d_sfirst, h_sf, 4 * (n + 1), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
    FP_CK(hipMemcpyAsync(c->d_sseq, h_ss, 4 * n_strips, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
    FP_CK(hipMemsetAsync(c->d_scal, 0, 16, c->stream), "hipMemsetAsync");
    FP_CK(hipEventRecord(c->ev[1], c->stream), "hipEventRecord");
    const uint32_t grid = (uint32_t)((n_strips + kBlock - 1) / kBlock);
    const bool wide = k > 32;
    if (seq4 && !wide) k_fp_hash<true, false><<<grid, kBlock, 0, c->stream>>>(c->d_data, c->d_off, c->d_sfirst, c->d_sseq, (uint32_t)n_strips, k, c->max_hash, c->d_surv, c->d_scal);
    else if (seq4) k_fp_hash<true, true><<<grid, kBlock, 0, c->stream>>>(c->d_data, c->d_off, c->d_sfirst, c->d_sseq, (uint32_t)n_strips, k, c->max_hash, c->d_surv, c->d_scal);
    else if (!wide) k_fp_hash<false, false><<<grid, kBlock, 0, c->stream>>>(c->d_data, c->d_off, c->d_sfirst, c->d_sseq, (uint32_t)n_strips, k, c->max_hash, c->d_surv, c->d_scal);
    else k_fp_hash<false, true><<<grid, kBlock, 0, c->stream>>>(c->d_data, c->d_off, c->d_sfirst, c->d_sseq, (uint32_t)n_strips, k, c->max_hash, c->d_surv, c->d_scal);
    FP_CK(hipGetLastError(), "k_fp_hash launch");
    FP_CK(hipEventRecord(c->ev[2], c->stream), "hipEventRecord");
    FP_CK(hipMemcpyAsync(c->h_scal, c->d_scal, 4, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
    FP_CK(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    const uint32_t ns = c->h_scal[0];
    if (ns) if (int r = reduce_batch(c, ns)) return r;
    FP_CK(hipEventRecord(c->ev[3], c->stream), "hipEventRecord");
    FP_CK(hipEventSynchronize(c->ev[3]), "hipEventSynchronize");
    float a = 0, b = 0, d = 0;
    FP_CK(hipEventElapsedTime(&a, c->ev[0], c->ev[1]), "hipEventElapsedTime");
    FP_CK(hipEventElapsedTime(&b, c->ev[1], c->ev[2]), "hipEventElapsedTime");
    FP_CK(hipEventElapsedTime(&d, c->ev[2], c->ev[3]), "hipEventElapsedTime");
    c->h2d_ms += a; c->hash_ms += b; c->reduce_ms += d;
    c->n_windows += n_win; c->n_batches += 1;
    return CL_OK;
}

int push(dut_fp_ctx *c, bool seq4, const uint8_t *data, const uint64_t *off, uint64_t n_seq)
{
    if (!c) return CL_ERR_INVALID;
    c->err.clear();
    if (n_seq == 0) return CL_OK;
    if (!data || !off) { c->err = "null sequence buffer or offsets"; return CL_ERR_INVALID; }
    // offsets: ascending (the kernel reads bases [off[i], off[i+1]) of the upload of [off[0], off[n_seq]) only)
    for (uint64_t i = 0; i < n_seq; ++i)
        if (off[i + 1] < off[i]) { c->err = "sequence offsets are not ascending at " + std::to_string(i); return CL_ERR_INVALID; }
    if (off[n_seq] - off[0] > (1ull << 46)) { c->err = "sequence offsets out of range"; return CL_ERR_INVALID; }
    FP_CK(hipSetDevice(c->device), "hipSetDevice");
    // batches of at most batch_bases bases (a longer sequence is a batch of its own)
    uint64_t i0 = 0;
    while (i0 < n_seq) {
        uint64_t i1 = i0 + 1;
        while (i1 < n_seq && off[i1 + 1] - off[i0] <= c->batch_bases) ++i1;
        if (off[i1] - off[i0] > kMaxBatchBases) { c->err = "a sequence of more than 2^30 bases"; return CL_ERR_RANGE; }
        if (int r = push_batch(c, seq4, data, off, i0, i1)) return r;
        i0 = i1;
    }
    return CL_OK;
}

} // namespace fp

extern "C" {

int dut_fp_create(const dut_fp_options *opt, int device_id, void *stream, dut_fp_ctx **out)
{
    if (!opt || !out) return CL_ERR_INVALID;
    *out = nullptr;
    if (opt->ksize < 1 || opt->ksize > 64) return CL_ERR_INVALID;
    dut_fp_ctx *c = new dut_fp_ctx();
    c->opt = *opt;
    c->max_hash = fp::max_hash(opt->scaled);
    c->device = device_id;
    if (const char *e = getenv("DUT_FP_BATCH_BASES")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v > 0) c->batch_bases = std::min<uint64_t>(v, fp::kMaxBatchBases);
    }
    auto fail = [&](hipError_t e, const char *what) { fp::dev_fail(c, e, what); dut_fp_destroy(c); return CL_ERR_DEVICE; };
    hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) return fail(e, "hipSetDevice");
    if (stream) c->stream = (hipStream_t)stream;
    else {
        if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
        c->own_stream = true;
    }
    for (auto &ev : c->ev) if ((e = hipEventCreate(&ev)) != hipSuccess) return fail(e, "hipEventCreate");
    if ((e = hipMalloc((void **)&c->d_scal, 16)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipHostMalloc((void **)&c->h_scal, 16, hipHostMallocDefault)) != hipSuccess) return fail(e, "hipHostMalloc");
    *out = c;
    return CL_OK;
}

int dut_fp_push_seq4(dut_fp_ctx *ctx, const uint8_t *seq4, const uint64_t *base_off, uint64_t n_seq)
{
    try { return fp::push(ctx, true, seq4, base_off, n_seq); }
    catch (const std::bad_alloc &) { return CL_ERR_NOMEM; }
}

int dut_fp_push_bytes(dut_fp_ctx *ctx, const uint8_t *bytes, const uint64_t *base_off, uint64_t n_seq)
{
    try { return fp::push(ctx, false, bytes, base_off, n_seq); }
    catch (const std::bad_alloc &) { return CL_ERR_NOMEM; }
}

int dut_fp_finish(dut_fp_ctx *c, dut_fp_result *out)
{
    if (!c || !out) return CL_ERR_INVALID;
    try {
        c->err.clear();
        FP_CK(hipSetDevice(c->device), "hipSetDevice");
        std::vector<uint64_t> h(c->n_table);
        std::vector<uint32_t> n(c->n_table);
        if (c->n_table) {
            FP_CK(hipMemcpyAsync(h.data(), c->d_tk, 8 * c->n_table, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
            FP_CK(hipMemcpyAsync(n.data(), c->d_tc, 4 * c->n_table, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
        }
        FP_CK(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        c->out_h.clear(); c->out_c.clear();
        for (size_t i = 0; i < h.size(); ++i)
            if (!c->opt.has_max_frequency || n[i] <= c->opt.max_frequency) { c->out_h.push_back(h[i]); c->out_c.push_back(n[i]); }
        out->processed = c->processed;
        out->n_distinct = c->n_table;
        out->n_entries = c->out_h.size();
        out->hashes = c->out_h.data();
        out->counts = c->out_c.data();
        fp::hexdigest(c->out_h, c->out_c, out->hexdigest);
        return CL_OK;
    } catch (const std::bad_alloc &) { c->err = "out of host memory"; return CL_ERR_NOMEM; }
}

void dut_fp_destroy(dut_fp_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void *bufs[] = {c->d_data, c->d_off, c->d_sfirst, c->d_sseq, c->d_surv, c->d_sorted, c->d_uniq, c->d_runc, c->d_scal,
                    c->d_tmp, c->d_tk, c->d_mk, c->d_nk, c->d_tc, c->d_mc, c->d_nc};
    for (void *p : bufs) if (p) (void)hipFree(p);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_scal) (void)hipHostFree(c->h_scal);
    for (auto &ev : c->ev) if (ev) (void)hipEventDestroy(ev);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *dut_fp_last_error(const dut_fp_ctx *c) { return c ? c->err.c_str() : "null context"; }

// device times of the pushes so far (ms from events): upload, hash kernel, sort + reduce + merge
int dut_fp_stats(const dut_fp_ctx *c, double *h2d_ms, double *hash_ms, double *reduce_ms, uint64_t *n_windows, uint64_t *n_batches)
{
    if (!c) return CL_ERR_INVALID;
    if (h2d_ms) *h2d_ms = c->h2d_ms;
    if (hash_ms) *hash_ms = c->hash_ms;
    if (reduce_ms) *reduce_ms = c->reduce_ms;
    if (n_windows) *n_windows = c->n_windows;
    if (n_batches) *n_batches = c->n_batches;
    return CL_OK;
}

// ---- host-only ----
uint64_t dut_fp_max_hash(uint64_t scaled) { return fp::max_hash(scaled); }

void dut_fp_sha256(const uint8_t *data, size_t len, uint8_t out32[32])
{
    fp::Sha256 s;
    s.update(data, len);
    s.final(out32);
}

} // extern "C"

namespace {

// the kernel's strips, walked one after the other
template <class Src>
int kmer_hashes_host(const Src &src, uint64_t len, uint32_t k, uint64_t *out, uint8_t *has_n)
{
    if (k < 1 || k > 64) return CL_ERR_INVALID;
    if (len < k) return CL_OK;
    if (!src.p || !out || !has_n) return CL_ERR_INVALID;
    const uint64_t nw = len - k + 1;
    for (uint64_t w = 0; w < nw; w += fp::kStrip) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(fp::kStrip, nw - w);
        auto emit = [&](bool in_range, bool hn, uint64_t h, uint32_t wi) {
            if (!in_range) return;
            out[w + wi] = hn ? 0 : h;
            has_n[w + wi] = hn ? 1 : 0;
        };
        if (k <= 32) fp::strip_walk<false>(src, w, n, k, k - 1 + n, emit);
        else fp::strip_walk<true>(src, w, n, k, k - 1 + n, emit);
    }
    return CL_OK;
}

} // namespace

extern "C" {

int dut_fp_kmer_hashes_host(const uint8_t *bytes, uint64_t len, uint32_t k, uint64_t *out, uint8_t *has_n)
{
    return kmer_hashes_host(fp::SrcBytes{bytes}, len, k, out, has_n);
}

int dut_fp_kmer_hashes_host_seq4(const uint8_t *seq4, uint64_t len, uint32_t k, uint64_t *out, uint8_t *has_n)
{
    return kmer_hashes_host(fp::SrcSeq4{seq4}, len, k, out, has_n);
}

int dut_fp_input_kind(const char *input, char *err, size_t err_len)
{
    auto set = [&](const char *m) { if (err && err_len) snprintf(err, err_len, "%s", m); };
    if (!input) { set("null path"); return CL_ERR_INVALID; }
    // Path::extension: the part after the last '.' of the file name, none for a name that starts with its only '.'
    std::string p(input);
    const size_t slash = p.find_last_of('/');
    const std::string name = slash == std::string::npos ? p : p.substr(slash + 1);
    const size_t dot = name.find_last_of('.');
    const std::string ext = (dot == std::string::npos || dot == 0) ? "" : name.substr(dot + 1);
    if (ext == "bam") return 1;
    if (ext == "fastq" || ext == "fq" || ext == "gz") return 2;
    if (ext == "cram") { set("CRAM is not supported: convert the file to BAM (samtools view -b)"); return CL_ERR_INVALID; }
    if (ext == "gam") { set("GAM input is not supported"); return CL_ERR_INVALID; }
    set("Unsupported file format. Must be .fastq, .fq, .fastq.gz, .fq.gz, .bam, or .cram");
    return CL_ERR_INVALID;
}

} // extern "C"

namespace {

// one batch of the reader, copied out of the reader's buffers (the reader refills them while this one is hashed)
struct Batch {
    std::vector<uint8_t> data;
    std::vector<uint64_t> off;
    uint64_t n = 0;
    int rc = CL_OK;
    double decode_ms = 0;
};

int fp_files_impl(const char *input, const char *output, const dut_fp_options *opt, const char *region, int device_id,
                  char *digest_out, uint64_t *processed_out, char *err, size_t err_len)
{
    auto set = [&](const std::string &m) { if (err && err_len) snprintf(err, err_len, "%s", m.c_str()); };
    if (!opt || !input) { set("null argument"); return CL_ERR_INVALID; }
    if (opt->ksize < 1 || opt->ksize > 64) { set("ksize must be in 1..64"); return CL_ERR_INVALID; }
    const int kind = dut_fp_input_kind(input, err, err_len);
    if (kind < 0) return kind;
    const bool seq4 = kind == 1;
    dut_bam *bam = nullptr;
    dut_fastq *fq = nullptr;
    char e2[512] = {0};
    if (seq4) bam = dut_bam_open(input, e2, sizeof(e2));
    else fq = dut_fastq_open(input, e2, sizeof(e2));
    if (!bam && !fq) { set(std::string("Failed to open ") + input + ": " + e2); return CL_ERR_INVALID; }
    uint64_t cap = fp::kDefaultBatchBases;
    if (const char *e = getenv("DUT_FP_BATCH_BASES")) { const unsigned long long v = strtoull(e, nullptr, 10); if (v) cap = std::min<uint64_t>(v, fp::kMaxBatchBases); }
    auto read_batch = [&](Batch &b) {
        const double t0 = dut::now_s();
        uint64_t n = 0; const uint64_t *off = nullptr; const uint8_t *d = nullptr;
        b.rc = seq4 ? dut_bam_next_seqs(bam, cap, &n, &off, &d) : dut_fastq_next(fq, cap, &n, &off, &d);
        b.n = 0;
        if (b.rc == CL_OK && n) {
            b.n = n;
            b.off.assign(off, off + n + 1);
            const size_t bytes = seq4 ? (size_t)((off[n] + 1) / 2) : (size_t)off[n];
            b.data.assign(d, d + bytes);
            if (b.data.empty()) b.data.push_back(0);
        }
        b.decode_ms = (dut::now_s() - t0) * 1e3;
    };
    auto close_readers = [&]() { if (bam) dut_bam_close(bam); if (fq) dut_fastq_close(fq); };
    dut_fp_ctx *ctx = nullptr;
    int rc = dut_fp_create(opt, device_id, nullptr, &ctx);
    if (rc != CL_OK) { set(ctx ? dut_fp_last_error(ctx) : "cannot create the fingerprint context on the device"); close_readers(); return rc; }
    Batch cur, next;
    read_batch(cur);
    const bool timing = dut::timing_on();
    uint64_t bi = 0;
    while (rc == CL_OK) {
        if (cur.rc != CL_OK) { rc = cur.rc; set(std::string("reading ") + input + ": " + (bam ? dut_bam_error(bam) : "read failed")); break; }
        if (cur.n == 0) break;
        // decode of the next batch on a second thread while this one is hashed on the device
        std::thread th([&]() { read_batch(next); });
        const double t0 = dut::now_s();
        double hash0 = ctx->hash_ms + ctx->reduce_ms + ctx->h2d_ms;
        rc = seq4 ? dut_fp_push_seq4(ctx, cur.data.data(), cur.off.data(), cur.n) : dut_fp_push_bytes(ctx, cur.data.data(), cur.off.data(), cur.n);
        const double push_ms = (dut::now_s() - t0) * 1e3;
        th.join();
        if (timing)
            fprintf(stderr, "[dut-timing] fingerprint batch %llu: %llu sequences, host decode %.2f ms, device %.2f ms (push call %.2f ms)\n",
                    (unsigned long long)bi, (unsigned long long)cur.n, cur.decode_ms,
                    ctx->hash_ms + ctx->reduce_ms + ctx->h2d_ms - hash0, push_ms);
        if (rc != CL_OK) { set(dut_fp_last_error(ctx)); break; }
        std::swap(cur, next);
        ++bi;
    }
    dut_fp_result res{};
    if (rc == CL_OK && (rc = dut_fp_finish(ctx, &res)) != CL_OK) set(dut_fp_last_error(ctx));
    close_readers();
    if (rc == CL_OK) {
        if (digest_out) memcpy(digest_out, res.hexdigest, 65);
        if (processed_out) *processed_out = res.processed;
        if (output) {
            FILE *f = fopen(output, "wb");
            if (!f) { set(std::string("Failed to create output file ") + output); rc = CL_ERR_INVALID; }
            else {
                std::string s;
                s.reserve(1 << 20);
                s += "#ksize=" + std::to_string(opt->ksize) + "\n#scaled=" + std::to_string(opt->scaled) + "\n#region=" +
                     std::string(region ? region : "full") + "\n";
                if (opt->has_max_frequency) s += "#max_frequency=" + std::to_string(opt->max_frequency) + "\n";
                for (uint64_t i = 0; i < res.n_entries; ++i) {
                    s += std::to_string(res.hashes[i]); s += '\t'; s += std::to_string(res.counts[i]); s += '\n';
                    if (s.size() > (1u << 20)) { fwrite(s.data(), 1, s.size(), f); s.clear(); }
                }
                const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
                if (fclose(f) != 0 || !ok) { set(std::string("Failed to write ") + output); rc = CL_ERR_INVALID; }
            }
        }
    }
    dut_fp_destroy(ctx);
    return rc;
}

} // namespace

extern "C" int dut_fp_files(const char *input, const char *reference, const char *output, const dut_fp_options *opt,
                            const char *region, int device_id, char *digest_out, uint64_t *processed_out, char *err, size_t err_len)
{
    (void)reference;
    try { return fp_files_impl(input, output, opt, region, device_id, digest_out, processed_out, err, err_len); }
    catch (const std::bad_alloc &) { if (err && err_len) snprintf(err, err_len, "out of host memory"); return CL_ERR_NOMEM; }
}
