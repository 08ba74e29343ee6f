// fingerprint_compare.hip -- fingerprint-compare (include/dut_fingerprint.h, dut_fpc_*): a set of sketches resident on
// the device and, for any list of pairs, what the two sketches share.
//
// The hashes (u64) and the counts (u32) of all added sketches lie concatenated in two device arrays, 12 bytes per entry.
// One compare is k_fpc_tiles over a flat list of tiles followed by k_fpc_sum over the pairs.  The merged sequence of a
// pair (n_a + n_b elements within the cut, ties A first) is cut every kTile elements by merge-path diagonals, so a
// workgroup always owns kTile merged elements, whatever the two sizes are.  A workgroup finds its pair in the prefix of
// tile counts, its two diagonals by a wave-wide search (64 probes a round), stages its stretch of B (hashes and counts) plus ONE look-ahead element
// in LDS, and looks every A element of its stretch up in that image.
//
// The seam rule: with ties A first, the partner of an A element is the element right behind it in the merged order
// (hashes within a sketch are distinct, so nothing can stand between the two).  It is therefore in the A element's own
// tile or is the first B element of the next one -- the look-ahead element.  A match belongs to the tile of its A
// element, which is exactly one tile, so no match is counted twice or dropped.  sum_a / sum_b shares are over the
// stretches proper (the look-ahead element's count belongs to the next tile).
//
// Accumulation: every tile stores one 32-byte partial; k_fpc_sum adds the partials of a pair with one wave and writes the
// record.  No atomics: several thousand tiles of one pair run at once and would all add into the same four words.
#include <hip/hip_runtime.h>

#include "fp_compare.h"
#include "host_parallel.h"

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace fpc {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kTile = 2048;                 // merged elements per tile
// one launch: gridDim.x * blockDim.x stays below 2^32 and gridDim.y at or below 65 535, so the tiles of a call are laid out in rows
constexpr uint32_t kMaxGridX = (1u << 24) - 1, kMaxGridY = 65535;
constexpr uint32_t kDefaultGridX = 1u << 22;
static_assert((uint64_t)kMaxGridX * kBlock < (1ull << 32) && (uint64_t)DUT_FPC_MAX_TILES <= (uint64_t)kMaxGridX * kMaxGridY, "every accepted tile count fits one launch");
constexpr uint32_t kPer = kTile / kBlock;        // elements of A a thread may own
constexpr uint32_t kGroup = 4;                   // searches a thread runs side by side
static_assert(kPer % kGroup == 0, "groups of searches");

struct Pair {                                    // one compared pair on the device
    uint64_t a_off, b_off;                       // first entry of each sketch in the concatenated arrays
    uint32_t n_a, n_b;                           // entries within the cut
};
struct Partial { uint64_t common, sum_min, sum_a, sum_b; };

// The first index of [lo, hi) at which pred is false (hi when there is none), for a pred that is true up to some index and
// false from there on: one wave, 64 probes a round, so a range of 2^24 takes four dependent loads and not twenty-four
// (a tile's searches are latency it cannot hide behind its own work).  pred is called with indices of [lo, hi) only.
template <class Pred>
__device__ __forceinline__ uint32_t wave_first_false(uint32_t lo, uint32_t hi, uint32_t lane, Pred pred)
{
    while (lo < hi) {
        const uint32_t step = (hi - lo + 63u) >> 6;
        const uint64_t at = (uint64_t)lo + (uint64_t)lane * step;          // (64-bit: lane * step may pass hi by far)
        const uint32_t k = (uint32_t)__popcll(__ballot(at < hi && pred((uint32_t)at)));   // the probes that hold: a prefix of the lanes
        if (k == 0) return lo;
        hi = (uint32_t)std::min<uint64_t>(hi, (uint64_t)lo + (uint64_t)k * step);         // the first probe that fails, if it is inside
        lo = lo + (k - 1) * step + 1;                                     // behind the last probe that holds
    }
    return lo;
}

// number of A elements among the first d merged elements (ties A first); d <= n_a + n_b
__device__ __forceinline__ uint32_t merge_path(const uint64_t *__restrict__ A, uint32_t n_a, const uint64_t *__restrict__ B,
                                               uint32_t n_b, uint32_t d, uint32_t lane)
{
    // i in [max(0, d - n_b), min(d, n_a)): i < n_a and d - 1 - i in [0, n_b)
    return wave_first_false(d > n_b ? d - n_b : 0u, d < n_a ? d : n_a, lane, [&](uint32_t i) { return A[i] <= B[d - 1 - i]; });
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((unsigned long long)v, o);
    return v;
}

// tile_start: n_pairs + 1 ascending tile indices (tile_start[n_pairs] = n_tiles); pairs without entries have no tile
__global__ __launch_bounds__(kBlock) void k_fpc_tiles(const uint64_t *__restrict__ hashes, const uint32_t *__restrict__ counts,
                                                      const Pair *__restrict__ pairs, const uint32_t *__restrict__ tile_start,
                                                      uint32_t n_pairs, uint32_t n_tiles, Partial *__restrict__ partials)
{
    __shared__ uint64_t s_h[kTile + 1];
    __shared__ uint32_t s_c[kTile + 1];
    __shared__ uint32_t s_diag[2];
    __shared__ uint64_t s_red[kBlock / 64][4];
    // the grid is rows of gridDim.x tiles (a launch takes fewer than 2^24 workgroups of 256 threads in x); the last row may
    // be short, and its spare workgroups leave as a whole before any barrier
    const uint32_t tile = blockIdx.y * gridDim.x + blockIdx.x, tid = threadIdx.x;
    if (tile >= n_tiles) return;
    // the pair: the last p with tile_start[p] <= tile (tile_start[0] = 0: there is one); every wave finds it for itself
    const uint32_t lo = wave_first_false(0u, n_pairs, tid & 63u, [&](uint32_t p) { return tile_start[p] <= tile; }) - 1u;
    const Pair pr = pairs[lo];
    const uint32_t t = tile - tile_start[lo];
    const uint64_t *__restrict__ A = hashes + pr.a_off, *__restrict__ B = hashes + pr.b_off;
    const uint32_t *__restrict__ CA = counts + pr.a_off, *__restrict__ CB = counts + pr.b_off;
    const uint64_t total = (uint64_t)pr.n_a + pr.n_b;
    const uint32_t d0 = t * kTile;                           // < total < 2^32: dut_fpc_add keeps every sketch below 2^31 entries
    const uint32_t d1 = (uint32_t)std::min<uint64_t>((uint64_t)d0 + kTile, total);
    if (tid < 128u) {                                        // wave 0: the tile's first diagonal, wave 1: its last
        const uint32_t a = merge_path(A, pr.n_a, B, pr.n_b, tid < 64u ? d0 : d1, tid & 63u);
        if ((tid & 63u) == 0) s_diag[tid >> 6] = a;
    }
    __syncthreads();
    const uint32_t a0 = s_diag[0], a1 = s_diag[1], b0 = d0 - a0, b1 = d1 - a1;
    const uint32_t nb = b1 - b0;                             // <= kTile
    const uint32_t nbl = nb + (b1 < pr.n_b ? 1u : 0u);       // with the look-ahead element: <= kTile + 1
    // every load of the tile is asked for before the first is waited for: a thread's kPer elements of A into registers, then
    // the stretch of B, which goes on into LDS (a tile has too little work of its own to hide one load behind the next)
    uint64_t xa[kPer];
    uint32_t ca[kPer];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = a0 + tid + k * kBlock;
        const bool in = i < a1;
        xa[k] = in ? A[i] : 0ull;
        ca[k] = in ? CA[i] : 0u;                             // (0: nothing for sum_a, and no match below)
    }
    uint64_t hb[kPer + 1];                                   // nbl <= kTile + 1: the last round is the look-ahead element's
    uint32_t cb[kPer + 1];
#pragma unroll
    for (uint32_t k = 0; k < kPer + 1; ++k) {
        const uint32_t i = tid + k * kBlock;
        const bool in = i < nbl;
        hb[k] = in ? B[b0 + i] : 0ull;
        cb[k] = in ? CB[b0 + i] : 0u;
    }
    uint64_t sum_b = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPer + 1; ++k) {
        const uint32_t i = tid + k * kBlock;
        if (i < nbl) { s_h[i] = hb[k]; s_c[i] = cb[k]; }
        if (i < nb) sum_b += cb[k];
    }
    __syncthreads();
    uint64_t common = 0, sum_min = 0, sum_a = 0;
    // kGroup searches side by side, so that kGroup LDS reads are in flight at every step; a group beyond the stretch of A
    // is skipped by the whole workgroup
    for (uint32_t g = 0; g < kPer && a0 + g * kBlock < a1; g += kGroup) {
        uint32_t at[kGroup];
#pragma unroll
        for (uint32_t j = 0; j < kGroup; ++j) at[j] = 0;
        // the last staged element <= x, if any (the trip count depends on nbl only: no divergence)
        for (uint32_t n = nbl; n > 1;) {
            const uint32_t half = n >> 1;
#pragma unroll
            for (uint32_t j = 0; j < kGroup; ++j) if (s_h[at[j] + half] <= xa[g + j]) at[j] += half;
            n -= half;
        }
#pragma unroll
        for (uint32_t j = 0; j < kGroup; ++j) {
            const uint32_t c = ca[g + j];
            sum_a += c;
            if (c && nbl && s_h[at[j]] == xa[g + j]) {
                common += 1;
                sum_min += std::min(c, s_c[at[j]]);
            }
        }
    }
    common = wave_sum(common); sum_min = wave_sum(sum_min); sum_a = wave_sum(sum_a); sum_b = wave_sum(sum_b);
    if ((tid & 63u) == 0) {
        s_red[tid >> 6][0] = common; s_red[tid >> 6][1] = sum_min; s_red[tid >> 6][2] = sum_a; s_red[tid >> 6][3] = sum_b;
    }
    __syncthreads();
    if (tid == 0) {
        Partial p = {0, 0, 0, 0};
        for (uint32_t w = 0; w < kBlock / 64; ++w) {
            p.common += s_red[w][0]; p.sum_min += s_red[w][1]; p.sum_a += s_red[w][2]; p.sum_b += s_red[w][3];
        }
        partials[tile] = p;
    }
}

// one wave per pair: the partials of its tiles, added in a fixed order, and the record
__global__ __launch_bounds__(64) void k_fpc_sum(const Partial *__restrict__ partials, const Pair *__restrict__ pairs,
                                                const uint32_t *__restrict__ tile_start, dut_fpc_record *__restrict__ out)
{
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    const uint32_t t0 = tile_start[p], t1 = tile_start[p + 1];
    uint64_t common = 0, sum_min = 0, sum_a = 0, sum_b = 0;
    for (uint32_t t = t0 + lane; t < t1; t += 64) {
        const Partial q = partials[t];
        common += q.common; sum_min += q.sum_min; sum_a += q.sum_a; sum_b += q.sum_b;
    }
    common = wave_sum(common); sum_min = wave_sum(sum_min); sum_a = wave_sum(sum_a); sum_b = wave_sum(sum_b);
    if (lane == 0) {
        dut_fpc_record r;
        r.n_a = pairs[p].n_a; r.n_b = pairs[p].n_b; r.n_common = common;
        r.sum_a = sum_a; r.sum_b = sum_b; r.sum_min = sum_min;
        out[p] = r;
    }
}

// entries of sketch q_off[i] .. + q_n[i] with hash <= q_cut[i]: one thread per query (a cut below the sketch's own max_hash)
__global__ __launch_bounds__(64) void k_fpc_cut(const uint64_t *__restrict__ hashes, const uint64_t *__restrict__ q_off,
                                                const uint32_t *__restrict__ q_n, const uint64_t *__restrict__ q_cut,
                                                uint32_t n_q, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_q) return;
    const uint64_t *h = hashes + q_off[i];
    const uint64_t cut = q_cut[i];
    uint32_t lo = 0, hi = q_n[i];                           // first index with h > cut
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (h[mid] <= cut) lo = mid + 1; else hi = mid;
    }
    out[i] = lo;
}

struct Meta {                                    // one added sketch
    uint32_t ksize;
    uint64_t scaled, max_hash, off, n;
    std::map<uint64_t, uint32_t> cut_len;        // entries within a cut below max_hash, once asked for
};

} // namespace fpc

struct dut_fpc_ctx {
    int device = 0;
    bool host_only = false;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    std::vector<fpc::Meta> sk;
    uint64_t n_entries = 0;
    // device: the concatenated sketches (grow together), the tables of one compare (grow-only)
    uint64_t *d_hashes = nullptr; uint32_t *d_counts = nullptr; size_t cap_entries = 0;
    uint8_t *d_tab = nullptr; size_t cap_tab = 0;                 // pairs | tile_start, or the cut queries
    fpc::Partial *d_part = nullptr; size_t cap_part = 0;
    dut_fpc_record *d_rec = nullptr; size_t cap_rec = 0;
    uint8_t *h_tab = nullptr; size_t cap_htab = 0;                // pinned staging of d_tab
    hipEvent_t ev[2] = {};
    std::vector<dut_fpc_record> out;
    std::vector<uint32_t> all_a, all_b;
    uint32_t grid_x = fpc::kDefaultGridX;                       // tiles per grid row (DUT_FPC_GRID_X: for the tests of the row layout)
    double kernel_ms = 0;
    uint64_t n_tiles = 0, bytes = 0;
};

namespace fpc {

int fail(dut_fpc_ctx *c, int rc, const std::string &m) { c->err = m; return rc; }
int dev_fail(dut_fpc_ctx *c, hipError_t e, const char *what)
{
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? CL_ERR_NOMEM : CL_ERR_DEVICE;
}
#define FPC_CK(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fpc::dev_fail(c, e_, what); } while (0)

template <class T>
int grow(dut_fpc_ctx *c, T *&p, size_t &cap, size_t need, const char *what)
{
    if (need <= cap) return CL_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    const hipError_t e = hipMalloc((void **)&p, need * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        return fail(c, CL_ERR_NOMEM, std::string("device memory exhausted: ") + what + " of " + std::to_string(need) + " entries does not fit");
    }
    cap = need;
    return CL_OK;
}

int stage(dut_fpc_ctx *c, size_t bytes)
{
    if (int r = grow(c, c->d_tab, c->cap_tab, bytes, "pair table")) return r;
    if (bytes > c->cap_htab) {
        if (c->h_tab) (void)hipHostFree(c->h_tab);
        c->h_tab = nullptr; c->cap_htab = 0;
        FPC_CK(hipHostMalloc((void **)&c->h_tab, bytes, hipHostMallocDefault), "hipHostMalloc");
        c->cap_htab = bytes;
    }
    return CL_OK;
}

// room for `more` further entries; the resident sketches are carried over
int reserve(dut_fpc_ctx *c, uint64_t more)
{
    const uint64_t need = c->n_entries + more;
    if (need <= c->cap_entries) return CL_OK;
    const size_t cap = (size_t)std::max<uint64_t>(need, c->cap_entries + c->cap_entries / 2);
    uint64_t *h = nullptr; uint32_t *n = nullptr;
    for (size_t want : {cap, (size_t)need}) {
        if (hipMalloc((void **)&h, want * 8) == hipSuccess) {
            if (hipMalloc((void **)&n, want * 4) == hipSuccess) {
                if (c->n_entries) {
                    hipError_t e = hipMemcpyAsync(h, c->d_hashes, c->n_entries * 8, hipMemcpyDeviceToDevice, c->stream);
                    if (e == hipSuccess) e = hipMemcpyAsync(n, c->d_counts, c->n_entries * 4, hipMemcpyDeviceToDevice, c->stream);
                    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
                    if (e != hipSuccess) { (void)hipFree(h); (void)hipFree(n); return dev_fail(c, e, "carrying the sketches over"); }
                }
                if (c->d_hashes) (void)hipFree(c->d_hashes);
                if (c->d_counts) (void)hipFree(c->d_counts);
                c->d_hashes = h; c->d_counts = n; c->cap_entries = want;
                return CL_OK;
            }
            (void)hipFree(h); h = nullptr;
        }
        (void)hipGetLastError();
    }
    return fail(c, CL_ERR_NOMEM, "device memory exhausted: a sketch set of " + std::to_string(need) + " entries does not fit");
}

// the pair list of one call, checked: "" or the refusal.  cut[p] = min of the two max_hash values.
std::string check_pairs(const std::vector<Meta> &sk, const uint32_t *pa, const uint32_t *pb, uint64_t n_pairs)
{
    if (n_pairs > DUT_FPC_MAX_PAIRS) return std::to_string(n_pairs) + " pairs: more than DUT_FPC_MAX_PAIRS (" + std::to_string(DUT_FPC_MAX_PAIRS) + ")";
    if (!pa || !pb) return "null pair arrays";
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (pa[p] >= sk.size() || pb[p] >= sk.size())
            return "pair " + std::to_string(p) + " (" + std::to_string(pa[p]) + ", " + std::to_string(pb[p]) + "): an id out of range (" + std::to_string(sk.size()) + " sketches)";
        if (sk[pa[p]].ksize != sk[pb[p]].ksize)
            return "pair " + std::to_string(p) + " (" + std::to_string(pa[p]) + ", " + std::to_string(pb[p]) + "): ksize " +
                   std::to_string(sk[pa[p]].ksize) + " against ksize " + std::to_string(sk[pb[p]].ksize);
    }
    return "";
}

// the prefix lengths within cuts below a sketch's own max_hash that no earlier call has asked for, by one small launch
int resolve_cuts(dut_fpc_ctx *c, const uint32_t *pa, const uint32_t *pb, uint64_t n_pairs)
{
    std::vector<std::pair<uint32_t, uint64_t>> q;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const uint64_t cut = std::min(c->sk[pa[p]].max_hash, c->sk[pb[p]].max_hash);
        for (uint32_t id : {pa[p], pb[p]}) {
            Meta &m = c->sk[id];
            if (cut < m.max_hash && m.n && m.cut_len.emplace(cut, 0xFFFFFFFFu).second) q.emplace_back(id, cut);
        }
    }
    if (q.empty()) return CL_OK;
    auto forget = [&]() { for (auto &e : q) c->sk[e.first].cut_len.erase(e.second); };
    const size_t nq = q.size(), o_n = 8 * nq, o_cut = (o_n + 4 * nq + 7) & ~(size_t)7, o_out = o_cut + 8 * nq, bytes = o_out + 4 * nq;
    if (int r = stage(c, bytes)) { forget(); return r; }
    uint64_t *off = (uint64_t *)c->h_tab, *cut = (uint64_t *)(c->h_tab + o_cut);
    uint32_t *n = (uint32_t *)(c->h_tab + o_n), *res = (uint32_t *)(c->h_tab + o_out);
    for (size_t i = 0; i < nq; ++i) { off[i] = c->sk[q[i].first].off; n[i] = (uint32_t)c->sk[q[i].first].n; cut[i] = q[i].second; }
    hipError_t e = hipMemcpyAsync(c->d_tab, c->h_tab, o_out, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        k_fpc_cut<<<(uint32_t)((nq + 63) / 64), 64, 0, c->stream>>>(c->d_hashes, (const uint64_t *)c->d_tab, (const uint32_t *)(c->d_tab + o_n),
                                                                   (const uint64_t *)(c->d_tab + o_cut), (uint32_t)nq, (uint32_t *)(c->d_tab + o_out));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(res, c->d_tab + o_out, 4 * nq, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { forget(); return dev_fail(c, e, "k_fpc_cut"); }
    for (size_t i = 0; i < nq; ++i) c->sk[q[i].first].cut_len[q[i].second] = res[i];
    return CL_OK;
}

int compare(dut_fpc_ctx *c, const uint32_t *pa, const uint32_t *pb, uint64_t n_pairs, const dut_fpc_record **out)
{
    if (!c) return CL_ERR_INVALID;
    c->err.clear();
    if (!out) return fail(c, CL_ERR_INVALID, "null out");
    *out = nullptr;
    if (c->host_only) return fail(c, CL_ERR_DEVICE, "a host-only context has no device");
    c->out.clear();
    c->kernel_ms = 0; c->n_tiles = 0; c->bytes = 0;
    if (n_pairs == 0) return CL_OK;
    const std::string bad = check_pairs(c->sk, pa, pb, n_pairs);
    if (!bad.empty()) return fail(c, CL_ERR_INVALID, bad);
    FPC_CK(hipSetDevice(c->device), "hipSetDevice");
    if (int r = resolve_cuts(c, pa, pb, n_pairs)) return r;
    // tiles per pair, counted before anything is allocated
    auto len_in = [&](uint32_t id, uint64_t cut) -> uint32_t {
        const Meta &m = c->sk[id];
        return cut < m.max_hash && m.n ? m.cut_len.at(cut) : (uint32_t)m.n;
    };
    uint64_t n_tiles = 0, bytes = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const uint64_t cut = std::min(c->sk[pa[p]].max_hash, c->sk[pb[p]].max_hash);
        const uint64_t m = (uint64_t)len_in(pa[p], cut) + len_in(pb[p], cut);
        n_tiles += (m + kTile - 1) / kTile;
        bytes += 12 * m;
    }
    if (n_tiles > DUT_FPC_MAX_TILES)
        return fail(c, CL_ERR_INVALID, std::to_string(n_tiles) + " tiles: more than one call's " + std::to_string(DUT_FPC_MAX_TILES) + " (split the pair list)");
    const size_t o_ts = sizeof(Pair) * n_pairs, tab_bytes = o_ts + 4 * (n_pairs + 1);
    if (int r = stage(c, tab_bytes)) return r;
    if (int r = grow(c, c->d_part, c->cap_part, (size_t)std::max<uint64_t>(n_tiles, 1), "tile partials")) return r;
    if (int r = grow(c, c->d_rec, c->cap_rec, (size_t)n_pairs, "pair records")) return r;
    Pair *hp = (Pair *)c->h_tab;
    uint32_t *ts = (uint32_t *)(c->h_tab + o_ts);
    uint32_t at = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const uint64_t cut = std::min(c->sk[pa[p]].max_hash, c->sk[pb[p]].max_hash);
        hp[p] = Pair{c->sk[pa[p]].off, c->sk[pb[p]].off, len_in(pa[p], cut), len_in(pb[p], cut)};
        ts[p] = at;
        at += (uint32_t)(((uint64_t)hp[p].n_a + hp[p].n_b + kTile - 1) / kTile);
    }
    ts[n_pairs] = at;
    c->out.resize(n_pairs);
    FPC_CK(hipMemcpyAsync(c->d_tab, c->h_tab, tab_bytes, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
    FPC_CK(hipEventRecord(c->ev[0], c->stream), "hipEventRecord");
    const Pair *dp = (const Pair *)c->d_tab;
    const uint32_t *dts = (const uint32_t *)(c->d_tab + o_ts);
    if (n_tiles) {
        // rows of at most grid_x tiles, and at most kMaxGridY of them: n_tiles <= DUT_FPC_MAX_TILES keeps gx below kMaxGridX
        const uint64_t gx = std::min<uint64_t>(n_tiles, std::max<uint64_t>(c->grid_x, (n_tiles + kMaxGridY - 1) / kMaxGridY));
        const dim3 grid((uint32_t)gx, (uint32_t)((n_tiles + gx - 1) / gx));
        k_fpc_tiles<<<grid, kBlock, 0, c->stream>>>(c->d_hashes, c->d_counts, dp, dts, (uint32_t)n_pairs, (uint32_t)n_tiles, c->d_part);
        FPC_CK(hipGetLastError(), "k_fpc_tiles launch");
    }
    k_fpc_sum<<<(uint32_t)n_pairs, 64, 0, c->stream>>>(c->d_part, dp, dts, c->d_rec);
    FPC_CK(hipGetLastError(), "k_fpc_sum launch");
    FPC_CK(hipEventRecord(c->ev[1], c->stream), "hipEventRecord");
    FPC_CK(hipMemcpyAsync(c->out.data(), c->d_rec, sizeof(dut_fpc_record) * n_pairs, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
    FPC_CK(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    float ms = 0;
    FPC_CK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]), "hipEventElapsedTime");
    c->kernel_ms = ms; c->n_tiles = n_tiles; c->bytes = bytes;
    *out = c->out.data();
    return CL_OK;
}

int add(dut_fpc_ctx *c, uint32_t ksize, uint64_t scaled, const uint64_t *hashes, const uint32_t *counts, uint64_t n, uint32_t *id)
{
    if (!c) return CL_ERR_INVALID;
    c->err.clear();
    if (!id) return fail(c, CL_ERR_INVALID, "null id");
    const std::string bad = validate(ksize, scaled, hashes, counts, n);
    if (!bad.empty()) return fail(c, CL_ERR_INVALID, bad);
    // a tile's diagonals are 32-bit: the two prefixes of any pair stay below 2^32 together
    if (n > 0x7FFFFFFFull) return fail(c, CL_ERR_RANGE, "a sketch of more than 2^31 - 1 entries");
    if (c->sk.size() >= 0xFFFFFFFFull) return fail(c, CL_ERR_RANGE, "too many sketches");
    if (!c->host_only && n) {
        FPC_CK(hipSetDevice(c->device), "hipSetDevice");
        if (int r = reserve(c, n)) return r;
        FPC_CK(hipMemcpyAsync(c->d_hashes + c->n_entries, hashes, n * 8, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
        FPC_CK(hipMemcpyAsync(c->d_counts + c->n_entries, counts, n * 4, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
        FPC_CK(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    }
    c->out.clear();
    *id = (uint32_t)c->sk.size();
    c->sk.push_back(Meta{ksize, scaled, max_hash(scaled), c->n_entries, n, {}});
    c->n_entries += n;
    return CL_OK;
}

} // namespace fpc

extern "C" {

int dut_fpc_create(int device_id, void *stream, dut_fpc_ctx **out)
{
    if (!out) return CL_ERR_INVALID;
    *out = nullptr;
    dut_fpc_ctx *c = new (std::nothrow) dut_fpc_ctx();
    if (!c) return CL_ERR_NOMEM;
    c->device = device_id;
    if (const char *e = getenv("DUT_FPC_GRID_X")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v > 0) c->grid_x = (uint32_t)std::min<unsigned long long>(v, fpc::kMaxGridX);
    }
    if (device_id == -1) { c->host_only = true; *out = c; return CL_OK; }
    auto failed = [&](hipError_t e) { (void)e; (void)hipGetLastError(); dut_fpc_destroy(c); return CL_ERR_DEVICE; };
    hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) return failed(e);
    if (stream) c->stream = (hipStream_t)stream;
    else {
        if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return failed(e);
        c->own_stream = true;
    }
    for (auto &ev : c->ev) if ((e = hipEventCreate(&ev)) != hipSuccess) return failed(e);
    *out = c;
    return CL_OK;
}

void dut_fpc_destroy(dut_fpc_ctx *c)
{
    if (!c) return;
    if (!c->host_only) {
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        void *bufs[] = {c->d_hashes, c->d_counts, c->d_tab, c->d_part, c->d_rec};
        for (void *p : bufs) if (p) (void)hipFree(p);
        if (c->h_tab) (void)hipHostFree(c->h_tab);
        for (auto &ev : c->ev) if (ev) (void)hipEventDestroy(ev);
        if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    }
    delete c;
}

const char *dut_fpc_last_error(const dut_fpc_ctx *c) { return c ? c->err.c_str() : "null context"; }

int dut_fpc_add(dut_fpc_ctx *c, uint32_t ksize, uint64_t scaled, const uint64_t *hashes, const uint32_t *counts, uint64_t n, uint32_t *id)
{
    try { return fpc::add(c, ksize, scaled, hashes, counts, n, id); }
    catch (const std::bad_alloc &) { c->err = "out of host memory"; return CL_ERR_NOMEM; }
}

int dut_fpc_compare(dut_fpc_ctx *c, const uint32_t *pairs_a, const uint32_t *pairs_b, uint64_t n_pairs, const dut_fpc_record **out)
{
    try { return fpc::compare(c, pairs_a, pairs_b, n_pairs, out); }
    catch (const std::bad_alloc &) { c->err = "out of host memory"; return CL_ERR_NOMEM; }
}

int dut_fpc_compare_all(dut_fpc_ctx *c, const dut_fpc_record **out, uint64_t *n_pairs_out)
{
    if (!c) return CL_ERR_INVALID;
    try {
        const uint64_t n = c->sk.size(), np = n * (n ? n - 1 : 0) / 2;
        if (n_pairs_out) *n_pairs_out = np;
        if (np > DUT_FPC_MAX_PAIRS) return fpc::compare(c, nullptr, nullptr, np, out);      // (refused there, with the count)
        c->all_a.clear(); c->all_b.clear();
        for (uint32_t i = 0; i < n; ++i) for (uint32_t j = i + 1; j < n; ++j) { c->all_a.push_back(i); c->all_b.push_back(j); }
        return fpc::compare(c, c->all_a.data(), c->all_b.data(), np, out);
    } catch (const std::bad_alloc &) { c->err = "out of host memory"; return CL_ERR_NOMEM; }
}

int dut_fpc_stats(const dut_fpc_ctx *c, double *kernel_ms, uint64_t *n_tiles, uint64_t *bytes)
{
    if (!c) return CL_ERR_INVALID;
    if (kernel_ms) *kernel_ms = c->kernel_ms;
    if (n_tiles) *n_tiles = c->n_tiles;
    if (bytes) *bytes = c->bytes;
    return CL_OK;
}

uint32_t dut_fpc_tile(void) { return fpc::kTile; }

// ---- host only ----
int dut_fpc_compare_host(const dut_fpc_sketch *sk, uint64_t n_sketches, const uint32_t *pairs_a, const uint32_t *pairs_b,
                         uint64_t n_pairs, dut_fpc_record *out, char *err, size_t err_len)
{
    auto set = [&](const std::string &m) { if (err && err_len) snprintf(err, err_len, "%s", m.c_str()); return CL_ERR_INVALID; };
    try {
        if (n_sketches && !sk) return set("null sketches");
        std::vector<fpc::Meta> meta;
        for (uint64_t i = 0; i < n_sketches; ++i) {
            const std::string bad = fpc::validate(sk[i].ksize, sk[i].scaled, sk[i].hashes, sk[i].counts, sk[i].n);
            if (!bad.empty()) return set("sketch " + std::to_string(i) + ": " + bad);
            meta.push_back(fpc::Meta{sk[i].ksize, sk[i].scaled, fpc::max_hash(sk[i].scaled), 0, sk[i].n, {}});
        }
        if (n_pairs == 0) return CL_OK;
        if (!out) return set("null out");
        const std::string bad = fpc::check_pairs(meta, pairs_a, pairs_b, n_pairs);
        if (!bad.empty()) return set(bad);
        dut::parallel_for((size_t)n_pairs, 1, [&](size_t p) {
            const dut_fpc_sketch &a = sk[pairs_a[p]], &b = sk[pairs_b[p]];
            out[p] = fpc::merge_pair(a.hashes, a.counts, a.n, b.hashes, b.counts, b.n, std::min(meta[pairs_a[p]].max_hash, meta[pairs_b[p]].max_hash));
        });
        return CL_OK;
    } catch (const std::bad_alloc &) { if (err && err_len) snprintf(err, err_len, "out of host memory"); return CL_ERR_NOMEM; }
}

int dut_fp_file_read(const char *path, dut_fpc_sketch *out, char *err, size_t err_len)
{
    auto set = [&](const std::string &m) { if (err && err_len) snprintf(err, err_len, "%s", m.c_str()); return CL_ERR_INVALID; };
    if (!path || !out) return set("null argument");
    try {
        memset(out, 0, sizeof(*out));
        fpc::SketchFile *s = new fpc::SketchFile();
        const std::string bad = fpc::parse_file(path, *s);
        if (!bad.empty()) { delete s; return set(bad); }
        out->ksize = s->ksize; out->scaled = s->scaled; out->n = s->hashes.size();
        out->hashes = s->hashes.data(); out->counts = s->counts.data();
        snprintf(out->region, sizeof(out->region), "%s", s->region.c_str());
        out->max_frequency = s->max_frequency; out->has_max_frequency = s->has_max_frequency ? 1 : 0;
        out->owner = s;
        return CL_OK;
    } catch (const std::bad_alloc &) { if (err && err_len) snprintf(err, err_len, "out of host memory"); return CL_ERR_NOMEM; }
}

void dut_fp_file_free(dut_fpc_sketch *s)
{
    if (!s) return;
    delete (fpc::SketchFile *)s->owner;
    memset(s, 0, sizeof(*s));
}

} // extern "C"

namespace {

std::string ratio(uint64_t num, uint64_t den)
{
    if (den == 0) return "NA";
    char b[64];
    snprintf(b, sizeof(b), "%.6f", (double)num / (double)den);
    return b;
}

} // namespace

extern "C" {

int dut_fpc_write(FILE *f, const char *const *names, uint64_t n_sketches, uint32_t ksize, const uint32_t *pairs_a,
                  const uint32_t *pairs_b, const uint64_t *pair_scaled, const dut_fpc_record *rec, uint64_t n_pairs,
                  double min_jaccard, int has_min_jaccard)
{
    if (!f || !names || (n_pairs && (!pairs_a || !pairs_b || !pair_scaled || !rec))) return CL_ERR_INVALID;
    try {
        std::string s = "##sketches=" + std::to_string(n_sketches) + "\n##pairs=" + std::to_string(n_pairs) + "\n##ksize=" + std::to_string(ksize) +
                        "\n#a\tb\tscaled\tn_a\tn_b\tcommon\tunion\tjaccard\tcontainment_a\tcontainment_b\tsum_a\tsum_b\tsum_min\tweighted_jaccard\n";
        for (uint64_t p = 0; p < n_pairs; ++p) {
            const dut_fpc_record &r = rec[p];
            if (pairs_a[p] >= n_sketches || pairs_b[p] >= n_sketches) return CL_ERR_INVALID;
            const uint64_t uni = r.n_a + r.n_b - r.n_common;
            if (has_min_jaccard && (uni == 0 || (double)r.n_common / (double)uni < min_jaccard)) continue;
            s += names[pairs_a[p]]; s += '\t'; s += names[pairs_b[p]]; s += '\t';
            for (uint64_t v : {pair_scaled[p], r.n_a, r.n_b, r.n_common, uni}) { s += std::to_string(v); s += '\t'; }
            s += ratio(r.n_common, uni) + '\t' + ratio(r.n_common, r.n_a) + '\t' + ratio(r.n_common, r.n_b) + '\t';
            for (uint64_t v : {r.sum_a, r.sum_b, r.sum_min}) { s += std::to_string(v); s += '\t'; }
            s += ratio(r.sum_min, r.sum_a + r.sum_b - r.sum_min) + '\n';
            if (s.size() > (1u << 20)) { if (fwrite(s.data(), 1, s.size(), f) != s.size()) return CL_ERR_INVALID; s.clear(); }
        }
        return fwrite(s.data(), 1, s.size(), f) == s.size() ? CL_OK : CL_ERR_INVALID;
    } catch (const std::bad_alloc &) { return CL_ERR_NOMEM; }
}

int dut_fpc_write_matrix(FILE *f, const char *const *names, const uint64_t *n_entries, uint64_t n, const dut_fpc_record *rec)
{
    if (!f || !names || !n_entries || (n > 1 && !rec)) return CL_ERR_INVALID;
    try {
        // the record of (i, j), i < j, in the row-major list of all pairs
        auto at = [&](uint64_t i, uint64_t j) -> const dut_fpc_record & { return rec[i * n - i * (i + 1) / 2 + (j - i - 1)]; };
        std::string s = "#name";
        for (uint64_t i = 0; i < n; ++i) { s += '\t'; s += names[i]; }
        s += '\n';
        for (uint64_t i = 0; i < n; ++i) {
            s += names[i];
            for (uint64_t j = 0; j < n; ++j) {
                s += '\t';
                if (i == j) s += n_entries[i] ? "1.000000" : "NA";
                else { const dut_fpc_record &r = i < j ? at(i, j) : at(j, i); s += ratio(r.n_common, r.n_a + r.n_b - r.n_common); }
            }
            s += '\n';
        }
        return fwrite(s.data(), 1, s.size(), f) == s.size() ? CL_OK : CL_ERR_INVALID;
    } catch (const std::bad_alloc &) { return CL_ERR_NOMEM; }
}

} // extern "C"

namespace {

int compare_files_impl(const char *const *paths, uint64_t n, const dut_fpc_file_options *opt, const char *out_path,
                       const char *matrix_path, int device_id, char *err, size_t err_len)
{
    auto set = [&](const std::string &m, int rc) { if (err && err_len) snprintf(err, err_len, "%s", m.c_str()); return rc; };
    const char *query = opt ? opt->query : nullptr;
    if (!paths && n) return set("null paths", CL_ERR_INVALID);
    if (!out_path) return set("no output path", CL_ERR_INVALID);
    if (n + (query ? 1 : 0) < 2) return set("fingerprint-compare needs at least two sketches", CL_ERR_INVALID);
    if (query && matrix_path) return set("the matrix is written without a query only", CL_ERR_INVALID);
    std::vector<const char *> names;
    if (query) names.push_back(query);
    for (uint64_t i = 0; i < n; ++i) names.push_back(paths[i]);
    std::vector<fpc::SketchFile> files(names.size());
    for (size_t i = 0; i < names.size(); ++i) {
        const std::string bad = fpc::parse_file(names[i], files[i]);
        if (!bad.empty()) return set(bad, CL_ERR_INVALID);
    }
    for (size_t i = 1; i < files.size(); ++i) {
        if (files[i].ksize != files[0].ksize)
            return set(std::string(names[i]) + ": ksize " + std::to_string(files[i].ksize) + " against ksize " + std::to_string(files[0].ksize) + " of " + names[0], CL_ERR_INVALID);
    }
    for (size_t i = 1; i < files.size(); ++i) {
        if (files[i].has_max_frequency != files[0].has_max_frequency || files[i].max_frequency != files[0].max_frequency) {
            fprintf(stderr, "warning: %s and %s were written with different max_frequency filters\n", names[0], names[i]);
            break;
        }
    }
    std::vector<uint32_t> pa, pb;
    if (query) for (uint32_t j = 1; j < names.size(); ++j) { pa.push_back(0); pb.push_back(j); }
    else for (uint32_t i = 0; i < names.size(); ++i) for (uint32_t j = i + 1; j < names.size(); ++j) { pa.push_back(i); pb.push_back(j); }
    std::vector<uint64_t> scaled(pa.size());
    for (size_t p = 0; p < pa.size(); ++p) {
        const fpc::SketchFile &a = files[pa[p]], &b = files[pb[p]];
        scaled[p] = fpc::max_hash(a.scaled) <= fpc::max_hash(b.scaled) ? a.scaled : b.scaled;
    }
    dut_fpc_ctx *ctx = nullptr;
    int rc = dut_fpc_create(device_id, nullptr, &ctx);
    if (rc != CL_OK) return set("cannot create the compare context on device " + std::to_string(device_id), rc);
    const dut_fpc_record *rec = nullptr;
    for (size_t i = 0; i < files.size() && rc == CL_OK; ++i) {
        uint32_t id = 0;
        rc = dut_fpc_add(ctx, files[i].ksize, files[i].scaled, files[i].hashes.data(), files[i].counts.data(), files[i].hashes.size(), &id);
        if (rc != CL_OK) set(std::string(names[i]) + ": " + dut_fpc_last_error(ctx), rc);
    }
    if (rc == CL_OK && (rc = dut_fpc_compare(ctx, pa.data(), pb.data(), pa.size(), &rec)) != CL_OK) set(dut_fpc_last_error(ctx), rc);
    if (rc == CL_OK) {
        FILE *f = fopen(out_path, "wb");
        if (!f) rc = set(std::string("Failed to create output file ") + out_path, CL_ERR_INVALID);
        else {
            const int w = dut_fpc_write(f, names.data(), names.size(), files[0].ksize, pa.data(), pb.data(), scaled.data(), rec, pa.size(),
                                        opt ? opt->min_jaccard : 0.0, opt ? opt->has_min_jaccard : 0);
            if (fclose(f) != 0 || w != CL_OK) rc = set(std::string("Failed to write ") + out_path, CL_ERR_INVALID);
        }
    }
    if (rc == CL_OK && matrix_path) {
        std::vector<uint64_t> ne(files.size());
        for (size_t i = 0; i < files.size(); ++i) ne[i] = files[i].hashes.size();
        FILE *f = fopen(matrix_path, "wb");
        if (!f) rc = set(std::string("Failed to create output file ") + matrix_path, CL_ERR_INVALID);
        else {
            const int w = dut_fpc_write_matrix(f, names.data(), ne.data(), names.size(), rec);
            if (fclose(f) != 0 || w != CL_OK) rc = set(std::string("Failed to write ") + matrix_path, CL_ERR_INVALID);
        }
    }
    dut_fpc_destroy(ctx);
    return rc;
}

} // namespace

extern "C" int dut_fingerprint_compare_files(const char *const *paths, uint64_t n, const dut_fpc_file_options *options, const char *out_path,
                                             const char *matrix_path, int device_id, char *err, size_t err_len)
{
    try { return compare_files_impl(paths, n, options, out_path, matrix_path, device_id, err, err_len); }
    catch (const std::bad_alloc &) { if (err && err_len) snprintf(err, err_len, "out of host memory"); return CL_ERR_NOMEM; }
}
