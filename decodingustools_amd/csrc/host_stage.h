// host_stage.h -- what the host stages of the engines stand on without a device (plain C++, no HIP): the staging array
// and the stage timer.  engine_base.hip.h and tile_walk.h include it.
#pragma once
#include "host_parallel.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

// dst[0, m) = src[0, m) in parallel chunks (no overlap)
template <typename T> inline void copy_parallel(T *dst, const T *src, size_t m)
{
    const size_t grain = (4u << 20) / sizeof(T);
    dut::parallel_for((m + grain - 1) / grain, 1, [&](size_t k) {
        const size_t a = k * grain, b = std::min(m, a + grain);
        memcpy(dst + a, src + a, (b - a) * sizeof(T));
    });
}

// Host staging array of a trivially copyable type that grows without value-initialising what it adds (a contig's
// per-read arrays are hundreds of megabytes: zero-filling them before they are overwritten showed) and appends in
// parallel chunks.  Throws std::bad_alloc like a vector.
template <typename T> struct RawVec {
    T *p = nullptr;
    size_t n = 0, cap = 0;
    RawVec() = default;
    RawVec(const RawVec &) = delete;
    RawVec &operator=(const RawVec &) = delete;
    RawVec(RawVec &&o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    ~RawVec() { free(p); }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T *data() { return p; }
    const T *data() const { return p; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    const T &back() const { return p[n - 1]; }
    void clear() { n = 0; }
    void release() { free(p); p = nullptr; n = cap = 0; }
    void swap(RawVec &o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(cap, o.cap); }
    void reserve(size_t want)
    {
        if (want <= cap) return;
        size_t nc = std::max(want, cap + cap / 2 + 16);
        T *q = static_cast<T *>(realloc(p, nc * sizeof(T)));
        if (!q) throw std::bad_alloc();
        p = q; cap = nc;
    }
    void resize(size_t m) { reserve(m); n = m; }                 // new elements are NOT initialised
    void push_back(const T &v) { reserve(n + 1); p[n++] = v; }
    void append(const T *src, size_t m) { reserve(n + m); copy_parallel(p + n, src, m); n += m; }
};

// DUT_TIMING=1: wall-clock of the engine's host stages on stderr (tooling; off by default)
struct StageTimer {
    bool on;
    double t0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    StageTimer() : on(getenv("DUT_TIMING") && *getenv("DUT_TIMING") == '1'), t0(on ? now() : 0.0) {}
    void lap(const char *what)
    {
        if (!on) return;
        const double t1 = now();
        fprintf(stderr, "[dut-timing]     engine: %-24s %8.1f ms\n", what, (t1 - t0) * 1e3);
        t0 = t1;
    }
};
