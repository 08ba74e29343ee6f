// engine_base.hip.h -- what the engines of callable_loci.hip stand on (a textual part of that translation unit): device
// buffers, the pinned staging ring and transfers through it, error returns, the exception guard of the C ABI and the
// kernel timer.  (The host staging array and the stage timer need no device: host_stage.h.)
#pragma once

#include "../../include/callable_loci.h"
#include "host_parallel.h"
#include "host_stage.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace {

// rocTX ranges around the host-visible phases (rocprofv3 --marker-trace shows them); bound at run time so
// that the library does not depend on the profiler's marker library being installed -- and only when that library
// is in the process already (a profiler brought it) or DUT_ROCTX=1 asks for it: loading it cold took 35 ms of a
// process's first contig
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        const char *want = getenv("DUT_ROCTX");
        const int mode = RTLD_NOW | RTLD_LOCAL | ((want && *want == '1') ? 0 : RTLD_NOLOAD);
        for (const char *lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
            void *h = dlopen(lib, mode);
            if (!h) continue;
            push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
            pop = (int (*)())dlsym(h, "roctxRangePop");
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
struct Range {
    static const Roctx &rt() { static const Roctx r; return r; }
    explicit Range(const char *name) { if (rt().push) rt().push(name); }
    ~Range() { if (rt().pop) rt().pop(); }
};

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;     // elements
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = n + n / 8 + 64;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), want * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    // like reserve, but the first `used` elements survive a reallocation
    hipError_t grow_keep(size_t n, size_t used, hipStream_t stream)
    {
        if (n <= cap) return hipSuccess;
        if (!p || used == 0) return reserve(n);
        T *q = nullptr;
        size_t want = n + n / 4 + 64;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&q), want * sizeof(T));
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(q, p, used * sizeof(T), hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { (void)hipFree(q); return e; }
        (void)hipFree(p);
        p = q; cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Pinned host memory that only grows (what was in it is not kept): the target of a device-to-host copy too large to go
// through pageable memory at the link's rate (cl_contig_depth_runs).
template <typename T> struct PinBuf {
    T *p = nullptr;
    size_t cap = 0;     // elements
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        size_t want = n + n / 8 + 64;
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), want * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

} // namespace

// Pinned staging ring for host-to-device copies, one per device and process (its contexts share it; a transfer holds
// it from start to finish): kCopyThreads host threads, each with its own stream and two pinned buffers; a thread fills
// one buffer (memcpy from the caller's pageable memory, or records built in place) while the DMA of its other buffer
// runs, so the link sees pinned memory only and the fills of all threads overlap all transfers.
struct PinRing {
    static constexpr int kCopyThreads = 16;                 // buffer pairs: plain copies use threads() of them, the walkers
                                                            // that produce a stream into the buffers (rows, run table) all
    static constexpr size_t kPinBytes = 4u << 20;
    static int threads()                                    // DUT_COPY_THREADS (1..16), default 8
    {
        static const int n = [] {
            const char *e = getenv("DUT_COPY_THREADS");
            const int v = e ? atoi(e) : 8;
            return v < 1 ? 1 : (v > kCopyThreads ? kCopyThreads : v);
        }();
        return n;
    }
    int device = 0;
    hipStream_t copy_stream[kCopyThreads] = {};
    uint8_t *pin[kCopyThreads][2] = {};
    hipEvent_t pin_ev[kCopyThreads][2] = {};
    // who is using the ring: a transfer holds it from ring_start to ring_finish -- across C-ABI calls for a quality
    // prefetch, and possibly released on another thread than the one that took it, so an ownership flag under a
    // condition variable rather than a mutex (unlocking a std::mutex from another thread is undefined)
    std::mutex own_mu;
    std::condition_variable own_cv;
    const void *owner = nullptr;
    void acquire(const void *who)
    {
        std::unique_lock<std::mutex> lk(own_mu);
        // a context of this device with an unclaimed prefetch pins the ring until its next push / upload / begin /
        // abort / destroy; a thread that drives two contexts must not interleave them there
        int waited = 0;
        while (owner && !own_cv.wait_for(lk, std::chrono::seconds(10), [this] { return owner == nullptr; }))
            if (++waited == 1)
                fprintf(stderr, "[callable_loci] waiting for the device's pinned staging ring: another context holds it "
                                "(an unclaimed cl_contig_prefetch_qual keeps it until that context's next push, upload, begin, abort or destroy)\n");
        owner = who;
    }
    void release(const void *who)
    {
        { std::lock_guard<std::mutex> g(own_mu); if (owner == who) owner = nullptr; }
        own_cv.notify_one();
    }
    // The ring's own threads: started once (at cl_create), asleep between transfers.  (A thread created per transfer had to
    // wait for the process's address-space lock whenever another thread was giving a few hundred megabytes back to the
    // system -- 26 ms in front of a 3 ms transfer, measured: profiles/r04_first_pass_stages.txt.)
    dut::Crew crew;
    bool ok = false;
    int slots = 0;                                          // thread slots that have their stream, buffers and events
    // slots [slots, n) are made (by the ring's owner, or at construction); false when the runtime refuses
    bool ensure_slots(int n)
    {
        if (n > kCopyThreads) n = kCopyThreads;
        if (hipSetDevice(device) != hipSuccess) return false;
        for (int t = slots; t < n; ++t) {
            if (hipStreamCreateWithFlags(&copy_stream[t], hipStreamNonBlocking) != hipSuccess) return false;
            for (int b = 0; b < 2; ++b) {
                if (hipHostMalloc(reinterpret_cast<void **>(&pin[t][b]), kPinBytes, hipHostMallocDefault) != hipSuccess) return false;
                // blocking waits: a copier that spins on its buffer's event burns a core the host stages beside it
                // need (DUT_PIN_SPIN=1: the runtime's default busy wait, for comparison)
                const char *spin = getenv("DUT_PIN_SPIN");
                const unsigned flags = hipEventDisableTiming | ((spin && *spin == '1') ? 0u : (unsigned)hipEventBlockingSync);
                if (hipEventCreateWithFlags(&pin_ev[t][b], flags) != hipSuccess) return false;
            }
            slots = t + 1;
        }
        return true;
    }
    explicit PinRing(int dev) : device(dev) { ok = ensure_slots(kCopyThreads); if (ok) crew.ensure(kCopyThreads); }
    ~PinRing()
    {
        (void)hipSetDevice(device);
        for (int t = 0; t < kCopyThreads; ++t) {
            for (int b = 0; b < 2; ++b) {
                if (pin_ev[t][b]) (void)hipEventDestroy(pin_ev[t][b]);
                if (pin[t][b]) (void)hipHostFree(pin[t][b]);
            }
            if (copy_stream[t]) (void)hipStreamDestroy(copy_stream[t]);
        }
    }
    PinRing(const PinRing &) = delete;
    PinRing &operator=(const PinRing &) = delete;
};

static std::shared_ptr<PinRing> acquire_ring(int device)
{
    static std::mutex mu;
    static std::map<int, std::weak_ptr<PinRing>> rings;
    std::lock_guard<std::mutex> g(mu);
    std::shared_ptr<PinRing> r = rings[device].lock();
    if (!r) {
        r = std::make_shared<PinRing>(device);
        if (!r->ok) return nullptr;
        rings[device] = r;
    }
    return r;
}

// What every engine of a context shares: its device and stream, the last error, and the state of its transfer through
// the ring (ring_start .. ring_finish).  cl_ctx derives from it.
struct EngineBase {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool host_only = false;          // cl_debug_host_create: staging and the row builder only, for the CPU test suite
    std::string err;
    std::shared_ptr<PinRing> ring;                    // the device's pinned staging ring (shared by its contexts)
    bool crew_busy = false;                           // a transfer in flight on the ring's threads (waited for by ring_finish)
    hipError_t copy_err[PinRing::kCopyThreads] = {};
    bool ring_held = false;                           // this context holds the ring's lock (ring_start .. ring_finish)
    double ring_t0 = 0;                               // DUT_TIMING: when the transfer in flight was started
    // cl_contig_prefetch_qual: quality bytes on their way to d_qual + kQualPad + pf_off before their tile is pushed
    const uint8_t *pf_src = nullptr;
    uint64_t pf_n = 0, pf_off = 0;
    bool pf_active = false;
};

namespace {

cl_status fail(EngineBase *c, cl_status s, const std::string &m)
{
    if (c) c->err = m;
    return s;
}

#define HIP_TRY(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fail(ctx, e__ == hipErrorOutOfMemory ? CL_ERR_NOMEM : CL_ERR_DEVICE,      \
                        std::string(#call) + ": " + hipGetErrorString(e__));                 \
    } while (0)

cl_status ensure_pins(EngineBase *c)
{
    if (c->ring) return CL_OK;
    c->ring = acquire_ring(c->device);
    if (!c->ring) return fail(c, CL_ERR_DEVICE, "cannot create the pinned staging ring (hipHostMalloc)");
    return CL_OK;
}

// n bytes to `dst` through the ring: fill(off, len, out) writes the bytes [off, off + len) of the transfer into the
// pinned buffer `out`.  Chunks are dealt round-robin to the copier threads.  Returns at once; ring_finish joins.
template <class Fill>
cl_status ring_start(EngineBase *c, uint8_t *dst, uint64_t n, Fill fill, uint64_t chunk_bytes = PinRing::kPinBytes, int want_threads = 0)
{
    cl_status s = ensure_pins(c);
    if (s != CL_OK) return s;
    PinRing *R = c->ring.get();
    c->ring_t0 = StageTimer::now();
    R->acquire(c);                                        // another context of this device may be using the ring
    c->ring_held = true;
    const uint64_t CH = chunk_bytes, nch = (n + CH - 1) / CH;
    // (plain copies saturate the link with DUT_COPY_THREADS buffers in flight; a fill that gathers small pieces is bound by
    // the fill and asks for all of the ring's pairs)
    const int T = want_threads > 0 ? std::min(want_threads, std::max(1, R->slots)) : PinRing::threads();
    const int nt = (int)std::min<uint64_t>((uint64_t)T, nch);
    for (int t = 0; t < PinRing::kCopyThreads; ++t) c->copy_err[t] = hipSuccess;
    c->crew_busy = true;
    R->crew.start(nt, [c, R, dst, n, fill, nch, CH, T](int t) {
            const bool timing = StageTimer().on;
            double t_fill = 0, t_issue = 0, t_wait = 0, t0 = timing ? StageTimer::now() : 0.0, ta;
            hipError_t e = hipSetDevice(c->device);
            int k = 0;
            for (uint64_t ch = (uint64_t)t; ch < nch && e == hipSuccess; ch += (uint64_t)T, ++k) {
                const int b = k & 1;
                const uint64_t off = ch * CH, len = std::min<uint64_t>(CH, n - off);
                if (timing) ta = StageTimer::now();
                if (k >= 2) e = hipEventSynchronize(R->pin_ev[t][b]);           // the buffer's previous transfer is done
                if (e != hipSuccess) break;
                if (timing) { const double tb = StageTimer::now(); t_wait += tb - ta; ta = tb; }
                fill(off, len, R->pin[t][b]);
                if (timing) { const double tb = StageTimer::now(); t_fill += tb - ta; ta = tb; }
                e = hipMemcpyAsync(dst + off, R->pin[t][b], len, hipMemcpyHostToDevice, R->copy_stream[t]);
                if (e == hipSuccess) e = hipEventRecord(R->pin_ev[t][b], R->copy_stream[t]);
                if (timing) t_issue += StageTimer::now() - ta;
            }
            // the thread's last transfers (one per buffer it used), waited for on their events
            if (timing) ta = StageTimer::now();
            hipError_t e2 = hipSuccess;
            for (int b = 0; b < 2 && b < k; ++b) { const hipError_t w = hipEventSynchronize(R->pin_ev[t][b]); if (e2 == hipSuccess) e2 = w; }
            c->copy_err[t] = e != hipSuccess ? e : e2;
            if (timing) {
                const double t1 = StageTimer::now();
                fprintf(stderr, "[dut-timing]       ring thread %d: %d buffers, started %.1f ms after the call, fill %.1f, issue %.1f, wait %.1f + %.1f ms\n", t, k,
                        (t0 - c->ring_t0) * 1e3, t_fill * 1e3, t_issue * 1e3, t_wait * 1e3, (t1 - ta) * 1e3);
            }
    });
    return CL_OK;
}

cl_status ring_finish(EngineBase *c)
{
    if (c->crew_busy) { c->ring->crew.wait(); c->crew_busy = false; }   // the ring's threads are done with this transfer
    if (c->ring_held) { c->ring_held = false; c->ring->release(c); }
    for (int t = 0; t < PinRing::kCopyThreads; ++t) HIP_TRY(c, c->copy_err[t]);
    return CL_OK;
}

// plain bytes through the ring, start to finish
cl_status ring_copy(EngineBase *c, void *dst, const void *src, uint64_t n)
{
    if (n == 0) return CL_OK;
    const uint8_t *s8 = static_cast<const uint8_t *>(src);
    cl_status s = ring_start(c, static_cast<uint8_t *>(dst), n, [s8](uint64_t off, uint64_t len, uint8_t *out) { memcpy(out, s8 + off, len); });
    if (s != CL_OK) return s;
    return ring_finish(c);
}

// a prefetch that was started and never claimed by a tile: wait for it, its bytes are simply overwritten later
void drop_prefetch(EngineBase *c)
{
    if (!c->pf_active) return;
    (void)ring_finish(c);
    c->pf_active = false; c->pf_src = nullptr; c->pf_n = 0;
}

// No exception leaves the library through the C ABI: an entry point runs its body in here.
template <class F> cl_status guarded(EngineBase *c, F &&f)
{
    try { return f(); }
    catch (const std::bad_alloc &) { return fail(c, CL_ERR_NOMEM, "out of memory"); }
    catch (...) { return fail(c, CL_ERR_INVALID, "internal error"); }
}

// ... and none leaves a walker thread of the ring: whatever its body throws (its buffers' allocations) is an error code
template <class F> void walker_guarded(hipError_t &err, F &&f)
{
    try { f(); } catch (...) { if (err == hipSuccess) err = hipErrorOutOfMemory; }
}

// The duration of a stretch of kernels on a stream by two HIP events (made at the first start), and the algorithmic
// bytes its owner counts for it.
struct KernelTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms = 0.0;
    uint64_t bytes = 0;
    hipError_t start(hipStream_t s)
    {
        for (hipEvent_t &e : ev)
            if (!e) { const hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; }
        return hipEventRecord(ev[0], s);
    }
    hipError_t stop(hipStream_t s) { return hipEventRecord(ev[1], s); }
    // once the stream has passed stop(): the duration becomes ms, or (add) is added to it
    hipError_t read(bool add = false)
    {
        float t = 0.f;
        const hipError_t r = hipEventElapsedTime(&t, ev[0], ev[1]);
        if (r == hipSuccess) ms = add ? ms + t : t;
        return r;
    }
    void destroy() { for (hipEvent_t &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; } }
};

} // namespace
