// callable_loci.hip -- implementation of include/callable_loci.h for MI355X (gfx950).
//
// Host side of the coverage engine: staging, uploads, kernel launches, event timing.  The work itself is in three headers:
// pileup_rows.hip.h (k_pileup_rows, the pass-bit form: the product), pileup_bytes.hip.h (k_pileup, the byte forms of
// DUT_QUAL_FORM=bytes) and kernels.hip.h (what both share: constants, the records between kernels and host, the wave
// primitives and k_tail, the one kernel behind the pileup).  engine_base.hip.h holds the memory and transfer plumbing, site_engine.hip.h
// the site engine (all parts of this translation unit).  What needs no device of the way a tile of reads enters -- the
// staged contig, the record of a push, the checks, the first pass over a tile and the whole walk of the pass-bit form -- is
// tile_walk.h, plain C++ that the sanitizer driver runs; here are the entries, the byte forms' device side (prefetch,
// pinned ring, d_qual) and their share of the first pass.  No CPU fallback exists: without a HIP device cl_create fails.
#include "../../include/callable_loci.h"
#include "kernels.hip.h"
#include "pileup_bytes.hip.h"
#include "pileup_rows.hip.h"
#include "window_depths.hip.h"
#include "depth_profile.hip.h"
#include "depth_runs.hip.h"
#include "depth_targets.hip.h"
#include "target_order.hip.h"
#include "gc_bias.hip.h"
#include "engine_base.hip.h"
#include "site_engine.hip.h"
#include "qual_pack.h"
#include "gc_bits.h"
#include "pass_rows.h"
#include "tile_walk.h"
#include "target_pieces.h"

using namespace clk;

// window size (reference positions per workgroup).  2048 -> about 19 KB of LDS per workgroup of the short-read
// variant, eight workgroups (32 waves) per CU.
#ifndef CL_WINDOW
#define CL_WINDOW 2048
#endif
constexpr uint32_t kT = CL_WINDOW;

struct cl_ctx : SiteCtx {              // (EngineBase, and the site engine's state in its one member `site`)
    dut::Thread prealloc;                             // cl_contig_reserve: the device buffers of the contig being pushed, allocated beside the push
    cl_options opt{};
    Opts dopt{};

    // host staging of the current contig
    bool in_contig = false, uploaded = false, ran = false;
    bool collected = false;          // cl_contig_collect has succeeded since the last cl_contig_run: d_iv holds all its intervals (cl_contig_targets)
    bool deep = false;               // this contig needs the 32-bit counter variant of k_pileup
    bool bits = true;                // the pass-bit form (default); DUT_QUAL_FORM=bytes at cl_create: the byte forms
    int form = 0;                    // the form of k_pileup the resident contig gets (pick_form, at upload)
    int32_t tid = 0;
    uint32_t contig_len = 0;
    Staging hs;                      // the staged arrays themselves (tile_walk.h)
    PushRecord acc;                  // what the pushes of the contig being pushed have accumulated beside them (tile_walk.h)
    uint32_t n_rec = 0;
    uint64_t dev_sum_cov = 0, dev_sum_mapq = 0;   // of the resident contig: the reads' separable sums (acc.host_sum_cov, acc.host_sum_mapq at upload)
    uint32_t head_span = kHeadSpanMax;   // most positions one head of k_pileup_rows spans (DUT_HEAD_SPAN: a test hook)
    bool heads8_only = false;            // DUT_HEADS8=1 (a test hook): every contig gets 8-byte heads
    bool rows_uniform = false;           // DUT_ROWS_UNIFORM=1 (a test hook): every segment of a window as high as its highest
    bool heads4 = false;                 // the resident contig's heads are the 4-byte form (pileup_rows.hip.h: HEAD4)
    uint64_t dev_sum_q = 0;          // of the resident contig: acc.host_sum_q at upload (a start value of every run's summary: d_sum0)
    uint32_t tail_max_chunks = kTailMaxChunks;   // most workgroups of k_tail (DUT_TAIL_CHUNKS: a test hook)
    uint32_t bounds_err = 0;             // kErrRange raised by the window bounds (reported by cl_contig_collect)
    uint32_t n_wide = 0;

    // device residents
    DevBuf<int32_t> d_pos;
    DevBuf<uint8_t> d_mapq;
    DevBuf<uint8_t> d_qual;
    DevBuf<uint8_t> d_ref;
    DevBuf<uint32_t> d_end;
    DevBuf<ReadRec> d_rec;           // the records of the short-read form of k_pileup
    DevBuf<uint2> d_heads;           // pass-bit form: the heads k_pileup_rows reads, {pos, span | low << 31} -- or, with
                                     // heads4, 4-byte heads, two to an element
    DevBuf<uint32_t> d_refn;         // pass-bit form: bit p = the reference base at p is 'N' / 'n' or lies beyond the reference
    DevBuf<uint4> d_rows;            // pass-bit form: the windows' rows, units of 4 rows x 8 blocks (128 bytes each: pass_rows.h)
    uint64_t n_row_groups = 0;       // ... how many units
    uint32_t max_groups = 0;         // most units of any segment of any window: picks the number of counter planes of k_pileup_rows
    DevBuf<uint32_t> d_win_words, d_wide_idx;   // d_win_words: per window n_inner | first state << 16 | last state << 24 (kernels.hip.h)
    DevBuf<WinMeta> d_win;
    DevBuf<uint8_t> d_state;         // per-position states: allocated and written for debug dumps only
    DevBuf<uint16_t> d_runs;         // per window kT entries: run starts inside the window
    DevBuf<uint8_t> d_win_wide;      // per window: sticky "needs 16-bit counter fields" mark (k_pileup)
    DevBuf<uint4> d_winpart;           // the windows' totals: WinRecords (pass-bit form) or WinPartials (byte forms)
    DevBuf<uint32_t> d_errflag;        // [0] error bits raised by the kernels of a run, [1] unused
    DevBuf<uint2> d_runtab;            // run-table form: the windows' match pieces (host_build_runs)
    uint64_t n_runtab = 0;
    DevBuf<uint32_t> d_lut;
    DevBuf<uint32_t> d_lut8;         // build_lut8's 64 words, what k_pileup_rows' fast path looks up
    DevBuf<DevSummary> d_summary;
    DevBuf<DevSummary> d_sum0;       // the start values of a run's summary (filled at upload; the pileup's window 0 copies them)
    DevBuf<Interval> d_iv;
    DevBuf<uint32_t> d_dbg;          // 3 * n_win * T
    // cl_contig_depth_profile: {sum_raw, sum_qc}, hist_raw, hist_qc, win_raw, win_qc -- on the device and as copied back
    DevBuf<unsigned long long> d_prof;
    std::vector<unsigned long long> h_prof;
    KernelTimer t_prof;              // the last profile's kernel (recorded while profiling is on)
    // cl_contig_depth_runs: per window {cnt, first, last} and the error word behind them; the windows' 64-bit offsets and
    // the total behind them; the runs, start[n] then value[n], on the device and as copied back (pinned)
    DevBuf<uint32_t> d_dr_win;
    DevBuf<unsigned long long> d_dr_off;
    DevBuf<uint32_t> d_dr_out;
    PinBuf<uint32_t> h_dr_out;
    KernelTimer t_dr_count, t_dr_write;   // count launch + scan, write launch (recorded while profiling is on)
    double dr_ms = 0.0;
    // cl_contig_targets: what goes up (the points, the windows' ranges of them, the targets), the windows' totals (a record
    // per window), their scanned offsets (a row per field), the prefixes at the points (a record per point), the records
    // and the error word behind them -- and the records as copied back
    DevBuf<uint32_t> d_tg_in, d_tg_out;
    DevBuf<uint4> d_tg_pre;
    DevBuf<ulonglong2> d_tg_win;
    DevBuf<unsigned long long> d_tg_off;
    std::vector<uint32_t> h_tg_in;
    std::vector<cl_target_stats> h_tg_out;
    KernelTimer t_tg[3];                  // k_target_depth, k_target_scan, k_target_finish (recorded while profiling is on)
    double tg_ms[3] = {0.0, 0.0, 0.0};
    // cl_contig_target_order: what goes up (the pieces, the windows' ranges of them, the clipped targets), the targets'
    // states with the two words behind them (the largest raw depth, the error word), the records -- and the records as
    // copied back
    DevBuf<uint32_t> d_to_in, d_to_st, d_to_out;
    std::vector<TargetPiece> h_to_pc;
    std::vector<uint32_t> h_to_first, h_to_tg;
    std::vector<cl_target_order> h_to_out;
    KernelTimer t_to[2];                  // the FIRST launch and its step; the rounds (recorded while profiling is on)
    double to_ms = 0.0;
    uint32_t to_rounds = 0;
    // cl_contig_gc_bias: the reference's {gc, valid} pairs of a call (gc_bias.hip.h), what the kernel adds to, and that as
    // copied back
    DevBuf<uint4> d_gc_bits;
    DevBuf<unsigned long long> d_gc_out;
    unsigned long long h_gc_out[kGcOutWords] = {};
    KernelTimer t_gc;                     // the last call's kernel (recorded while profiling is on)
    double gc_upload_ms = 0.0;            // ... and its pack + upload, by the host's clock
    // The device buffers of the context, listed once: f(buffer) for each one that cl_layout_info.device_bytes counts, which
    // is all of them but d_prof and the site engine's (they never were).  cl_destroy and cl_contig_layout walk this list.
    template <class F> void each_buffer(F &&f)
    {
        f(d_pos); f(d_mapq); f(d_qual); f(d_ref); f(d_end); f(d_rec); f(d_heads); f(d_refn); f(d_rows); f(d_win_words); f(d_wide_idx);
        f(d_win); f(d_state); f(d_runs); f(d_win_wide); f(d_winpart); f(d_errflag);
        f(d_runtab); f(d_lut); f(d_lut8); f(d_summary); f(d_sum0); f(d_iv); f(d_dbg); f(d_dr_win); f(d_dr_off); f(d_dr_out);
    }
    // the counter planes of k_pileup_rows and the depth kernels by the deepest window's rows (4 per group): 8 planes count to 255
    uint32_t counter_planes() const { return max_groups <= 63u ? 8u : max_groups <= 16383u ? 16u : 32u; }

    uint32_t n_reads = 0;
    uint64_t n_cigar = 0, n_qual = 0;
    uint32_t extent = 0, n_win = 0;

    std::vector<cl_interval> h_iv;
    DevSummary h_sum{};

    // profiling
    bool profiling = false;
    static constexpr int kEvSets = 64;       // runs that can be in flight before events are read back
    hipEvent_t ev[kEvSets][3] = {};          // per run: before the pileup, after it, after the tail
    bool ev_made = false;
    int ev_pending = 0;
    double ms[CL_K_COUNT] = {};
    uint64_t n_runs = 0;
};

static SiteCtx *site_ctx(cl_ctx *c) { return c; }
static void join_prealloc(cl_ctx *c) { if (c->prealloc.joinable()) c->prealloc.join(); }   // (cl_contig_reserve's helper thread)

namespace {

// constants of the byte-parallel threshold test (pileup_bytes.hip.h: swar_ge7)
void make_ge_consts(uint8_t T, uint32_t &ge_add, uint32_t &ge_or, uint32_t &ge_and)
{
    uint32_t add;
    if (T == 0) { add = 0x80u; ge_or = 0xFFFFFFFFu; ge_and = 0xFFFFFFFFu; }
    else if (T <= 128) { add = 128u - T; ge_or = 0xFFFFFFFFu; ge_and = 0xFFFFFFFFu; }
    else { add = 256u - T; ge_or = 0u; ge_and = 0u; }
    ge_add = add * 0x01010101u;
}

// lut[raw] = smallest low_mapq_count with (low as f64 / raw as f64) > max_low_mapq_fraction
// (callable_profiler.rs:100-101), or 0xFFFFFFFF when no count <= raw qualifies.  Built with the
// same IEEE f64 divide and compare as the reference, so the device test `low >= lut[raw]` is
// exact by construction (the quotient is monotone in `low`).
void build_lut(double frac, std::vector<uint32_t> &lut)
{
    lut.assign(kLutSize, 0xFFFFFFFFu);
    for (uint32_t raw = 1; raw < kLutSize; ++raw) {
        double g = std::floor(frac * (double)raw) - 2.0;
        if (!(g == g)) continue;                 // NaN fraction: the comparison is never true
        if (g > (double)raw) continue;
        uint32_t low = g < 0.0 ? 0u : (uint32_t)g;
        while (low <= raw && !(((double)low / (double)raw) > frac)) ++low;
        if (low <= raw) lut[raw] = low;
    }
}

// The thresholds of depths 0..255 as bytes, four per word, for k_pileup_rows' fast path (which sees depths below 255 only):
// 255 = never -- depth 0, a depth below min_depth_for_low_mapq (callable_profiler.rs:100), and a threshold no byte-sized
// count reaches (a count is at most the depth: below 255 here).
void build_lut8(const std::vector<uint32_t> &lut, uint32_t min_depth_for_low_mapq, uint32_t (&lut8)[64])
{
    for (uint32_t i = 0; i < 256; ++i) {
        const uint32_t v = (i == 0 || i < min_depth_for_low_mapq || lut[i] > 254u) ? 255u : lut[i];
        if (i % 4 == 0) lut8[i / 4] = 0;
        lut8[i / 4] |= v << (8 * (i % 4));
    }
}

cl_status ensure_events(cl_ctx *c)
{
    if (c->ev_made) return CL_OK;
    for (auto &set : c->ev)
        for (hipEvent_t &e : set) HIP_TRY(c, hipEventCreate(&e));
    c->ev_made = true;
    return CL_OK;
}

cl_status harvest_events(cl_ctx *c)
{
    for (int s = 0; s < c->ev_pending; ++s) {
        HIP_TRY(c, hipEventSynchronize(c->ev[s][2]));
        // (the per-read and per-window indexes are built on the host at upload: CL_K_PREP and CL_K_BOUNDS stay 0)
        float pileup = 0.f, tail = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&pileup, c->ev[s][0], c->ev[s][1]));
        HIP_TRY(c, hipEventElapsedTime(&tail, c->ev[s][1], c->ev[s][2]));
        c->ms[CL_K_PILEUP] += pileup; c->ms[CL_K_RLE] += tail;
        c->n_runs += 1;
    }
    c->ev_pending = 0;
    return CL_OK;
}

// which form of k_pileup a resident contig gets: by its shape, decided once at upload and kept in the context
// (3 k_pileup_rows; the byte forms, pileup_bytes.hip.h: LONG = 0 records (short reads), 2 the run table (long reads))
int pick_form(const cl_ctx *c)
{
    if (c->bits) return 3;           // the pass-bit form: head records + rows, whatever the reads' shape
    int form = 0;
    // long-read shape (8 or more CIGAR operations per read on average): the host's walk leaves a table of match pieces
    // per window (the run-table form).  It also wins where the operation-parallel form of rounds 1-2 was used -- long
    // match runs, HiFi-like: 0.157 against 0.292 ms at 20 Mb with 800-base runs, 0.185 against 0.382 with 150-base runs
    // (profiles/r03_hifi_forms.txt) --, so every long-read shape gets it.
    if (c->n_reads && c->n_cigar >= 8ull * c->n_reads) form = 2;
    return form;
}

// The records of one read for the short-read form of k_pileup (pileup_bytes.hip.h: ReadRec), in order: put(k, rec) for
// k = 0 .. count - 1; returns the count.  What the reference's column walk sees of the read (mod.rs:22-37): it is in
// every column of [pos, end) -- the head record --, and the bases of its M/=/X operations that have a quality byte are
// tested against min_base_quality -- the head's own run and the piece records.  Reads below min_mapping_quality are
// only counted (mod.rs:25): head alone.  A read without a reference span is in no column: no record.
template <class Put>
inline uint32_t gen_read_recs(int32_t pos, uint32_t end, uint32_t mq, uint32_t min_mapq, const uint32_t *cig, uint32_t nops,
                              unsigned long long q0, unsigned long long ql, Put &&put, uint32_t *phase = nullptr)
{
    // *phase: (reference position - query offset) mod 16 of the first run that gets a record -- where the read's quality
    // bytes have to start, mod 16, for that run's 16-position units to be 16-byte aligned in memory
    if (phase) *phase = 0u;
    bool first_run = true;
    const uint32_t span = end - (uint32_t)pos;
    if (span == 0u) return 0u;
    ReadRec head;
    head.pos = pos; head.span = span; head.qual_lo = 0u; head.meta = mq | 0x100u;
    uint32_t k = 1;
    if (mq >= min_mapq) {
        unsigned long long xr = (uint32_t)pos, y = 0;
        for (uint32_t j = 0; j < nops && xr <= 0xFFFF0000ull; ++j) {
            const uint32_t cw = cig[j], op = cw & 15u, l = cw >> 4;
            if ((0x181u >> op) & 1u) {                                     // M = X
                const unsigned long long lq = y < ql ? std::min<unsigned long long>(ql - y, l) : 0ull;   // bases that have a quality byte
                for (unsigned long long off = 0; off < lq; off += 0xFFFFull) {
                    const uint32_t len = (uint32_t)std::min<unsigned long long>(lq - off, 0xFFFFull);
                    const unsigned long long px = xr + off;
                    if (px > 0xFFFF0000ull) break;                          // flagged kErrRange by cl_push_reads
                    if (first_run) { first_run = false; if (phase) *phase = (uint32_t)((px - (y + off)) & 15ull); }
                    if (k == 1u && !(head.meta >> 16) && px == (uint32_t)pos) {
                        head.qual_lo = (uint32_t)(q0 + y + off); head.meta |= len << 16;
                    } else {
                        ReadRec r;
                        r.pos = (int32_t)(uint32_t)px; r.span = 0u; r.qual_lo = (uint32_t)(q0 + y + off); r.meta = mq | (len << 16);
                        put(k++, r);
                    }
                }
                xr += l; y += l;
            } else if ((0x18Du >> op) & 1u) xr += l;                       // D N
            else if ((0x193u >> op) & 1u) y += l;                          // I S
        }
    }
    put(0u, head);
    return k;
}

// A read's share of summed_baseq (contig_profiler.rs:65-70): the sum of the quality bytes that pass min_base_quality
// over the bases of its M/=/X operations that have a quality byte (q[0, ql): the read's quality string).  Reads of few
// operations: run by run; reads of many (long reads, a run every ~15 bases): the whole string minus the inserted and
// clipped bases, so that the vector loop sees long stretches.
inline uint64_t read_pass_sum(const uint8_t *q, unsigned long long ql, const uint32_t *cig, uint32_t nops, uint8_t thr, int level)
{
    unsigned long long y = 0;
    uint64_t sum = 0;
    if (nops <= 8u) {
        for (uint32_t j = 0; j < nops; ++j) {
            const uint32_t cw = cig[j], op = cw & 15u, l = cw >> 4;
            if ((0x181u >> op) & 1u) { if (y < ql) sum += dut::qual_pass_sum(q + y, std::min<unsigned long long>(ql - y, l), thr, level); y += l; }
            else if ((0x193u >> op) & 1u) y += l;
        }
        return sum;
    }
    uint64_t minus = 0;
    for (uint32_t j = 0; j < nops; ++j) {
        const uint32_t cw = cig[j], op = cw & 15u, l = cw >> 4;
        if ((0x181u >> op) & 1u) y += l;
        else if ((0x193u >> op) & 1u) { if (y < ql) minus += dut::qual_pass_sum(q + y, std::min<unsigned long long>(ql - y, l), thr, 0); y += l; }
    }
    return dut::qual_pass_sum(q, std::min<unsigned long long>(ql, y), thr, level) - minus;
}

// DUT_FAULT_INJECT=<what> (tests only; read at every upload): the named builder hands the bounds checks of the upload an
// index that lies outside its array -- "rows" a window's group range, "runtab" a read's quality offset in the run table,
// "rec" a record's quality offset -- so that a test can see the check refuse what would otherwise be a device fault.
bool fault_injected(const char *what)
{
    const char *e = getenv("DUT_FAULT_INJECT");
    return e && strcmp(e, what) == 0;
}

// bytes of read records per pinned buffer (DUT_REC_CHUNK: a test hook that puts the buffer seams inside the records of
// one read with small inputs; a multiple of the record size; read once)
uint64_t rec_chunk_bytes()
{
    static const uint64_t n = [] {
        const char *e = getenv("DUT_REC_CHUNK");
        uint64_t v = e ? strtoull(e, nullptr, 0) : PinRing::kPinBytes;
        v &= ~(uint64_t)(sizeof(ReadRec) - 1);
        return v < sizeof(ReadRec) ? sizeof(ReadRec) : (v > PinRing::kPinBytes ? PinRing::kPinBytes : v);
    }();
    return n;
}

// The fill of ring_start for an array of n_rec records (heads, ReadRec) plus a zeroed padding record, built in place by
// record number: read i of n owns the records [ro[i], ro[i + 1]).  A pinned buffer covers a range [j0, j1) of record
// numbers; the read that holds j0 is found by binary search, and emit(i, put) is called for every read with a record in
// the range: put(k, rec) stores the read's k-th record if the buffer holds it.
template <class Rec, class Emit>
auto rec_range_fill(const uint32_t *ro, size_t n, uint32_t n_rec, Emit emit)
{
    return [ro, n, n_rec, emit](uint64_t off, uint64_t len, uint8_t *out) {
        Rec *o = reinterpret_cast<Rec *>(out);
        const uint64_t j0 = off / sizeof(Rec), j1 = (off + len) / sizeof(Rec);
        if (j1 > n_rec) memset(static_cast<void *>(o + (std::max<uint64_t>(n_rec, j0) - j0)), 0, (j1 - std::max<uint64_t>(n_rec, j0)) * sizeof(Rec));   // the padding record
        if (j0 >= n_rec) return;
        // the read that holds record j0: the last one whose range starts at or before it
        size_t i = (size_t)(std::upper_bound(ro, ro + n + 1, (uint32_t)j0) - ro) - 1;
        for (; i < n && ro[i] < j1; ++i) {
            const uint64_t jb = ro[i];
            emit(i, [&](uint32_t k, const Rec &r) { const uint64_t j = jb + k; if (j >= j0 && j < j1) o[j - j0] = r; });
        }
    };
}

// hs.rec_of: the prefix sums of the reads' record counts (counted by cl_push_reads' walk)
cl_status build_rec_index(cl_ctx *c)
{
    const size_t n = c->hs.pos.size();
    RawVec<uint32_t> &ro = c->hs.rec_of;
    ro.resize(n + 1);
    ro[0] = 0u;
    if (!c->acc.rec_counted) {
        // some tile looked like long reads and skipped the count, yet the contig as a whole gets the short-read form
        const int32_t *hp = c->hs.pos.data(); const uint8_t *hm = c->hs.mapq.data(); const uint32_t *he = c->hs.end.data();
        const uint32_t *hc = c->hs.cigar_off.data(), *hcig = c->hs.cigar.data(); const unsigned long long *hq = c->hs.qual_off.data();
        const uint32_t min_mapq = c->opt.min_mapping_quality;
        uint32_t *cw = c->hs.rec_cnt.data();
        dut::parallel_for(n, dut::grain_for(n, 65536), [&](size_t i) {
            cw[i] = gen_read_recs(hp[i], he[i], hm[i], min_mapq, hcig + hc[i], hc[i + 1] - hc[i], 0ull, hq[i + 1] - hq[i], [](uint32_t, const ReadRec &) {});
        });
        c->acc.rec_counted = true;
    }
    const uint32_t *cnt = c->hs.rec_cnt.data();
    const size_t grain = dut::grain_for(n, 262144), nchunk = n ? (n + grain - 1) / grain : 0;
    std::vector<uint64_t> tot(nchunk + 1, 0);
    dut::parallel_for(nchunk, 1, [&](size_t k) {
        const size_t a = k * grain, b = std::min(n, a + grain);
        uint64_t t = 0;
        for (size_t i = a; i < b; ++i) t += cnt[i];
        tot[k + 1] = t;
    });
    for (size_t k = 0; k < nchunk; ++k) tot[k + 1] += tot[k];
    if (tot[nchunk] >= (1ull << 29)) return fail(c, CL_ERR_RANGE, "more than 2^29 read records in one contig");
    dut::parallel_for(nchunk, 1, [&](size_t k) {
        const size_t a = k * grain, b = std::min(n, a + grain);
        uint32_t run = (uint32_t)tot[k];
        for (size_t i = a; i < b; ++i) { run += cnt[i]; ro[i + 1] = run; }
    });
    c->n_rec = (uint32_t)tot[nchunk];
    return CL_OK;
}

// The windows' candidate ranges: an index of the resident reads (binary searches over the sorted positions), built on
// the host at upload -- where the positions still are -- instead of in every run (round 1 ran the same rules as a
// device function in front of every pileup launch; the parity tests hold the results of this one against the oracle).
void host_window_bounds(const cl_ctx *c, std::vector<WinMeta> &win, uint32_t &flags)
{
    const uint32_t n = (uint32_t)c->hs.pos.size(), n_wide = (uint32_t)c->hs.wide_pos.size();
    const int32_t *pos = c->hs.pos.data(), *wpos = c->hs.wide_pos.data();
    auto lb = [](const int32_t *p, uint32_t cnt, long long key) {
        return (uint32_t)(std::lower_bound(p, p + cnt, key, [](int32_t v, long long k) { return (long long)v < k; }) - p);
    };
    std::atomic<uint32_t> fl{0};
    win.resize((size_t)c->n_win + 1);
    dut::parallel_for(c->n_win, 512, [&](size_t w) {
        const long long W = (long long)w * kT;
        WinMeta m;
        m.lo = lb(pos, n, W - (long long)c->acc.span_n + 1);
        m.hi = lb(pos, n, W + (long long)kT);
        m.wlo = 0; m.wn = 0;
        if (n_wide) {
            m.wlo = lb(wpos, n_wide, W - (long long)c->acc.span_w + 1);
            m.wn = lb(wpos, n_wide, W - (long long)c->acc.span_n + 1) - m.wlo;
        }
        m.q0 = 0; m.rlo = 0; m.rn = 0;
        if (!c->bits) {
            // the byte forms of k_pileup address the quality bytes of a window with 32-bit offsets
            const uint32_t first = m.wn ? c->hs.wide_idx[m.wlo] : m.lo;      // lo <= n: the offsets array has n + 1 entries
            const unsigned long long qf = c->hs.qual_off[first], qh = c->hs.qual_off[m.hi];
            m.q0 = qf;
            if (m.hi > first && qh - qf > 0xFFFF0000ull) fl.fetch_or(kErrRange);
        }
        win[w] = m;
    });
    flags = fl.load();
}

// ... and, once the host's walks over the reads of the windows are done (run table, rows: they index reads), the ranges as
// the kernel wants them: the record forms' candidates are records -- those of the reads [lo, hi) lie side by side, the
// wide reads' are listed in wide_rec (wro: the prefix sums of the wide reads' record counts).
void finish_windows(const cl_ctx *c, const std::vector<uint32_t> &wro_v, std::vector<WinMeta> &win, uint32_t &flags)
{
    static const uint32_t kZero[1] = {0u};
    const uint32_t *wro = wro_v.empty() ? kZero : wro_v.data();      // (no wide read: wlo = wn = 0 everywhere)
    std::atomic<uint32_t> fl{0};
    dut::parallel_for(c->n_win, 4096, [&](size_t w) {
        WinMeta &m = win[w];
        if (c->form != 2) {
            const uint32_t *ro = c->hs.rec_of.data();
            m.lo = ro[m.lo]; m.hi = ro[m.hi];
            const uint32_t w1 = wro[m.wlo + m.wn];
            m.wlo = wro[m.wlo]; m.wn = w1 - m.wlo;
        }
        // more candidates than the 16-bit differences of the pileup kernels can hold: the 32-bit variant is needed
        if ((m.hi - m.lo) + m.wn > 32767u) fl.fetch_or(kNeedDeep);
    });
    flags |= fl.load();
}

// The run table of the run-table form (pileup_bytes.hip.h, LONG = 2): per window of kT positions the M/=/X pieces of the reads
// that cover it -- what the reference's column walk visits as (alignment, qpos) with !is_del (mod.rs:30-37), grouped by
// window instead of by column.  One more walk over the staged CIGARs, at upload: a thread takes a range of windows
// and sweeps it with a list of read cursors (operation index, reference and query position), so every operation is
// visited once per range it touches; reads that start before the range enter at their last checkpoint in front of it
// (the 64-operation checkpoints of cl_push_reads' walk).  Reads below min_mapping_quality never enter (mod.rs:25).
// A piece = {x, y}: x + 16 u = the byte offset of unit u's qualities from the window's quality base;
// y = start | end - 1 << 11 | (read & 1) << 29 | valid << 31; it covers the unit of its start and at most the next one.
// The pieces go to HBM through stream_windows<RunTableForm>, below.
struct RunCur { uint32_t k, k1, x, y, qlen, flags; unsigned long long q0; };

// One window: the cursors of `act` emit their pieces inside [W, W + kT) to out[0, cap) and move on; finished reads
// leave the list.  Returns the number of pieces, or SIZE_MAX when `cap` did not suffice (the list is then spoilt: the
// caller restores its copy).
// `qend` = bytes of the padded quality allocation: every piece is checked against it as it is emitted -- the kernel loads
// 16 bytes at allocation offset qwin + (uint32)(x + 16 u) for the unit(s) of the piece, and the lanes behind a window's
// last entry repeat that entry's loads -- and *out_of_range is set when a load would leave the allocation (the upload then
// fails with CL_ERR_RANGE instead of launching a kernel that faults).
size_t sweep_window(std::vector<RunCur> &act, const uint32_t *cig, uint32_t W, unsigned long long qwin, uint2 *out, size_t cap,
                    unsigned long long qend, std::atomic<bool> *out_of_range)
{
    const uint32_t Wend = W + kT;
    size_t n = 0, keep = 0;
    const size_t na = act.size();
    for (size_t i = 0; i < na; ++i) {
        RunCur cu = act[i];
        // every piece of an operation that starts at (x, y) has the same first word: q + kQualPad - sr with q = qrel + y +
        // (sp - x) and sr = sp - W
        const uint32_t qb = (uint32_t)(cu.q0 - qwin) + (uint32_t)kQualPad + W;
        while (cu.k < cu.k1 && cu.x < Wend) {
            const uint32_t cw = cig[cu.k], op = cw & 15u, l = cw >> 4;
            const uint32_t radv = (0x18Du >> op) & 1u, qadv = (0x193u >> op) & 1u, ism = (0x181u >> op) & 1u;
            const uint32_t xe = cu.x + (radv ? l : 0u);
            if (ism) {
                if (n + (kT / 32u + 2u) > cap) return SIZE_MAX;                 // what one clipped run can emit at most
                const uint32_t sp = cu.x > W ? cu.x : W;
                const uint32_t lq = cu.y < cu.qlen ? std::min(cu.qlen - cu.y, l) : 0u;   // bases that have a quality byte
                uint32_t tp = xe < Wend ? xe : Wend;
                tp = (cu.x + lq) < tp ? (cu.x + lq) : tp;
                if (sp < tp) {
                    uint32_t sr = sp - W;
                    const uint32_t tr = tp - W, ex = qb + cu.y - cu.x;
                    do {
                        const uint32_t pe = std::min(tr, ((sr >> 4) + 2u) << 4);
                        out[n++] = make_uint2(ex, sr | ((pe - 1u) << 11) | cu.flags);
                        // the first and the last unit the kernel loads for this piece, as it computes their addresses
                        if (qwin + (uint32_t)(ex + ((sr >> 4) << 4)) + 16ull > qend || qwin + (uint32_t)(ex + (((pe - 1u) >> 4) << 4)) + 16ull > qend)
                            out_of_range->store(true, std::memory_order_relaxed);
                        sr = pe;
                    } while (sr < tr);
                }
            }
            if (xe > Wend) break;                                // the operation goes on in the next window
            if (xe < cu.x) { cu.k = cu.k1; break; }              // wraps the 32-bit coordinate: flagged kErrRange by cl_push_reads
            cu.x = xe; cu.y += qadv ? l : 0u; cu.k += 1u;
        }
        if (cu.k < cu.k1) act[keep++] = cu;
    }
    act.resize(keep);
    return n;
}

// pieces per pinned buffer (DUT_RUN_CHUNK: a test hook that makes the buffer-full and oversized-window paths reachable
// with small inputs; read once)
size_t run_chunk_entries()
{
    static const size_t n = [] {
        const char *e = getenv("DUT_RUN_CHUNK");
        const size_t full = PinRing::kPinBytes / sizeof(uint2);
        const size_t v = e ? (size_t)strtoull(e, nullptr, 0) : full;
        return v < kT / 32u + 2u ? kT / 32u + 2u : (v > full ? full : v);
    }();
    return n;
}

// host views of the staged contig for the run table's sweep (what dut::RowReads is for the rows')
struct RunReads {
    const int32_t *pos;
    const uint8_t *mapq;
    const uint32_t *end, *coff, *cig, *ckx, *cky;
    const unsigned long long *qoff;
    uint32_t min_mapq;
    uint32_t inject_read;                         // DUT_FAULT_INJECT=runtab: the read whose quality offset is moved out of range
};

RunReads run_reads(const cl_ctx *c)
{
    RunReads H;
    H.pos = c->hs.pos.data(); H.mapq = c->hs.mapq.data(); H.end = c->hs.end.data();
    H.coff = c->hs.cigar_off.data(); H.cig = c->hs.cigar.data(); H.ckx = c->hs.ck_x.data(); H.cky = c->hs.ck_y.data();
    H.qoff = c->hs.qual_off.data();
    H.min_mapq = c->opt.min_mapping_quality;
    H.inject_read = fault_injected("runtab") ? c->n_reads / 2u : 0xFFFFFFFFu;
    return H;
}

// a read that covers positions at or after W enters the sweep (reads below min_mapq never do, mod.rs:25): at its first
// operation, or -- a read of more than kLongOps operations that starts before W -- at its last checkpoint at or before W
inline void run_enter(std::vector<RunCur> &act, const RunReads &H, uint32_t r, uint32_t W)
{
    if (H.mapq[r] < H.min_mapq) return;
    RunCur cu;
    cu.k = H.coff[r]; cu.k1 = H.coff[r + 1]; cu.x = (uint32_t)H.pos[r]; cu.y = 0;
    if (cu.k >= cu.k1 || H.end[r] <= W) return;
    const unsigned long long ql = H.qoff[r + 1] - H.qoff[r];
    cu.qlen = ql > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)ql;
    cu.q0 = H.qoff[r]; cu.flags = ((r & 1u) << 29) | 0x80000000u;
    if (r == H.inject_read) cu.q0 += 0x7FFFFFF0ull;
    if (cu.k1 - cu.k > kLongOps && cu.x < W) {
        const uint32_t jlo = (cu.k + 63u) >> 6, jhi = (cu.k1 - 1u) >> 6;
        if (jlo <= jhi && H.ckx[jlo] <= W) {
            uint32_t lo_j = jlo, hi_j = jhi;
            while (lo_j < hi_j) {
                const uint32_t mid = lo_j + ((hi_j - lo_j + 1u) >> 1);
                if (H.ckx[mid] <= W) lo_j = mid; else hi_j = mid - 1u;
            }
            cu.k = lo_j << 6; cu.x = H.ckx[lo_j]; cu.y = H.cky[lo_j];
        }
    }
    act.push_back(cu);
}

// units of rows per pinned buffer (DUT_ROW_CHUNK, in kilobytes = 8 units: a test hook that makes the buffer-full and
// oversized-window paths reachable with small inputs; read once)
size_t row_chunk_units()
{
    static const size_t n = [] {
        constexpr size_t kPerKB = 1024 / (dut::kRowUnitWords * sizeof(uint32_t));
        const char *e = getenv("DUT_ROW_CHUNK");
        const size_t full = PinRing::kPinBytes / 1024;
        const size_t v = e ? (size_t)strtoull(e, nullptr, 0) : full;
        return (v < 1 ? 1 : (v > full ? full : v)) * kPerKB;
    }();
    return n;
}

// DUT_ROWS_UNIFORM=1, read when a context is made (a test and A/B hook: the equal-heights form of every window, that is
// the bytes of one stack per window through the segments' code)
bool rows_uniform_env() { const char *e = getenv("DUT_ROWS_UNIFORM"); return e && *e == '1'; }

dut::RowReads row_reads(const cl_ctx *c)
{
    dut::RowReads H;
    H.pos = c->hs.pos.data(); H.end = c->hs.end.data(); H.mapq = c->hs.mapq.data();
    H.off = c->hs.rb_off.data(); H.bits = c->hs.qbits.data();
    H.sc_off = c->hs.sc_off.data(); H.sc = c->hs.sc.data();
    H.min_mapq = c->opt.min_mapping_quality;
    return H;
}

// the first size of the row array, in units: per window of mean depth d eight stacks of ~1.45 d rows (a window's ONE
// stack stood at ~1.7 d, and a stack per segment stores 0.85 to 0.96 of that), a quarter of that in units, one unit of
// rounding per segment (cl_contig_reserve allocates by it ahead of the upload)
uint64_t row_units_estimate(uint64_t n_qual, uint64_t n_win) { return (n_qual / kT) * 31 / 10 + n_win * dut::kRowSegments + 8192; }

// What differs between the two tables that stream_windows builds: the unit a window is made of (Word x kUnitWords), how
// many units a pinned buffer holds, the device array (in units), the cursor of a read and how it enters and is swept,
// what a window's record says of its units (Form::record: rn, and whatever else the form keeps there), what is checked
// and kept at the end, and the messages.
struct RunTableForm {                     // byte form, long reads: a unit = a match piece (sweep_window)
    using Word = uint2;
    using Cur = RunCur;
    struct Scratch {};
    static constexpr size_t kUnitWords = 1;
    static constexpr const char *kTooMany = "more than 2^32 match pieces in one contig";
    static constexpr const char *kNoFit = "run table: the second sizing pass did not fit";
    cl_ctx *c;
    const RunReads H;
    const unsigned long long qend;
    std::atomic<bool> oor{false};
    explicit RunTableForm(cl_ctx *c_) : c(c_), H(run_reads(c_)), qend(c_->n_qual + 2ull * kQualPad) {}
    static size_t chunk_units() { return run_chunk_entries(); }
    uint64_t estimate() const { return c->n_qual / 12 + (uint64_t)c->n_win * 8 + 65536; }   // a piece per ~12 aligned bases
    hipError_t reserve(uint64_t units) { return c->d_runtab.reserve(units); }
    Word *table() const { return c->d_runtab.p; }
    uint64_t capacity() const { return c->d_runtab.cap; }
    void enter(std::vector<Cur> &act, uint32_t r, uint32_t W) const { run_enter(act, H, r, W); }
    size_t window(std::vector<Cur> &act, uint32_t W, const WinMeta &m, Word *out, size_t cap, Scratch &) { return sweep_window(act, H.cig, W, m.q0, out, cap, qend, &oor); }
    static void record(WinMeta &m, size_t cnt, const Scratch &) { m.rn = (uint32_t)std::min<size_t>(cnt, 0xFFFFFFFFu); }
    cl_status check() { return oor.load() ? fail(c, CL_ERR_RANGE, "a match piece of the run table addresses quality bytes outside the resident array") : CL_OK; }
    void done(uint64_t total, uint32_t) { c->n_runtab = total; }
};

struct RowsForm {                         // pass-bit form: a unit = 4 rows of one segment of a window (pass_rows.h)
    using Word = uint32_t;
    using Cur = dut::RowCur;
    using Scratch = dut::SegScratch;
    static constexpr size_t kUnitWords = dut::kRowUnitWords;
    static constexpr const char *kTooMany = "more than 2^32 units of pass-bit rows in one contig";
    static constexpr const char *kNoFit = "pass-bit rows: the second sizing pass did not fit";
    cl_ctx *c;
    const dut::RowReads H;
    explicit RowsForm(cl_ctx *c_) : c(c_), H(row_reads(c_)) {}
    static size_t chunk_units() { return row_chunk_units(); }
    uint64_t estimate() const { return row_units_estimate(c->n_qual, c->n_win); }
    hipError_t reserve(uint64_t units) { return c->d_rows.reserve(units * (kUnitWords / 4)); }
    Word *table() const { return reinterpret_cast<Word *>(c->d_rows.p); }
    uint64_t capacity() const { return c->d_rows.cap / (kUnitWords / 4); }
    void enter(std::vector<Cur> &act, uint32_t r, uint32_t W) const { dut::rows_enter(act, H, r, W); }
    size_t window(std::vector<Cur> &act, uint32_t W, const WinMeta &, Word *out, size_t cap, Scratch &sc) { return dut::rows_window_segments<kT>(act, H, W, out, cap, sc, c->rows_uniform); }
    // the record of a window of `cnt` units: rn = its highest segment, the eight heights as the bytes of q0 (kernels.hip.h)
    static void record(WinMeta &m, size_t, const Scratch &sc) { m.rn = sc.most; m.q0 = sc.word; }
    cl_status check() { return CL_OK; }
    void done(uint64_t total, uint32_t most) { c->n_row_groups = total; c->max_groups = most; }   // most: picks the counter planes
};

// A per-window table of the resident contig, built at upload and streamed to HBM: a thread takes a range of windows
// and sweeps it with a list of read cursors (Form::enter, Form::window); the units of a window are written straight
// into the pinned buffers of the staging ring, a buffer leaves when the next window no longer fits, buffers are placed
// in the device array in the order they fill (a window only needs its own units contiguous: its record holds their
// index), so the table exists nowhere in host memory.  win[w].rlo = first unit, rn by Form::record (the number of units, or
// the pass-bit form's highest segment); a window that no read's cursor reaches gets rlo = rn = 0.
template <class Form>
cl_status stream_windows(cl_ctx *c, std::vector<WinMeta> &win)
{
    using Word = typename Form::Word;
    constexpr size_t UW = Form::kUnitWords;
    const uint32_t n_win = c->n_win;
    if (n_win == 0) return CL_OK;
    cl_status s = ensure_pins(c);
    if (s != CL_OK) return s;
    Form F(c);
    const uint32_t *wide_idx = c->hs.wide_idx.data();
    // (as many walkers as the staging ring has buffer pairs -- DUT_COPY_THREADS, 8 by default --: pinning 16 MB more per
    // further walker costs more than the walker saves: 73 ms with 16 walkers against 23 ms with 8 at chr21 30x)
    const int nt = std::max(1, std::min<int>(std::max(1, c->ring->slots), dut::worker_threads()));
    // tasks: several per thread so that uneven depth evens out, not so short that the range-start walks show
    const size_t per = std::max<size_t>(16, (size_t)n_win / (8 * (size_t)nt) + 1);
    const size_t ntasks = ((size_t)n_win + per - 1) / per;
    const size_t capU = Form::chunk_units();
    // the device array: an estimate first; a contig that needs more tells how much
    uint64_t want = F.estimate();
    for (int attempt = 0; attempt < 2; ++attempt) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, F.reserve(want));
        Word *const d_tab = F.table();
        const uint64_t dev_cap = F.capacity();
        std::atomic<uint64_t> dev_next{0};
        std::atomic<size_t> next_task{0};
        std::atomic<uint32_t> most{0};                           // the largest rn of any window
        PinRing *R = c->ring.get();
        R->acquire(static_cast<EngineBase *>(c));                // (the identity ring_finish releases it under)
        c->ring_held = true;
        if (!R->ensure_slots(nt)) { (void)ring_finish(c); return fail(c, CL_ERR_DEVICE, "cannot extend the pinned staging ring (hipHostMalloc)"); }
        for (int t = 0; t < PinRing::kCopyThreads; ++t) c->copy_err[t] = hipSuccess;
        c->crew_busy = true;
        R->crew.start(nt, [&](int t) {
                hipError_t err = hipSetDevice(c->device);
                int kb = 0;                                                  // buffers this thread has sent
                auto cur_buf = [&]() { return reinterpret_cast<Word *>(R->pin[t][kb & 1]); };
                auto send = [&](Word *dst, size_t units) {                   // the current buffer leaves; on to the other one
                    if (err != hipSuccess) return;
                    err = hipMemcpyAsync(dst, cur_buf(), units * UW * sizeof(Word), hipMemcpyHostToDevice, R->copy_stream[t]);
                    if (err == hipSuccess) err = hipEventRecord(R->pin_ev[t][kb & 1], R->copy_stream[t]);
                    ++kb;
                    if (kb >= 2 && err == hipSuccess) err = hipEventSynchronize(R->pin_ev[t][kb & 1]);   // its previous transfer is done
                };
                std::vector<typename Form::Cur> act, save;
                std::vector<uint32_t> in_buf;                                // windows whose units lie in the current buffer
                typename Form::Scratch scr;
                RawVec<Word> big;
                size_t used = 0;
                uint32_t my_most = 0;
                auto flush = [&]() {
                    if (!used) return;
                    const uint64_t off = dev_next.fetch_add(used);
                    if (off + used <= dev_cap) send(d_tab + off * UW, used);  // else: the array is too small, only the total counts now
                    for (uint32_t w : in_buf) win[w].rlo += (uint32_t)off;
                    in_buf.clear(); used = 0;
                };
                walker_guarded(err, [&] {
                    size_t task;
                    while ((task = next_task.fetch_add(1)) < ntasks) {
                        const size_t w0 = task * per, w1 = std::min<size_t>(n_win, w0 + per);
                        act.clear();
                        for (size_t w = w0; w < w1; ++w) {
                            const uint32_t W = (uint32_t)(w * kT);
                            WinMeta &m = win[w];
                            if (w == w0) {
                                // what covers the range's first window: the wide reads in front of read lo, then [lo, hi)
                                for (uint32_t i = 0; i < m.wn; ++i) F.enter(act, wide_idx[m.wlo + i], W);
                                for (uint32_t r = m.lo; r < m.hi; ++r) F.enter(act, r, W);
                            } else {
                                for (uint32_t r = win[w - 1].hi; r < m.hi; ++r) F.enter(act, r, W);   // the reads that start in this window
                            }
                            if (act.empty()) { m.rlo = 0; m.rn = 0; continue; }
                            save = act;
                            size_t cnt = F.window(act, W, m, cur_buf() + used * UW, capU - used, scr);
                            if (cnt == SIZE_MAX) {                           // the buffer is full: it leaves, the window starts over
                                flush();
                                act = save;
                                cnt = F.window(act, W, m, cur_buf(), capU, scr);
                            }
                            if (cnt == SIZE_MAX) {
                                // a window that no buffer holds (depth in the thousands): through a block of its own
                                size_t bc = capU * 4;
                                for (;;) {
                                    big.clear(); big.resize(bc * UW);
                                    act = save;
                                    cnt = F.window(act, W, m, big.data(), bc, scr);
                                    if (cnt != SIZE_MAX) break;
                                    bc *= 4;
                                }
                                const uint64_t off = dev_next.fetch_add(cnt);
                                if (off + cnt <= dev_cap && err == hipSuccess)
                                    err = hipMemcpy(d_tab + off * UW, big.data(), cnt * UW * sizeof(Word), hipMemcpyHostToDevice);
                                m.rlo = (uint32_t)off; Form::record(m, cnt, scr);
                                my_most = std::max(my_most, m.rn);
                                continue;
                            }
                            m.rlo = (uint32_t)used; Form::record(m, cnt, scr);
                            my_most = std::max(my_most, m.rn);
                            if (cnt) in_buf.push_back((uint32_t)w);
                            used += cnt;
                        }
                    }
                    flush();
                });
                for (int b = 0; b < 2 && b < kb; ++b) { const hipError_t e = hipEventSynchronize(R->pin_ev[t][b]); if (err == hipSuccess) err = e; }
                uint32_t seen = most.load();
                while (seen < my_most && !most.compare_exchange_weak(seen, my_most)) {}
                c->copy_err[t] = err;
        });
        s = ring_finish(c);
        if (s != CL_OK) return s;
        const uint64_t total = dev_next.load();
        if ((s = F.check()) != CL_OK) return s;
        if (total >= 0xFFFFFFF0ull) return fail(c, CL_ERR_RANGE, Form::kTooMany);
        if (total <= dev_cap) { F.done(total, most.load()); return CL_OK; }
        want = total;                                            // exact now: once more
    }
    return fail(c, CL_ERR_DEVICE, Form::kNoFit);
}

// The device buffers whose size follows from the number of windows, each with its element count: f(buffer, elements).
// The reference is d_refn (a bit per position) in the pass-bit form, d_ref (the bytes) in the byte forms.
template <class F> void each_extent_buffer(cl_ctx *c, size_t n_win, bool pass_bits, F &&f)
{
    const size_t padded = n_win * kT;
    // (d_win_words: k_tail reads the words four at a time, so the array holds whole quads -- kernels.hip.h: quad_at)
    // (d_winpart, in 16-byte words: a WinRecord per window in the pass-bit form, a WinPartial in the byte forms)
    f(c->d_win, n_win + 1); f(c->d_win_words, n_win + 4); f(c->d_winpart, (n_win + 1) * ((pass_bits ? sizeof(WinRecord) : sizeof(WinPartial)) / sizeof(uint4)));
    f(c->d_runs, padded + 16); f(c->d_win_wide, n_win + 1);
    if (pass_bits) f(c->d_refn, padded / 32 + 4); else f(c->d_ref, padded + 16);
}

// allocate and lay out everything that depends on the extent (called by cl_contig_upload, the staged arrays still there)
cl_status size_for_extent(cl_ctx *c, uint32_t extent)
{
    c->extent = extent;
    c->n_win = (uint32_t)(((uint64_t)extent + kT - 1) / kT);
    const size_t padded = (size_t)c->n_win * kT;
    hipError_t alloc = hipSuccess;
    each_extent_buffer(c, c->n_win, c->form == 3, [&](auto &buf, size_t n) { if (alloc == hipSuccess) alloc = buf.reserve(n); });
    HIP_TRY(c, alloc);
    HIP_TRY(c, hipMemsetAsync(c->d_win_wide.p, 0, c->n_win + 1, c->stream));
    // (k_tail reads whole quads of packed words: the padding behind the last window's is never counted, and is zero)
    HIP_TRY(c, hipMemsetAsync(c->d_win_words.p, 0, ((size_t)c->n_win + 4) * sizeof(uint32_t), c->stream));
    // reference bytes: [0,ref_len) from the caller, 'N' beyond (mod.rs:79-80).  The pass-bit form needs one bit of a
    // base -- is it 'N' / 'n' (mod.rs:100-101) --, taken here, where the bytes pass through the host's hands anyway:
    // 1/8 of the transfer, 1/8 of what every run reads
    {
        const uint8_t *ref = c->hs.ref.data();
        const uint64_t nref = std::min<uint64_t>(c->hs.ref.size(), padded);
        cl_status rs;
        if (c->form == 3)
            rs = ring_start(c, reinterpret_cast<uint8_t *>(c->d_refn.p), padded / 8, [ref, nref](uint64_t off, uint64_t len, uint8_t *out) {
                // (a buffer of the ring is a whole number of 64-bit words: 4 MB, and padded / 8 = 256 bytes per window)
                const uint64_t p = off * 8;
                dut::ref_n_words(ref + std::min<uint64_t>(p, nref), p < nref ? nref - p : 0, len / 8, reinterpret_cast<uint64_t *>(out), dut::qual_pack_level());
            });
        else rs = ring_start(c, c->d_ref.p, padded + 16, [ref, nref](uint64_t off, uint64_t len, uint8_t *out) {
            const uint64_t have = off < nref ? std::min<uint64_t>(len, nref - off) : 0;
            if (have) memcpy(out, ref + off, have);
            if (have < len) memset(out + have, 'N', len - have);
        });
        // ... beside it, the windows' candidate ranges
        std::vector<WinMeta> win;
        uint32_t flags = 0;
        host_window_bounds(c, win, flags);
        if (rs == CL_OK) rs = ring_finish(c); else (void)ring_finish(c);
        if (rs != CL_OK) return rs;
        c->n_runtab = 0; c->n_row_groups = 0; c->max_groups = 0;
        if (c->form == 3) {
            // the windows' pass-bit rows: one more walk over the staged CIGARs, streamed to HBM through the ring
            StageTimer tr;
            rs = stream_windows<RowsForm>(c, win);
            if (rs != CL_OK) return rs;
            tr.lap("upload: pass-bit rows (walk + H2D)");
        }
        if (c->form == 2 && !(flags & kErrRange)) {
            // the windows' match pieces: one more walk over the staged CIGARs, streamed to HBM through the ring
            StageTimer tr;
            rs = stream_windows<RunTableForm>(c, win);
            if (rs != CL_OK) return rs;
            tr.lap("upload: run table (walk + H2D)");
        }
        // DUT_VALIDATE=1 (tooling: tools/fuzz_parity.py sets it): what the kernels will index is checked on the host before
        // anything is launched -- candidate ranges against the resident arrays, and every entry of the run table (read
        // back from the device) against the quality array -- so that a bad index is an error message, not a GPU fault
        finish_windows(c, c->hs.wide_rec_of, win, flags);
        // what k_pileup_rows streams per window must lie inside the resident rows: checked in the product build, once per
        // contig (an index past the array is an error return, not a device fault)
        if (c->form == 3) {
            std::atomic<bool> bad{false};
            const uint64_t ngr = c->n_row_groups;
            if (fault_injected("rows") && c->n_win) win[c->n_win / 2].rlo += 0x7FFFFFF0u;
            dut::parallel_for(c->n_win, 8192, [&](size_t w) {
                const uint64_t units = dut::rows_window_units(win[w].rn, win[w].q0);
                // (the kernels address a window's units with 32-bit byte offsets, below 2^31: pileup_rows.hip.h, row_lane)
                if ((uint64_t)win[w].rlo + units > ngr || units >= (1ull << 24)) bad.store(true);
            });
            if (bad.load()) return fail(c, CL_ERR_RANGE, "a window's pass-bit rows lie outside the resident row array, or take 2 GB or more");
        }
        static const bool validate = [] { const char *e = getenv("DUT_VALIDATE"); return e && *e == '1'; }();
        if (validate && !(flags & kErrRange)) {
            const uint64_t n_cand = c->form != 2 ? c->n_rec : c->hs.pos.size();
            uint64_t n_wide_list = c->hs.wide_idx.size();
            if (c->form != 2) n_wide_list = c->hs.wide_rec_of.empty() ? 0 : c->hs.wide_rec_of.back();
            std::vector<uint2> tab;
            if (c->form == 2 && c->n_runtab) {
                tab.resize(c->n_runtab);
                HIP_TRY(c, hipMemcpy(tab.data(), c->d_runtab.p, c->n_runtab * sizeof(uint2), hipMemcpyDeviceToHost));
            }
            const uint64_t qend = c->n_qual + 2 * (uint64_t)kQualPad;
            for (uint32_t w = 0; w < c->n_win; ++w) {
                const WinMeta &m = win[w];
                char msg[256];
                if (m.lo > m.hi || m.hi > n_cand || (uint64_t)m.wlo + m.wn > n_wide_list) {
                    snprintf(msg, sizeof(msg), "validate: window %u: candidates [%u, %u) of %llu, wide [%u, +%u) of %llu", w, m.lo, m.hi, (unsigned long long)n_cand, m.wlo, m.wn, (unsigned long long)n_wide_list);
                    return fail(c, CL_ERR_DEVICE, msg);
                }
                if (c->form != 2) continue;
                if ((uint64_t)m.rlo + m.rn > c->n_runtab) {
                    snprintf(msg, sizeof(msg), "validate: window %u: run table entries [%u, +%u) of %llu", w, m.rlo, m.rn, (unsigned long long)c->n_runtab);
                    return fail(c, CL_ERR_DEVICE, msg);
                }
                for (uint32_t i = 0; i < m.rn; ++i) {
                    const uint2 d = tab[(size_t)m.rlo + i];
                    const uint32_t sr = d.y & 2047u, er = (d.y >> 11) & 2047u, u0 = sr >> 4, u1 = er >> 4;
                    // the kernel adds the unit's 16 u to x in 32 bits and that to the window's base (allocation-relative: q0)
                    const unsigned long long off = m.q0 + (uint32_t)(d.x + (u1 << 4)) + 16ull;   // end of the last byte it loads for the entry
                    if (!(d.y >> 31) || er < sr || u1 > u0 + 1u || off > qend || m.q0 + (uint32_t)(d.x + (u0 << 4)) + 16ull > qend) {
                        snprintf(msg, sizeof(msg), "validate: window %u entry %u: x %u y 0x%08x (start %u end-1 %u), q0 %llu: loads up to byte %llu of %llu",
                                 w, i, d.x, d.y, sr, er, (unsigned long long)m.q0, off, (unsigned long long)qend);
                        return fail(c, CL_ERR_DEVICE, msg);
                    }
                }
            }
        }
        if (c->n_win) HIP_TRY(c, hipMemcpyAsync(c->d_win.p, win.data(), (size_t)c->n_win * sizeof(WinMeta), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        // a window with more candidates than the 16-bit counters / differences hold: the 32-bit form from the start
        c->deep = (flags & kNeedDeep) != 0;
        c->bounds_err = flags & kErrRange;
    }
    return CL_OK;
}

// The start values of a run's contig summary: zero counts, the host's separable sums (pass-bit form), the extent.
DevSummary summary_start_values(const cl_ctx *c)
{
    DevSummary s0{};
    if (c->form == 3) { s0.summed_baseq = c->dev_sum_q; s0.summed_coverage = c->dev_sum_cov; s0.summed_mapq = c->dev_sum_mapq; }
    s0.extent = c->extent;
    return s0;
}

// windows per workgroup of k_tail: kTailMinWpc while that takes no more than `max_chunks` workgroups, else what fills
// max_chunks, rounded up to a multiple of 16 (the kernel's waves) -- so that what every workgroup re-reads of the windows
// before its own stays linear in the contig's length.  At most kTailMaxWpc, which a thread's four windows of the own
// chunk cover: the cap yields to that (2^21 windows of 2 048 positions are the most a contig has: 4 096 at 512 chunks).
uint32_t tail_wpc(uint32_t n_win, uint32_t max_chunks)
{
    if (max_chunks == 0u) max_chunks = 1u;
    if ((n_win + kTailMinWpc - 1u) / kTailMinWpc <= max_chunks) return kTailMinWpc;
    const uint64_t per = ((uint64_t)n_win + max_chunks - 1u) / max_chunks;
    return (uint32_t)std::min<uint64_t>((per + 15u) & ~15ull, kTailMaxWpc);
}

// what runs behind the pileup kernel, one launch: the windows' run lists -> intervals, the windows' partials -> the
// contig summary (k_tail).  `restart`: the summary's start values are copied by the stream (hipMemcpyAsync from d_sum0)
// instead of by the pileup's window 0 -- the tail alone launched again (cl_contig_collect, a larger interval buffer: the
// summary is accumulated, so it starts over); a contig without windows launches no pileup and gets them this way too.
cl_status launch_tail(cl_ctx *c, bool restart)
{
    const uint32_t cap = (uint32_t)std::min<size_t>(c->d_iv.cap, 0xFFFFFFFFu);
    if (restart || c->n_win == 0)
        HIP_TRY(c, hipMemcpyAsync(c->d_summary.p, c->d_sum0.p, sizeof(DevSummary), hipMemcpyDeviceToDevice, c->stream));
    if (c->n_win == 0) {                                 // nothing to classify: the flags, as the tail leaves them
        HIP_TRY(c, hipMemsetAsync(c->d_errflag.p, 0, 2 * sizeof(uint32_t), c->stream));
        return CL_OK;
    }
    const uint32_t wpc = tail_wpc(c->n_win, c->tail_max_chunks);
    // the summary's workgroups, in front of the grid: kTailSumWindows windows each, at most kTailMaxSum of them
    const uint32_t n_sum = std::min((c->n_win + kTailSumWindows - 1u) / kTailSumWindows, kTailMaxSum);
    const uint32_t wps = (c->n_win + n_sum - 1u) / n_sum;
    // (the windows' totals: the records of k_pileup_rows in the pass-bit form, the WinPartials of k_pileup in the byte forms)
    const auto kern = c->form == 3 ? k_tail<(int)kT, true> : k_tail<(int)kT, false>;
    hipLaunchKernelGGL(kern, dim3(n_sum + (c->n_win + wpc - 1) / wpc), dim3(kTailBlock), 0, c->stream,
                       c->d_runs.p, c->d_win_words.p, static_cast<const void *>(c->d_winpart.p), c->d_errflag.p, c->d_summary.p, c->n_win, c->extent, wpc,
                       n_sum, wps, c->d_iv.p, cap);
    return CL_OK;
}

// What a launch of either pileup kernel is given: one aggregate initialisation in the record's member order, so that a
// member added to the record and not filled here fails the build instead of reaching the device as a null pointer.
#pragma clang diagnostic push
#pragma clang diagnostic error "-Wmissing-field-initializers"
BytesArgs bytes_args(const cl_ctx *c, uint32_t *dbg_raw, uint32_t *dbg_qc, uint32_t *dbg_low)
{
    return BytesArgs{
        Reads{c->d_pos.p, c->d_mapq.p, c->d_qual.p + kQualPad, c->n_reads}, c->dopt,
        c->d_rec.p, c->d_end.p, c->d_win.p, c->d_wide_idx.p, c->d_ref.p, c->d_lut.p, c->d_runtab.p,
        c->d_state.p, c->d_runs.p, c->d_win_words.p, reinterpret_cast<WinPartial *>(c->d_winpart.p),
        reinterpret_cast<unsigned long long *>(c->d_summary.p), reinterpret_cast<const unsigned long long *>(c->d_sum0.p),
        c->extent, c->n_win, (c->n_win + 7) / 8, dbg_raw, dbg_qc, dbg_low,
        (c->n_reads && c->n_qual <= 128ull * c->n_reads) ? 2u : 3u,   // upl: by the mean read length
        c->d_win_wide.p, c->d_errflag.p};
}
RowsArgs rows_args(const cl_ctx *c, uint32_t *dbg_raw, uint32_t *dbg_qc, uint32_t *dbg_low)
{
    return RowsArgs{
        c->d_rows.p, c->d_heads.p, c->d_wide_idx.p, c->d_win.p, c->d_refn.p, c->d_lut8.p,
        c->d_runs.p, c->d_win_words.p, reinterpret_cast<WinRecord *>(c->d_winpart.p),
        reinterpret_cast<unsigned long long *>(c->d_summary.p), reinterpret_cast<const unsigned long long *>(c->d_sum0.p),
        c->extent, c->n_win, (c->n_win + 7) / 8, c->opt.min_depth, c->opt.max_depth,
        c->opt.min_depth_for_low_mapq, c->d_lut.p, c->opt.max_low_mapq_fraction,
        c->d_state.p, dbg_raw, dbg_qc, dbg_low};
}
// ... and what the three depth kernels read of a run (window_depths.hip.h): the first member of their records
DepthResidents depth_residents(const cl_ctx *c)
{
    return DepthResidents{c->d_win.p, c->d_heads.p, c->d_wide_idx.p, c->d_rows.p, c->extent, c->n_win};
}
#pragma clang diagnostic pop

// The instantiation of a depth kernel that fits the resident contig, out of the kernel's table over (counter planes 8, 16,
// 32; heads of 8 bytes, of 4).  A kernel that does not look at one of the two has the same entry along it.
template <class Args> using DepthKernel = void (*)(Args);
template <class Args> DepthKernel<Args> depth_kernel(const cl_ctx *c, const DepthKernel<Args> (&table)[3][2])
{
    const uint32_t np = c->counter_planes();
    return table[np == 8u ? 0 : np == 16u ? 1 : 2][c->heads4 ? 1 : 0];
}
const DepthKernel<DepthArgs> kDepthProfileKernels[3][2] = {{k_depth_profile<8, false>, k_depth_profile<8, true>},
    {k_depth_profile<16, false>, k_depth_profile<16, true>}, {k_depth_profile<32, false>, k_depth_profile<32, true>}};
const DepthKernel<TargetArgs> kTargetDepthKernels[3][2] = {{k_target_depth<8, false>, k_target_depth<8, true>},
    {k_target_depth<16, false>, k_target_depth<16, true>}, {k_target_depth<32, false>, k_target_depth<32, true>}};
const DepthKernel<OrderArgs> kTargetOrderFirstKernels[3][2] = {{k_target_order<8, false, true>, k_target_order<8, true, true>},
    {k_target_order<16, false, true>, k_target_order<16, true, true>}, {k_target_order<32, false, true>, k_target_order<32, true, true>}};
const DepthKernel<OrderArgs> kTargetOrderRoundKernels[3][2] = {{k_target_order<8, false, false>, k_target_order<8, true, false>},
    {k_target_order<16, false, false>, k_target_order<16, true, false>}, {k_target_order<32, false, false>, k_target_order<32, true, false>}};
const DepthKernel<GcArgs> kGcBiasKernels[3][2] = {{k_gc_bias<8, false>, k_gc_bias<8, true>},
    {k_gc_bias<16, false>, k_gc_bias<16, true>}, {k_gc_bias<32, false>, k_gc_bias<32, true>}};
// (only the raw depths come from the heads, and they need no plane; the qc depths are the rows' column sums)
const DepthKernel<RunsArgs> kDepthRunsRawKernels[3][2] = {{k_depth_runs<8, false, false>, k_depth_runs<8, false, true>},
    {k_depth_runs<8, false, false>, k_depth_runs<8, false, true>}, {k_depth_runs<8, false, false>, k_depth_runs<8, false, true>}};
const DepthKernel<RunsArgs> kDepthRunsQcKernels[3][2] = {{k_depth_runs<8, true, false>, k_depth_runs<8, true, false>},
    {k_depth_runs<16, true, false>, k_depth_runs<16, true, false>}, {k_depth_runs<32, true, false>, k_depth_runs<32, true, false>}};

// (the 32-bit counter variant, DEEP, of either kernel is used only when the window bounds asked for it: kNeedDeep)
template <bool DEBUG> void launch_bytes(cl_ctx *c, const BytesArgs &a)
{
    const uint32_t grid = a.n_win8 * 8u;
    if (grid == 0) return;
#define CL_LAUNCH(DEEP_, LONG_) hipLaunchKernelGGL((k_pileup<(int)kT, DEBUG, DEEP_, LONG_>), dim3(grid), dim3(kBlock), 0, c->stream, a)
    if (c->form == 2) { if (c->deep) CL_LAUNCH(true, 2); else CL_LAUNCH(false, 2); }
    else { if (c->deep) CL_LAUNCH(true, 0); else CL_LAUNCH(false, 0); }
#undef CL_LAUNCH
}
template <bool DEBUG> void launch_rows(cl_ctx *c, const RowsArgs &a)
{
    const uint32_t grid = a.n_win8 * 8u;
    if (grid == 0) return;
#define CL_LAUNCH(DEEP_, NP_) do { \
        if (c->heads4) hipLaunchKernelGGL((k_pileup_rows<(int)kT, DEBUG, DEEP_, NP_, true>), dim3(grid), dim3(kRowsBlock), 0, c->stream, a); \
        else hipLaunchKernelGGL((k_pileup_rows<(int)kT, DEBUG, DEEP_, NP_, false>), dim3(grid), dim3(kRowsBlock), 0, c->stream, a); } while (0)
    if (c->counter_planes() == 8u) { if (c->deep) CL_LAUNCH(true, 8); else CL_LAUNCH(false, 8); }
    else if (c->counter_planes() == 16u) { if (c->deep) CL_LAUNCH(true, 16); else CL_LAUNCH(false, 16); }
    else { if (c->deep) CL_LAUNCH(true, 32); else CL_LAUNCH(false, 32); }
#undef CL_LAUNCH
}

cl_status enqueue(cl_ctx *c, bool debug, uint32_t *dbg_raw, uint32_t *dbg_qc, uint32_t *dbg_low)
{
    const bool prof = c->profiling && !debug;
    if (prof) {
        cl_status s = ensure_events(c);
        if (s != CL_OK) return s;
        if (c->ev_pending == cl_ctx::kEvSets) s = harvest_events(c);   // ring full: read back (host sync)
        if (s != CL_OK) return s;
    }
    hipEvent_t *ev = c->ev[c->ev_pending < cl_ctx::kEvSets ? c->ev_pending : 0];
    // d_errflag is zero here: cleared at upload, and by k_tail at the end of every run
    // (a run has no per-read kernel: the read ends and CIGAR checkpoints the long-read forms need are an index the host
    // built at upload; CL_K_PREP stays in the timing table as an empty slot)
    if (prof) HIP_TRY(c, hipEventRecord(ev[0], c->stream));
    if (debug) HIP_TRY(c, c->d_state.reserve((size_t)c->n_win * kT + 16));
    if (c->form == 3) {
        const RowsArgs a = rows_args(c, dbg_raw, dbg_qc, dbg_low);
        if (debug) launch_rows<true>(c, a); else launch_rows<false>(c, a);
    } else {
        const BytesArgs a = bytes_args(c, dbg_raw, dbg_qc, dbg_low);
        if (debug) launch_bytes<true>(c, a); else launch_bytes<false>(c, a);
    }
    if (prof) HIP_TRY(c, hipEventRecord(ev[1], c->stream));
    { const cl_status ts = launch_tail(c, false); if (ts != CL_OK) return ts; }
    if (prof) {
        HIP_TRY(c, hipEventRecord(ev[2], c->stream));
        c->ev_pending += 1;
    }
    HIP_TRY(c, hipGetLastError());
    return CL_OK;
}

// The staged contig's windows one after the other, each with the cursors the upload's walkers would hold there:
// build(w, W, act) runs a row builder over the window and leaves in `act` what goes on into the next one.
template <class Build>
cl_status debug_rows_walk(cl_ctx *c, const char *who, uint32_t *n_windows, Build &&build)
{
    return guarded(c, [&]() -> cl_status {
        if (!c || !c->in_contig || !c->bits) return fail(c, CL_ERR_INVALID, (std::string(who) + ": no staged contig in the pass-bit form").c_str());
        const uint32_t extent = (uint32_t)std::max<uint64_t>(c->contig_len, c->acc.host_max_end);
        const uint32_t n_win = (uint32_t)(((uint64_t)extent + kT - 1) / kT);
        c->n_win = n_win;
        if (n_windows) *n_windows = n_win;
        std::vector<WinMeta> win;
        uint32_t flags = 0;
        host_window_bounds(c, win, flags);
        const dut::RowReads H = row_reads(c);
        std::vector<dut::RowCur> act, save;
        for (uint32_t w = 0; w < n_win; ++w) {
            const uint32_t W = w * kT;
            const WinMeta &m = win[w];
            // (every third window entered afresh, as the first window of a thread's range is -- through the checkpoints of the
            // long reads --, the others carried over from the window before, as inside a range)
            act.clear();
            if (w % 3u == 0u) {
                for (uint32_t i = 0; i < m.wn; ++i) dut::rows_enter(act, H, c->hs.wide_idx[m.wlo + i], W);
                for (uint32_t r = m.lo; r < m.hi; ++r) dut::rows_enter(act, H, r, W);
            } else {
                act = save;
                for (uint32_t r = win[w - 1].hi; r < m.hi; ++r) dut::rows_enter(act, H, r, W);
            }
            build(w, W, H, act);
            save = act;
        }
        return CL_OK;
    });
}

} // namespace

extern "C" {

int cl_abi_version(void) { return CL_ABI_VERSION; }

int cl_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

cl_status cl_create(const cl_options *opt, int device_id, void *stream, cl_ctx **out)
{
    if (!opt || !out) return CL_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n)
        return CL_ERR_DEVICE;
    cl_ctx *c = new (std::nothrow) cl_ctx();
    if (!c) return CL_ERR_NOMEM;
    c->device = device_id;
    c->opt = *opt;
    // DUT_QUAL_FORM=bytes: the quality bytes themselves go to the device and k_pileup tests them there (the byte forms:
    // records for short reads, the run table for long ones) -- the forms of rounds 1-3, kept selectable so that their
    // measurements stay reproducible.  Default: the pass-bit form (k_pileup_rows).  Read per context.
    { const char *qf = getenv("DUT_QUAL_FORM"); c->bits = !(qf && strcmp(qf, "bytes") == 0); }
    // DUT_HEAD_SPAN (a test hook): spans beyond this many positions are cut into several heads -- 2^31 - 1 in earnest, which
    // only a contig of more than 2 Gb can hold; the tests put the seams into ordinary reads
    { const char *h8 = getenv("DUT_HEADS8"); c->heads8_only = h8 && *h8 == '1'; }   // (a test hook: both head forms on one input)
    // DUT_TAIL_CHUNKS=<n> (a test hook, and a column of A/B runs): the most workgroups k_tail gets, instead of kTailMaxChunks --
    // with a small n a few hundred windows reach more than 64 windows per workgroup and a ragged last chunk
    { const char *tc = getenv("DUT_TAIL_CHUNKS"); if (tc) { const unsigned long long v = strtoull(tc, nullptr, 0); if (v >= 1 && v <= 65535) c->tail_max_chunks = (uint32_t)v; } }
    c->rows_uniform = rows_uniform_env();
    { const char *hs = getenv("DUT_HEAD_SPAN"); if (hs) { const unsigned long long v = strtoull(hs, nullptr, 0); if (v >= 1 && v <= kHeadSpanMax) c->head_span = (uint32_t)v; } }
    if (hipSetDevice(device_id) != hipSuccess) { delete c; return CL_ERR_DEVICE; }
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return CL_ERR_DEVICE; }
        c->own_stream = true;
    }
    Opts &o = c->dopt;
    o.min_depth = opt->min_depth; o.max_depth = opt->max_depth; o.min_mapq = opt->min_mapping_quality;
    o.min_depth_for_low_mapq = opt->min_depth_for_low_mapq; o.max_low_mapq = opt->max_low_mapq;
    o.max_low_mapq_fraction = opt->max_low_mapq_fraction;
    // pass_bytes: per byte (x + k + c) >> 1 has bit 7 set iff x >= min_base_quality
    o.ge_k = (opt->min_base_quality == 0 ? 255u : 256u - opt->min_base_quality) * 0x01010101u;
    o.ge_c = opt->min_base_quality == 0 ? 0x01010101u : 0u;
    o.md_all = opt->min_depth > 255 ? 1u : 0u;
    make_ge_consts((uint8_t)(opt->min_depth > 255 ? 255 : opt->min_depth), o.md_add, o.md_or, o.md_and);
    o.xd_on = (opt->max_depth >= 1 && opt->max_depth <= 254) ? 1u : 0u;
    make_ge_consts((uint8_t)(o.xd_on ? opt->max_depth + 1 : 255), o.xd_add, o.xd_or, o.xd_and);
    std::vector<uint32_t> lut;
    build_lut(opt->max_low_mapq_fraction, lut);
    uint32_t lut8[64];
    build_lut8(lut, opt->min_depth_for_low_mapq, lut8);
    bool ok = c->d_lut.reserve(kLutSize) == hipSuccess && c->d_lut8.reserve(64) == hipSuccess &&
              c->d_summary.reserve(1) == hipSuccess && c->d_sum0.reserve(1) == hipSuccess && c->d_errflag.reserve(2) == hipSuccess &&
              hipMemcpy(c->d_lut.p, lut.data(), kLutSize * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(c->d_lut8.p, lut8, sizeof(lut8), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok || ensure_pins(c) != CL_OK) { cl_destroy(c); return CL_ERR_DEVICE; }
    *out = c;
    return CL_OK;
}

void cl_destroy(cl_ctx *c)
{
    if (!c) return;
    if (c->host_only) { delete c; return; }
    (void)hipSetDevice(c->device);
    StageTimer tmr;
    drop_prefetch(c);                                     // its copiers write into d_qual: joined before anything is released
    join_prealloc(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    tmr.lap("destroy: sync");
    c->each_buffer([](auto &buf) { buf.release(); });
    c->d_prof.release(); c->site.release(); c->h_dr_out.release();
    c->d_gc_bits.release(); c->d_gc_out.release(); c->t_gc.destroy();
    c->d_tg_in.release(); c->d_tg_pre.release(); c->d_tg_out.release(); c->d_tg_win.release(); c->d_tg_off.release();
    c->d_to_in.release(); c->d_to_st.release(); c->d_to_out.release();
    c->t_prof.destroy(); c->t_dr_count.destroy(); c->t_dr_write.destroy();
    for (KernelTimer &t : c->t_tg) t.destroy();
    for (KernelTimer &t : c->t_to) t.destroy();
    if (c->ev_made)
        for (auto &set : c->ev)
            for (hipEvent_t e : set) (void)hipEventDestroy(e);
    tmr.lap("destroy: device buffers");
    c->ring.reset();
    tmr.lap("destroy: staging ring");
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    tmr.lap("destroy: stream, context");
}

const char *cl_last_error(const cl_ctx *c) { return c ? c->err.c_str() : "null context"; }

// the staged contig and the record of its pushes as they are without a tile (cl_contig_begin, cl_contig_abort)
static void drop_staged(cl_ctx *c) { c->hs.clear(); c->acc = PushRecord(); }

cl_status cl_contig_begin(cl_ctx *c, int32_t tid, uint32_t contig_len, const uint8_t *ref_bases,
                          uint64_t ref_len)
{
    return guarded(c, [&]() -> cl_status {
        if (!c) return CL_ERR_INVALID;
        if (contig_len > 0xFFF00000u) return fail(c, CL_ERR_RANGE, "contig length beyond the engine's 32-bit range");
        if (ref_len && !ref_bases) return fail(c, CL_ERR_INVALID, "ref_bases is null");
        if (!c->host_only) { drop_prefetch(c); join_prealloc(c); }
        take_staging(c->hs);
        c->tid = tid; c->contig_len = contig_len;
        const uint64_t nref = std::min<uint64_t>(ref_len, contig_len);
        drop_staged(c);
        c->hs.ref.append(ref_bases, nref); c->hs.cigar_off.push_back(0u); c->hs.qual_off.push_back(0ull);
        c->h_iv.clear();
        c->n_wide = 0; c->bounds_err = 0;
        c->in_contig = true; c->uploaded = false; c->ran = false; c->collected = false;
        return CL_OK;
    });
}

namespace {
// quality bytes staged on the host so far go to the device, behind the ones already there
cl_status flush_staged_qual(cl_ctx *c)
{
    if (c->hs.qual.empty()) return CL_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_qual.grow_keep(c->acc.q_dev + c->hs.qual.size() + 2 * kQualPad, kQualPad + c->acc.q_dev, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_qual.p + kQualPad + c->acc.q_dev, c->hs.qual.data(), c->hs.qual.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->acc.q_dev += c->hs.qual.size();
    c->hs.qual.clear();
    return CL_OK;
}
constexpr uint64_t kDirectQual = 4u << 20;   // tiles with at least this many quality bytes skip the host staging copy
} // namespace

cl_status cl_contig_prefetch_qual(cl_ctx *c, const uint8_t *qual, uint64_t n_bytes)
{
    if (!c || !c->in_contig || c->uploaded) return fail(c, CL_ERR_INVALID, "cl_contig_prefetch_qual outside cl_contig_begin .. upload");
    if (c->bits) return CL_OK;                                  // pass-bit form: no quality byte goes to the device
    if (!qual || n_bytes < kDirectQual) return CL_OK;            // small tiles are staged on the host anyway
    return guarded(c, [&] {
        drop_prefetch(c);
        cl_status fs = flush_staged_qual(c);
        if (fs != CL_OK) return fs;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, c->d_qual.grow_keep(c->acc.q_dev + n_bytes + 2 * kQualPad, c->acc.q_dev ? kQualPad + c->acc.q_dev : 0, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        cl_status rs = ring_start(c, c->d_qual.p + kQualPad + c->acc.q_dev, n_bytes,
                                  [qual](uint64_t off, uint64_t len, uint8_t *out) { memcpy(out, qual + off, len); });
        if (rs != CL_OK) { (void)ring_finish(c); return rs; }
        c->pf_src = qual; c->pf_n = n_bytes; c->pf_off = c->acc.q_dev; c->pf_active = true;
        return CL_OK;
    });
}

// Pass-bit form: what cl_contig_upload will need on the device is known from the contig's length and the caller's hint --
// allocated on a thread of its own while the caller admits and pushes the reads (a fresh context spends 15-20 ms of a
// chr21-sized contig's first pass in hipMalloc otherwise).  Only sizes are guessed here: cl_contig_upload reserves what it
// needs again and so makes up for a guess that fell short or an allocation that failed.  Joined before any buffer is used.
static void start_prealloc(cl_ctx *c, uint64_t n_reads, uint64_t n_qual)
{
    join_prealloc(c);
    const uint32_t contig_len = c->contig_len;
    // (one window more than the contig's length gives: the extent may turn out larger than the length)
    const size_t n_win = ((size_t)contig_len + kT - 1) / kT + 1;
    // (heads: 4 bytes each where the reads are short -- a contig of long reads has spans beyond kWideSpan and keeps 8)
    const bool guess4 = !c->heads8_only && n_qual / std::max<uint64_t>(n_reads, 1) < kWideSpan / 8;
    const size_t n_heads = n_reads ? (guess4 ? ((size_t)n_reads + 2) / 2 : (size_t)n_reads + 1) : 0;
    const size_t n_rows = n_qual ? row_units_estimate(n_qual, n_win) * (dut::kRowUnitWords / 4) : 0;
    // nothing to do for a context whose buffers hold this contig already (the usual case from its second contig on):
    // no thread is made for that
    bool enough = c->d_heads.cap >= n_heads && c->d_rows.cap >= n_rows && c->d_iv.cap != 0;
    each_extent_buffer(c, n_win, true, [&](auto &buf, size_t n) { enough = enough && buf.cap >= n; });
    if (enough) return;
    c->prealloc = dut::spawn_or_run([c, n_win, n_heads, n_rows]() {
        if (hipSetDevice(c->device) != hipSuccess) return;
        each_extent_buffer(c, n_win, true, [](auto &buf, size_t n) { (void)buf.reserve(n); });
        (void)c->d_heads.reserve(n_heads); (void)c->d_rows.reserve(n_rows);
        if (c->d_iv.cap == 0) (void)c->d_iv.reserve(1u << 20);
    });
}

cl_status cl_contig_reserve(cl_ctx *c, uint64_t n_reads, uint64_t n_cigar_ops, uint64_t n_qual_bytes)
{
    if (!c || !c->in_contig || c->uploaded) return fail(c, CL_ERR_INVALID, "cl_contig_reserve outside cl_contig_begin .. upload");
    drop_prefetch(c);                                        // the quality buffer may move below
    try {
        c->hs.pos.reserve(n_reads); c->hs.mapq.reserve(n_reads);
        c->hs.cigar_off.reserve(n_reads + 1); c->hs.qual_off.reserve(n_reads + 1);
        c->hs.cigar.reserve(n_cigar_ops);
        if (c->bits) c->hs.qbits.reserve(((n_qual_bytes + 63) >> 6) + 2);
    } catch (const std::bad_alloc &) {
        return fail(c, CL_ERR_NOMEM, "host staging allocation failed");
    }
    if (c->bits) {
        if (!c->host_only && c->hs.pos.empty()) start_prealloc(c, n_reads, n_qual_bytes);
        return CL_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_qual.grow_keep(n_qual_bytes + 2 * kQualPad, c->acc.q_dev ? kQualPad + c->acc.q_dev : 0, c->stream));
    return CL_OK;
}

// a refusal of tile_walk.h as the status of the call, its message in the context
static cl_status push_status(cl_ctx *c, const Offence &f) { return f.st == CL_OK ? CL_OK : fail(c, f.st, f.msg); }

// what both entries check of a tile before they look at a read; `who` names the caller in the one message that does
static cl_status tile_header(cl_ctx *c, const char *who, uint64_t n, const int32_t *pos, const uint8_t *mapq, const uint32_t *cigar_off,
                             const uint32_t *cigar, const uint64_t *qual_off, TileHead &h)
{
    if (!c->in_contig || c->uploaded) return fail(c, CL_ERR_INVALID, std::string(who) + " outside cl_contig_begin .. upload");
    return push_status(c, tile_header(c->hs.pos.size(), n, pos, mapq, cigar_off, cigar, qual_off, h));
}
static WalkOpts walk_opts(const cl_ctx *c) { return {c->contig_len, c->opt.min_mapping_quality, c->opt.min_base_quality, c->head_span}; }

// What the byte forms do with a read in the first pass over a tile (walk_tile; the pass-bit form's share is BitsForm): for
// reads with more than kLongOps operations the (reference, query) position before every operation whose index in the
// contig's CIGAR array is a multiple of 64, where k_pileup starts its walk of such a read instead of at its first
// operation; and the records the short-read form would get for the read, counted here where its CIGAR is hot.
namespace {
struct BytesChunk : WalkChunk {
    uint32_t n_long = 0;
    void fold(PushRecord &a) const { a.n_long += n_long; if (n_long) a.has_long = true; }
};
struct BytesForm {
    const cl_read_tile *t;
    uint32_t *rec_cnt, *ck_x, *ck_y;                               // (rec_cnt: this tile's entries; ck_x, ck_y: the contig's)
    uint32_t shift;                                                // tile op index -> contig op index (mod 2^32)
    uint32_t min_mapq;
    // (a tile of long-read shape -- 8 or more operations per read -- will not get the short-read form: its reads'
    // records are not counted here, that would be a second pass over every operation)
    bool count_recs;
    void blank(size_t i) const { rec_cnt[i] = 0u; }
    bool ref_length(BytesChunk &o, size_t i, int32_t p, const uint32_t *cig, uint32_t nops, unsigned long long &l) const
    {
        if (nops <= kLongOps) return false;
        o.n_long += 1;
        uint32_t yq = 0;                                               // query advance (M I S = X), modulo 2^32
        const uint32_t k0 = t->cigar_off[i] + shift;
        for (uint32_t q = 0; q < nops; ++q) {
            const uint32_t kc = k0 + q;
            if ((kc & 63u) == 0u) {
                const unsigned long long cx = (unsigned long long)(uint32_t)p + l;
                ck_x[kc >> 6] = cx > 0xFFFF0000ull ? 0xFFFF0000u : (uint32_t)cx;
                ck_y[kc >> 6] = yq;
            }
            const uint32_t cw = cig[q], len = cw >> 4, op = cw & 15u;
            const bool radv = ((0x18Du >> op) & 1u) != 0u, qadv = ((0x193u >> op) & 1u) != 0u;
            l += radv ? len : 0u;
            yq += qadv ? len : 0u;
            if (radv && len == 0u) o.err |= kErrCigar;
        }
        return true;
    }
    void read(BytesChunk &, size_t i, int32_t p, const uint32_t *cig, uint32_t nops, uint32_t end) const
    {
        if (!count_recs) return;
        const unsigned long long ql = t->qual_off[i + 1] - t->qual_off[i];
        // one M/=/X operation as long as the qualities (96 reads in 100 of aligner output): one record, no walk
        if (nops == 1u && end != (uint32_t)p && ql < 0x10000ull && ((0x181u >> (cig[0] & 15u)) & 1u) && (cig[0] >> 4) == ql) rec_cnt[i] = 1u;
        else rec_cnt[i] = gen_read_recs(p, end, t->mapq[i], min_mapq, cig, nops, 0ull, ql, [](uint32_t, const ReadRec &) {});
    }
};
} // namespace

static cl_status cl_push_reads_impl(cl_ctx *c, const cl_read_tile *t)
{
    if (!c || !t) return CL_ERR_INVALID;
    TileHead h;
    const cl_status hst = tile_header(c, "cl_push_reads", t->n_reads, t->pos, t->mapq, t->cigar_off, t->cigar, t->qual_off, h);
    if (hst != CL_OK || h.n == 0) return hst;
    const uint64_t n = h.n, q0 = h.q0, ncig = h.ncig, nq = h.nq;
    const uint32_t cig0 = h.cig0;
    Staging &hs = c->hs;
    if (nq && !t->qual) return fail(c, CL_ERR_INVALID, "null qual array");
    if (hs.cigar.size() + ncig > 0xFFFFFFF0ull) return fail(c, CL_ERR_RANGE, "more than 2^32 CIGAR operations in one contig");
    if (c->acc.q_dev + hs.qual.size() + nq >= (1ull << 38)) return fail(c, CL_ERR_RANGE, "more than 2^38 quality bytes in one contig");
    if (c->bits) return push_status(c, push_reads_bits(hs, c->acc, walk_opts(c), t, h));   // the pass-bit form: no quality byte goes to the device
    const uint32_t cbase = (uint32_t)hs.cigar.size();
    const uint64_t rbase = hs.pos.size();

    // ---- a large tile: its quality bytes go from the caller's buffer to the device through the pinned staging
    //      ring, and they start now (unless cl_contig_prefetch_qual already sent exactly these bytes): the copier
    //      threads fill pinned buffers and queue their transfers while this thread validates the tile and stages
    //      the small arrays.  All are joined before the call returns (the caller's buffer is free again then);
    //      nothing of the context changes if the tile turns out to be invalid. ----
    struct RingGuard { cl_ctx *c; bool active = false; ~RingGuard() { if (active) (void)ring_finish(c); } } ring{c};
    const bool direct = nq >= kDirectQual;
    if (direct) {
        const uint8_t *src = t->qual + q0;
        const bool prefetched = c->pf_active && c->pf_src == src && c->pf_n == nq && hs.qual.empty() && c->pf_off == c->acc.q_dev;
        if (prefetched) {
            c->pf_active = false; c->pf_src = nullptr; c->pf_n = 0;
            ring.active = true;                               // the transfer in flight is this tile's
        } else {
            drop_prefetch(c);
            cl_status fs = flush_staged_qual(c);
            if (fs != CL_OK) return fs;
            HIP_TRY(c, hipSetDevice(c->device));
            HIP_TRY(c, c->d_qual.grow_keep(c->acc.q_dev + nq + 2 * kQualPad, c->acc.q_dev ? kQualPad + c->acc.q_dev : 0, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));          // the (re)allocation above is done
            cl_status rs = ring_start(c, c->d_qual.p + kQualPad + c->acc.q_dev, nq,
                                      [src](uint64_t off, uint64_t len, uint8_t *out) { memcpy(out, src + off, len); });
            if (rs != CL_OK) return rs;
            ring.active = true;
        }
    } else if (c->pf_active) {
        drop_prefetch(c);
    }
    const unsigned long long qbase = c->acc.q_dev + hs.qual.size();
    StageTimer tmr;

    // ---- the one walk over every CIGAR of the tile (walk_tile, BytesForm).  Its entries [rbase, rbase + n) of the
    //      staging arrays, and the tile's checkpoints, are written beyond the arrays' sizes, as everything below is; the
    //      sizes follow when the tile is accepted, so a refused tile leaves nothing but unused capacity behind ----
    const size_t n_ck = ((cbase + ncig) >> 6) + 2;
    try {
        hs.rec_cnt.reserve(rbase + n); hs.end.reserve(rbase + n);
        hs.ck_x.reserve(n_ck); hs.ck_y.reserve(n_ck);
    } catch (const std::bad_alloc &) {
        return push_status(c, kNoMemory);
    }
    const bool count_recs = ncig < 8ull * n;
    const std::vector<BytesChunk> ch = walk_tile<BytesChunk>(t, h, hs.pos.empty() ? 0 : hs.pos.back(), c->contig_len, hs.end.data() + rbase,
        BytesForm{t, hs.rec_cnt.data() + rbase, hs.ck_x.data(), hs.ck_y.data(), cbase - cig0, c->opt.min_mapping_quality, count_recs});
    tmr.lap("push: validate + spans");
    if (const Offence f = first_offence(ch); f.st != CL_OK) return push_status(c, f);

    // ---- staging of the small arrays (offsets rebased onto the contig's): everything the tile can need is reserved,
    //      then written in parallel while the ring moves the qualities ----
    const size_t n_wide_new = wide_reads(ch);
    try {
        hs.pos.reserve(rbase + n); hs.mapq.reserve(rbase + n); hs.cigar.reserve(cbase + ncig);
        hs.cigar_off.reserve(rbase + n + 1); hs.qual_off.reserve(rbase + n + 1);   // (entry r + 1 closes read r)
        hs.wide_idx.reserve(hs.wide_idx.size() + n_wide_new); hs.wide_pos.reserve(hs.wide_pos.size() + n_wide_new);
        if (!direct) hs.qual.reserve(hs.qual.size() + nq);
    } catch (const std::bad_alloc &) {
        return push_status(c, kNoMemory);
    }
    copy_parallel(hs.pos.data() + rbase, t->pos, n);
    copy_parallel(hs.mapq.data() + rbase, t->mapq, n);
    copy_parallel(hs.cigar.data() + cbase, t->cigar + cig0, ncig);
    uint32_t *co = hs.cigar_off.data() + rbase;
    unsigned long long *qo = hs.qual_off.data() + rbase;
    dut::parallel_for(n, 262144, [&](size_t i) {
        co[i + 1] = cbase + (t->cigar_off[i + 1] - cig0);
        qo[i + 1] = qbase + (t->qual_off[i + 1] - q0);
    });
    tmr.lap("push: stage small arrays");
    if (ring.active) {
        ring.active = false;
        cl_status rs = ring_finish(c);                         // a failed copy: nothing was committed
        if (rs != CL_OK) return rs;
    }
    tmr.lap("push: wait for the qualities");
    // ---- the tile is accepted (nothing below can fail: the capacity is there) ----
    walk_fold(hs, c->acc, ch, rbase, t->pos);
    if (!count_recs) c->acc.rec_counted = false;
    hs.end.resize(rbase + n); hs.rec_cnt.resize(rbase + n); hs.ck_x.resize(n_ck); hs.ck_y.resize(n_ck);
    hs.pos.resize(rbase + n); hs.mapq.resize(rbase + n); hs.cigar.resize(cbase + ncig);
    hs.cigar_off.resize(rbase + n + 1); hs.qual_off.resize(rbase + n + 1);
    if (direct) c->acc.q_dev += nq;
    else hs.qual.insert(hs.qual.end(), t->qual + q0, t->qual + q0 + nq);
    return CL_OK;
}

cl_status cl_push_reads(cl_ctx *c, const cl_read_tile *t)
{
    return guarded(c, [&] { return cl_push_reads_impl(c, t); });
}

cl_status cl_push_reads_bits(cl_ctx *c, const cl_read_tile_bits *b)
{
    return guarded(c, [&]() -> cl_status {
        if (!c || !b) return CL_ERR_INVALID;
        // (inside a contig the wrong form is the first refusal; outside one, tile_header's)
        if (c->in_contig && !c->uploaded && !c->bits) return fail(c, CL_ERR_INVALID, "cl_push_reads_bits: this context runs the byte forms (DUT_QUAL_FORM=bytes), which need the quality bytes: use cl_push_reads");
        TileHead h;
        const cl_status hs = tile_header(c, "cl_push_reads_bits", b->n_reads, b->pos, b->mapq, b->cigar_off, b->cigar, b->qual_off, h);
        if (hs != CL_OK || h.n == 0) return hs;
        const uint64_t n = h.n, nq = h.nq;
        if (nq && (!b->pass_bits || !b->pass_sum)) return fail(c, CL_ERR_INVALID, "null pass_bits / pass_sum array");
        if (c->acc.q_dev + nq >= (1ull << 38)) return fail(c, CL_ERR_RANGE, "more than 2^38 quality values in one contig");
        cl_read_tile t;
        t.n_reads = n; t.pos = b->pos; t.mapq = b->mapq; t.cigar_off = b->cigar_off; t.cigar = b->cigar; t.qual_off = b->qual_off; t.qual = nullptr;
        static const uint64_t kNoBits[2] = {0, 0};
        static const uint32_t kNoSum[1] = {0};
        return push_status(c, push_reads_bits(c->hs, c->acc, walk_opts(c), &t, h, b->pass_bits ? b->pass_bits : kNoBits, b->pass_sum ? b->pass_sum : kNoSum));
    });
}

static cl_status cl_contig_upload_impl(cl_ctx *c)
{
    Range rg("cl_contig_upload");
    if (!c || !c->in_contig) return fail(c, CL_ERR_INVALID, "cl_contig_upload without cl_contig_begin");
    if (c->host_only) return fail(c, CL_ERR_DEVICE, "a host-only context (cl_debug_host_create) has no device to upload to");
    HIP_TRY(c, hipSetDevice(c->device));
    drop_prefetch(c);
    join_prealloc(c);
    c->n_reads = (uint32_t)c->hs.pos.size();
    c->n_cigar = c->bits ? c->acc.host_n_ops : c->hs.cigar.size();
    if (!c->bits) {
        cl_status fs = flush_staged_qual(c);
        if (fs != CL_OK) return fs;
    }
    c->n_qual = c->acc.q_dev;
    c->dev_sum_q = c->acc.host_sum_q; c->dev_sum_cov = c->bits ? c->acc.host_sum_cov : 0; c->dev_sum_mapq = c->bits ? c->acc.host_sum_mapq : 0;
    c->n_wide = (uint32_t)c->hs.wide_idx.size();
    const size_t n = c->n_reads;
    c->form = pick_form(c);
    const int form = c->form;
    StageTimer tmr0;
    // What the device needs of the per-read fields depends on the form of the pileup kernel the contig gets: the record
    // forms (pass bits: always; bytes: short reads) read records (built below) and nothing else per read; the run-table
    // form pos, mapq and end of the windows' candidates, and the table that the walk in size_for_extent() builds from the
    // staged CIGARs.  No form reads a CIGAR or an offset array: neither is uploaded.
    if (form == 2) HIP_TRY(c, c->d_end.reserve(n + 1));
    if (!c->bits) HIP_TRY(c, c->d_qual.grow_keep(c->n_qual + 2 * kQualPad, c->n_qual ? kQualPad + c->n_qual : 0, c->stream));
    HIP_TRY(c, c->d_wide_idx.reserve(c->n_wide + 1));
    tmr0.lap("upload: device buffers");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    tmr0.lap("upload: stream idle");
    StageTimer tmr;
    // everything goes through the pinned staging ring (pageable vectors -> pinned buffers -> HBM, the fills overlapping
    // the transfers)
    cl_status rs = CL_OK;
    if (form == 2) {
        HIP_TRY(c, c->d_pos.reserve(n + 1));
        HIP_TRY(c, c->d_mapq.reserve(n + 1));
        if ((rs = ring_copy(c, c->d_pos.p, c->hs.pos.data(), n * sizeof(int32_t))) != CL_OK) return rs;
        if ((rs = ring_copy(c, c->d_mapq.p, c->hs.mapq.data(), n)) != CL_OK) return rs;
        if ((rs = ring_copy(c, c->d_end.p, c->hs.end.data(), n * sizeof(uint32_t))) != CL_OK) return rs;
    }
    c->hs.rec_of.clear(); c->hs.wide_rec_of.clear(); c->n_rec = 0;
    if (form == 3) {
        // the heads (pileup_rows.hip.h): 8 bytes per read the pileup holds -- [pos, pos + span) and whether its mapq counts
        // as low (mod.rs:22-28) --, built straight into the pinned buffers; a span beyond kHeadSpanMax is cut into
        // several heads (h_rec_cnt, counted by cl_push_reads' walk).  4 bytes per head where every head fits them: no
        // wide read (every span <= kWideSpan: 15 bits hold it) and no span cut (span_n is the longest of those spans), so
        // that a read has at most one head and every window reads it as an ordinary candidate.
        if ((rs = build_rec_index(c)) != CL_OK) return rs;
        tmr.lap("upload: record index");
        const uint32_t n_rec = c->n_rec;
        c->heads4 = !c->heads8_only && c->n_wide == 0 && c->acc.span_n <= c->head_span && c->acc.span_n <= kWideSpan;
        const size_t head_bytes = c->heads4 ? sizeof(uint32_t) : sizeof(uint2);
        HIP_TRY(c, c->d_heads.reserve((((size_t)n_rec + 1) * head_bytes + sizeof(uint2) - 1) / sizeof(uint2)));
        const int32_t *hp = c->hs.pos.data(); const uint8_t *hm = c->hs.mapq.data(); const uint32_t *he = c->hs.end.data();
        const uint32_t *ro = c->hs.rec_of.data();
        const uint32_t max_low = c->opt.max_low_mapq, hs = c->head_span;
        auto send_heads = [&](auto head) {                       // head: a value of the head's type, uint32_t or uint2
            using Head = decltype(head);
            return ring_start(c, reinterpret_cast<uint8_t *>(c->d_heads.p), ((uint64_t)n_rec + 1) * sizeof(Head),
                              rec_range_fill<Head>(ro, n, n_rec, [=](size_t i, auto &&put) {
                const uint32_t low = (uint32_t)hm[i] <= max_low ? 0x80000000u : 0u, cnt = ro[i + 1] - ro[i];
                uint64_t x = (uint32_t)hp[i];
                const uint64_t e = he[i];
                if constexpr (sizeof(Head) == sizeof(uint32_t)) { if (cnt) put(0u, ((uint32_t)x & 0xFFFFu) | ((uint32_t)(e - x) << 16) | low); }
                else for (uint32_t k = 0; k < cnt; ++k, x += hs) put(k, make_uint2((uint32_t)x, (uint32_t)std::min<uint64_t>(hs, e - x) | low));
            }), rec_chunk_bytes());
        };
        rs = c->heads4 ? send_heads(uint32_t()) : send_heads(uint2());
        if (rs == CL_OK) rs = ring_finish(c); else (void)ring_finish(c);
        if (rs != CL_OK) return rs;
        tmr.lap("upload: heads built + sent");
    } else if (form != 2) {
        // the records (pileup_bytes.hip.h: ReadRec): the host's walk over the CIGARs, so that the device decodes none --
        // north_star's "CIGAR-expanded ref spans" on the host side of the boundary.  Counted first (the reads' record
        // ranges are what the windows' candidate ranges index), then built straight into the pinned buffers: a buffer
        // covers a range of record numbers, the reads it belongs to are found by binary search.  Pass-bit form: a head
        // record per read and nothing else (its M/=/X runs are in the rows).
        if ((rs = build_rec_index(c)) != CL_OK) return rs;
        tmr.lap("upload: record index");
        const uint32_t n_rec = c->n_rec;
        HIP_TRY(c, c->d_rec.reserve((size_t)n_rec + 1));
        const int32_t *hp = c->hs.pos.data(); const uint8_t *hm = c->hs.mapq.data(); const uint32_t *he = c->hs.end.data();
        const uint32_t *hc = c->hs.cigar_off.data(), *hcig = c->hs.cigar.data(); const unsigned long long *hq = c->hs.qual_off.data();
        const uint32_t *ro = c->hs.rec_of.data();
        const uint32_t min_mapq = c->opt.min_mapping_quality;
        // byte form: k_pileup loads 16-byte units around a record's run [qoff, qoff + len): within 15 bytes of its ends,
        // which the padding of the quality array covers as long as the run itself lies inside [0, n_qual] -- checked for
        // every record as it is built (CL_ERR_RANGE instead of a launch that would fault)
        std::atomic<bool> rec_oor{false};
        std::atomic<bool> *roor = &rec_oor;
        const unsigned long long nq_all = c->n_qual;
        const size_t inject_read = fault_injected("rec") ? n / 2 : (size_t)-1;
        rs = ring_start(c, reinterpret_cast<uint8_t *>(c->d_rec.p), ((uint64_t)n_rec + 1) * sizeof(ReadRec),
                        rec_range_fill<ReadRec>(ro, n, n_rec, [hp, hm, he, hc, hcig, hq, min_mapq, roor, nq_all, inject_read](size_t i, auto &&put) {
            const unsigned long long q0i = hq[i] + (i == inject_read ? 0x7FFFFFF0ull : 0ull);
            if (q0i + (hq[i + 1] - hq[i]) > nq_all) roor->store(true, std::memory_order_relaxed);   // (runs lie inside the read's bytes)
            gen_read_recs(hp[i], he[i], hm[i], min_mapq, hcig + hc[i], hc[i + 1] - hc[i], q0i, hq[i + 1] - hq[i], put);
        }), rec_chunk_bytes());
        if (rs == CL_OK) rs = ring_finish(c); else (void)ring_finish(c);
        if (rs != CL_OK) return rs;
        if (rec_oor.load()) return fail(c, CL_ERR_RANGE, "a read record addresses quality bytes outside the resident array");
        tmr.lap("upload: records built + sent");
    }
    std::vector<uint32_t> wide_rec;                      // record forms: the wide reads' records, read by read
    if (c->n_wide && form != 2) {
        c->hs.wide_rec_of.assign(c->n_wide + 1, 0u);
        for (uint32_t j = 0; j < c->n_wide; ++j) {
            const uint32_t i = c->hs.wide_idx[j];
            for (uint32_t r = c->hs.rec_of[i]; r < c->hs.rec_of[i + 1]; ++r) wide_rec.push_back(r);
            c->hs.wide_rec_of[j + 1] = (uint32_t)wide_rec.size();
        }
        HIP_TRY(c, c->d_wide_idx.reserve(wide_rec.size() + 1));
        if (!wide_rec.empty())
            HIP_TRY(c, hipMemcpyAsync(c->d_wide_idx.p, wide_rec.data(), wide_rec.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    } else if (c->n_wide) {
        HIP_TRY(c, hipMemcpyAsync(c->d_wide_idx.p, c->hs.wide_idx.data(), c->n_wide * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    if (!c->bits && c->d_qual.p) {
        HIP_TRY(c, hipMemsetAsync(c->d_qual.p, 0, kQualPad, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_qual.p + kQualPad + c->n_qual, 0, kQualPad, c->stream));
    }
    HIP_TRY(c, hipMemsetAsync(c->d_errflag.p, 0, 2 * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // a read overhanging the contig end makes the reference walk (and classify as REF_N, mod.rs:100-101) positions
    // up to its end: the extent is known from the spans computed at cl_push_reads
    tmr.lap("upload: small + sync");
    cl_status s = size_for_extent(c, (uint32_t)std::max<uint64_t>(c->contig_len, c->acc.host_max_end));
    if (s != CL_OK) return s;
    tmr.lap("upload: extent, ref, bounds");
    {   // the start values of every run's summary (the stream is idle: size_for_extent ended with a sync)
        const DevSummary s0 = summary_start_values(c);
        HIP_TRY(c, hipMemcpy(c->d_sum0.p, &s0, sizeof(DevSummary), hipMemcpyHostToDevice));
    }
    if (c->d_iv.cap == 0) HIP_TRY(c, c->d_iv.reserve(1u << 20));
    // The staged copy is no longer needed; its memory goes to the process's staging pool for the next contig, this
    // context's or another's (giving back and re-faulting a few hundred megabytes per contig was a fifth of a contig's
    // host time).
    give_staging(c->hs);
    tmr.lap("upload: done");
    c->uploaded = true; c->ran = false; c->collected = false;
    return CL_OK;
}

cl_status cl_contig_upload(cl_ctx *c)
{
    return guarded(c, [&] { return cl_contig_upload_impl(c); });
}

cl_status cl_debug_read_records(int32_t pos, const uint32_t *cigar, uint32_t n_ops, uint8_t mapq, uint8_t min_mapping_quality,
                                uint64_t qual_off, uint64_t qual_len, uint32_t *out, uint32_t cap,
                                uint32_t *n_records, uint32_t *phase)
{
    if ((n_ops && !cigar) || (cap && !out) || !n_records) return CL_ERR_INVALID;
    // the read's end as cl_push_reads' walk takes it: pos + bam_cigar2rlen, the read spanning nothing beyond the range
    unsigned long long l = 0;
    for (uint32_t q = 0; q < n_ops; ++q) if ((0x18Du >> (cigar[q] & 15u)) & 1u) l += cigar[q] >> 4;
    if (pos < 0) return CL_ERR_INVALID;
    const uint32_t end = l <= 0xFFFF0000ull - (uint64_t)pos ? (uint32_t)((uint64_t)pos + l) : (uint32_t)pos;
    uint32_t ph = 0;
    const uint32_t n = gen_read_recs(pos, end, mapq, min_mapping_quality, cigar, n_ops, qual_off, qual_len,
                                     [&](uint32_t k, const ReadRec &r) {
                                         if (k < cap) { out[4 * k] = (uint32_t)r.pos; out[4 * k + 1] = r.span; out[4 * k + 2] = r.qual_lo; out[4 * k + 3] = r.meta; }
                                     }, &ph);
    *n_records = n;
    if (phase) *phase = ph;
    return CL_OK;
}

cl_status cl_debug_qual_pack(const uint8_t *qual, uint64_t n, uint8_t min_base_quality, int level, uint64_t *words_out, uint64_t *sum_out)
{
    if (level >= 10 && level <= 12) {                            // the one-pass form cl_push_reads uses per read
        if ((n && !qual) || !words_out) return CL_ERR_INVALID;
        const uint64_t sm = dut::qual_pass_read(qual, n, min_base_quality, words_out, level - 10);
        if (sum_out) *sum_out = sm;
        return CL_OK;
    }
    if ((n && !qual) || level < 0 || level > 2) return CL_ERR_INVALID;
    if (words_out) {
        dut::qual_pass_words(qual, n >> 6, min_base_quality, words_out, level);
        if (n & 63ull) words_out[n >> 6] = dut::qual_pass_partial(qual + (n & ~63ull), (uint32_t)(n & 63ull), min_base_quality);
    }
    if (sum_out) *sum_out = dut::qual_pass_sum(qual, n, min_base_quality, level);
    return CL_OK;
}

cl_status cl_debug_ref_n_bits(const uint8_t *ref, uint64_t n_bases, uint64_t n_words, int level, uint64_t *words_out)
{
    if ((n_bases && !ref) || (n_words && !words_out) || level < 0 || level > 2) return CL_ERR_INVALID;
    dut::ref_n_words(ref, n_bases, n_words, words_out, level);
    return CL_OK;
}

cl_status cl_debug_gc_bits(const uint8_t *ref, uint64_t n_bases, uint64_t n_words, int level, uint64_t *gc_out, uint64_t *valid_out)
{
    if ((n_bases && !ref) || (n_words && (!gc_out || !valid_out)) || level < 0 || level > 2) return CL_ERR_INVALID;
    dut::gc_bit_words(ref, n_bases, n_words, gc_out, valid_out, 1, level);
    return CL_OK;
}

cl_status cl_debug_host_create(const cl_options *opt, cl_ctx **out)
{
    if (!opt || !out) return CL_ERR_INVALID;
    *out = nullptr;
    cl_ctx *c = new (std::nothrow) cl_ctx();
    if (!c) return CL_ERR_NOMEM;
    c->device = -1; c->opt = *opt; c->host_only = true; c->bits = true;
    c->rows_uniform = rows_uniform_env();
    *out = c;
    return CL_OK;
}

cl_status cl_debug_pass_rows(cl_ctx *c, uint32_t *n_groups, uint32_t n_win_cap, uint32_t *rows, uint64_t cap_words,
                             uint64_t *n_words, uint32_t *n_windows, uint64_t *summed_baseq)
{
    dut::RowScratch sc;
    std::vector<uint32_t> buf;
    uint64_t used = 0;
    const cl_status s = debug_rows_walk(c, "cl_debug_pass_rows", n_windows, [&](uint32_t w, uint32_t W, const dut::RowReads &H, std::vector<dut::RowCur> &act) {
        size_t cap = 16, cnt;
        const std::vector<dut::RowCur> start = act;
        for (;;) {
            buf.assign(cap * dut::kRowGroupWords, 0xDEADBEEFu);         // groups must be zeroed by the builder itself
            act = start;
            cnt = dut::rows_window<kT>(act, H, W, buf.data(), cap, sc);
            if (cnt != SIZE_MAX) break;
            cap *= 4;
        }
        if (w < n_win_cap && n_groups) n_groups[w] = (uint32_t)cnt;
        const uint64_t nw = (uint64_t)cnt * dut::kRowGroupWords;
        if (rows && used + nw <= cap_words) memcpy(rows + used, buf.data(), nw * sizeof(uint32_t));
        used += nw;
    });
    if (s != CL_OK) return s;
    if (summed_baseq) *summed_baseq = c->acc.host_sum_q;
    if (n_words) *n_words = used;
    return CL_OK;
}

cl_status cl_debug_pass_rows_segments(cl_ctx *c, uint32_t *heights, uint64_t *height_words, uint32_t n_win_cap, uint32_t *units,
                                      uint64_t cap_words, uint64_t *n_words, uint32_t *n_windows)
{
    dut::SegScratch sc;
    std::vector<uint32_t> buf;
    uint64_t used = 0;
    const cl_status s = debug_rows_walk(c, "cl_debug_pass_rows_segments", n_windows, [&](uint32_t w, uint32_t W, const dut::RowReads &H, std::vector<dut::RowCur> &act) {
        size_t cap = 16, cnt;
        const std::vector<dut::RowCur> start = act;
        for (;;) {
            buf.assign(cap * dut::kRowUnitWords, 0xDEADBEEFu);          // units must be written whole by the builder itself
            act = start;
            cnt = dut::rows_window_segments<kT>(act, H, W, buf.data(), cap, sc, c->rows_uniform);
            if (cnt != SIZE_MAX) break;
            cap *= 4;
        }
        if (w < n_win_cap && heights) memcpy(heights + (size_t)w * dut::kRowSegments, sc.h, sizeof(sc.h));
        if (w < n_win_cap && height_words) height_words[w] = sc.word;
        const uint64_t nw = (uint64_t)cnt * dut::kRowUnitWords;
        if (units && used + nw <= cap_words) memcpy(units + used, buf.data(), nw * sizeof(uint32_t));
        used += nw;
    });
    if (s != CL_OK) return s;
    if (n_words) *n_words = used;
    return CL_OK;
}

cl_status cl_contig_run(cl_ctx *c)
{
    Range rg("cl_contig_run");
    if (!c || !c->uploaded) return fail(c, CL_ERR_INVALID, "cl_contig_run before cl_contig_upload");
    HIP_TRY(c, hipSetDevice(c->device));
    c->collected = false;
    cl_status s = enqueue(c, false, nullptr, nullptr, nullptr);
    if (s == CL_OK) c->ran = true;
    return s;
}

cl_status cl_sync(cl_ctx *c)
{
    if (!c) return CL_ERR_INVALID;
    if (c->host_only) return fail(c, CL_ERR_DEVICE, "a host-only context has no device");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return harvest_events(c);
}

static cl_status check_summary(cl_ctx *c)
{
    if ((c->h_sum.err | c->bounds_err | c->acc.host_err) & kErrRange) return fail(c, CL_ERR_RANGE, "a read ends beyond the engine's 32-bit coordinate range");
    if ((c->h_sum.err | c->acc.host_err) & kErrCigar)
        return fail(c, CL_ERR_CIGAR, "malformed CIGAR: zero-length reference-consuming operation, or a single non-match "
                                     "operation on a read that spans reference positions (undefined in htslib's pileup)");
    return CL_OK;
}

cl_status cl_contig_collect(cl_ctx *c, cl_contig_summary *out, const cl_interval **intervals, size_t *n_intervals)
{
    return guarded(c, [&]() -> cl_status {
        Range rg("cl_contig_collect");
        if (!c || !c->ran) return fail(c, CL_ERR_INVALID, "cl_contig_collect before cl_contig_run");
        HIP_TRY(c, hipSetDevice(c->device));
        StageTimer tmr;
        // every `continue` below re-runs the contig for one distinct reason (32-bit counters: once; 16-bit fields in the
        // marked windows: the marks are sticky, at most twice; a larger extent: once per overhang level), so a handful of
        // rounds always suffices -- if they do not, the device state and h_sum disagree and nothing may be returned
        bool converged = false;
        for (int attempt = 0; attempt < 8 && !converged; ++attempt) {
            HIP_TRY(c, hipMemcpyAsync(&c->h_sum, c->d_summary.p, sizeof(DevSummary), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            cl_status s = harvest_events(c);
            if (s != CL_OK) return s;
            s = check_summary(c);
            if (s != CL_OK) return s;
            // a window touched by more reads than the 16-bit counters hold: redo with 32-bit counters
            if ((c->h_sum.err & kNeedDeep) && !c->deep) {
                c->deep = true;
                s = enqueue(c, false, nullptr, nullptr, nullptr);
                if (s != CL_OK) return s;
                continue;
            }
            // a position deeper than 255 in a window that used the 8-bit counter sets beyond their safe
            // candidate count: the kernel marked those windows, run again (they now use 16-bit fields)
            if ((c->h_sum.err & kNeedWide8) && !c->deep) {             // the marks are sticky: at most one more run raises it
                s = enqueue(c, false, nullptr, nullptr, nullptr);
                if (s != CL_OK) return s;
                continue;
            }
            // (a read that overhangs the contig end makes the reference walk, and classify as REF_N, positions up to its
            // end, mod.rs:100-101: the extent was sized for that at upload from the ends computed at cl_push_reads)
            if (c->h_sum.n_intervals > c->d_iv.cap) {
                HIP_TRY(c, c->d_iv.reserve(c->h_sum.n_intervals));
                s = launch_tail(c, true);
                if (s != CL_OK) return s;
                HIP_TRY(c, hipGetLastError());
            }
            converged = true;
        }
        if (!converged) return fail(c, CL_ERR_DEVICE, "cl_contig_collect: the re-run loop (counter width / extent) did not converge");
        tmr.lap("collect: kernels + summary");
        const size_t niv = c->h_sum.n_intervals;
        static_assert(sizeof(cl_interval) == sizeof(Interval), "interval layout");
        try { c->h_iv.resize(niv); } catch (const std::bad_alloc &) { return fail(c, CL_ERR_NOMEM, "interval buffer"); }
        if (niv) {
            HIP_TRY(c, hipMemcpyAsync(c->h_iv.data(), c->d_iv.p, niv * sizeof(Interval), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        tmr.lap("collect: intervals D2H");
        if (out) {
            static_assert(offsetof(DevSummary, max_end) == sizeof(cl_contig_summary), "summary layout");
            memcpy(out, &c->h_sum, sizeof(cl_contig_summary));
        }
        if (intervals) *intervals = c->h_iv.data();
        if (n_intervals) *n_intervals = niv;
        c->collected = true;
        return CL_OK;
    });
}

cl_status cl_contig_finish(cl_ctx *c, cl_contig_summary *out, const cl_interval **intervals, size_t *n_intervals)
{
    StageTimer tmr;
    cl_status s = cl_contig_upload(c);
    if (s != CL_OK) return s;
    tmr.lap("finish: upload");
    s = cl_contig_run(c);
    if (s != CL_OK) return s;
    tmr.lap("finish: run (launches)");
    s = cl_contig_collect(c, out, intervals, n_intervals);
    tmr.lap("finish: collect");
    return s;
}

cl_status cl_contig_abort(cl_ctx *c)
{
    if (!c) return CL_ERR_INVALID;
    if (!c->host_only) {
        (void)hipSetDevice(c->device);
        drop_prefetch(c);                                 // joins the copiers: nothing reads the caller's buffer any more
        join_prealloc(c);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
    }
    drop_staged(c);
    c->in_contig = false; c->uploaded = false; c->ran = false; c->collected = false;
    return CL_OK;
}

cl_status cl_device_summary(cl_ctx *c, void **dev_ptr, size_t *bytes)
{
    if (!c || !dev_ptr || !bytes) return CL_ERR_INVALID;
    *dev_ptr = c->d_summary.p;
    *bytes = sizeof(cl_contig_summary);
    return CL_OK;
}

cl_status cl_set_profiling(cl_ctx *c, int on)
{
    if (!c) return CL_ERR_INVALID;
    c->profiling = on != 0;
    return CL_OK;
}

cl_status cl_get_kernel_ms(cl_ctx *c, double ms[CL_K_COUNT], uint64_t *n_runs)
{
    if (!c) return CL_ERR_INVALID;
    cl_status s = harvest_events(c);
    if (s != CL_OK) return s;
    if (ms) for (int i = 0; i < CL_K_COUNT; ++i) ms[i] = c->ms[i];
    if (n_runs) *n_runs = c->n_runs;
    return CL_OK;
}

cl_status cl_reset_kernel_ms(cl_ctx *c)
{
    if (!c) return CL_ERR_INVALID;
    cl_status s = harvest_events(c);
    if (s != CL_OK) return s;
    for (int i = 0; i < CL_K_COUNT; ++i) c->ms[i] = 0.0;
    c->n_runs = 0;
    return CL_OK;
}

cl_status cl_contig_bytes(cl_ctx *c, uint64_t *input_bytes, uint64_t *output_bytes)
{
    if (!c || !c->uploaded) return fail(c, CL_ERR_INVALID, "no resident contig");
    // What one run of the resident form must read at least once, counted strictly: the array elements the form's kernel
    // addresses, nothing it does not (no CIGAR word: none is resident in any form), and what it must write: the intervals
    // (12 bytes each; the per-position counters and states never reach HBM).
    //   every form   reference bytes (extent; pass bits: one bit per position) + one 32-byte window record per window
    //   pass bits    the rows (1 KB per group of 4 rows) + a head per read with a span, 8 bytes or 4 + the wide list
    //   bytes, 0     the quality bytes + the 16-byte records (heads and pieces) + the wide list
    //   bytes, 2     the quality bytes + 8 bytes per piece of the run table + pos 4, end 4, mapq 1 per read + the wide list
    uint64_t in = (c->form == 3 ? ((uint64_t)c->extent + 7) / 8 : (uint64_t)c->extent) + (uint64_t)c->n_win * sizeof(WinMeta);
    if (c->form == 3) in += c->n_row_groups * (uint64_t)(dut::kRowUnitWords * sizeof(uint32_t)) + (uint64_t)c->n_rec * (c->heads4 ? sizeof(uint32_t) : sizeof(uint2)) + (uint64_t)c->n_wide * 4;
    else if (c->form == 0) in += c->n_qual + (uint64_t)c->n_rec * sizeof(ReadRec) + (uint64_t)c->n_wide * 4;
    else in += c->n_qual + c->n_runtab * 8 + (uint64_t)c->n_reads * 9 + (uint64_t)c->n_wide * 4;
    if (input_bytes) *input_bytes = in;
    if (output_bytes) *output_bytes = 12ull * c->h_sum.n_intervals;
    return CL_OK;
}

cl_status cl_contig_layout(cl_ctx *c, cl_layout_info *out)
{
    if (!c || !out || !c->uploaded) return fail(c, CL_ERR_INVALID, "no resident contig");
    memset(out, 0, sizeof(*out));
    out->form = c->form;
    out->n_reads = c->n_reads; out->n_records = c->n_rec; out->n_windows = c->n_win;
    out->n_qual = c->n_qual; out->n_cigar = c->n_cigar;
    out->row_groups = c->n_row_groups; out->max_groups = c->max_groups;
    out->run_table_entries = c->n_runtab;
    out->counter_planes = c->form == 3 ? c->counter_planes() : 0u;
    // HBM this context holds: the capacity of the device buffers of each_buffer, as cl_destroy walks them
    uint64_t b = 0;
    c->each_buffer([&](auto &buf) { b += buf.cap * sizeof(*buf.p); });
    out->device_bytes = b;
    // what cl_contig_upload sent over the link for this contig (every transfer goes through the pinned staging ring)
    const uint64_t padded = (uint64_t)c->n_win * kT + 16;
    uint64_t h = (c->form == 3 ? ((uint64_t)c->n_win * kT) / 8 : padded) + (uint64_t)c->n_win * sizeof(WinMeta) + (uint64_t)c->n_wide * 4;
    if (c->form == 3) h += c->n_row_groups * (uint64_t)(dut::kRowUnitWords * sizeof(uint32_t)) + ((uint64_t)c->n_rec + 1) * (c->heads4 ? sizeof(uint32_t) : sizeof(uint2));
    else if (c->form == 0) h += c->n_qual + ((uint64_t)c->n_rec + 1) * sizeof(ReadRec);
    else h += c->n_qual + c->n_runtab * 8 + (uint64_t)c->n_reads * 9;
    out->upload_h2d_bytes = h;
    if (c->n_win) { out->tail_wpc = tail_wpc(c->n_win, c->tail_max_chunks); out->tail_chunks = (c->n_win + out->tail_wpc - 1u) / out->tail_wpc; }
    return CL_OK;
}

cl_status cl_debug_depths(cl_ctx *c, uint32_t *raw, uint32_t *qc, uint32_t *low, uint8_t *state, uint64_t cap)
{
    return guarded(c, [&]() -> cl_status {
        if (!c || !c->ran) return fail(c, CL_ERR_INVALID, "cl_debug_depths needs a collected contig");
        HIP_TRY(c, hipSetDevice(c->device));
        if (cap < c->extent) return fail(c, CL_ERR_INVALID, "cap < extent");
        const size_t padded = (size_t)c->n_win * kT;
        HIP_TRY(c, c->d_dbg.reserve(3 * padded + 1));
        cl_status s = enqueue(c, true, c->d_dbg.p, c->d_dbg.p + padded, c->d_dbg.p + 2 * padded);
        if (s != CL_OK) return s;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const size_t nb = (size_t)c->extent * sizeof(uint32_t);
        if (raw && nb) HIP_TRY(c, hipMemcpy(raw, c->d_dbg.p, nb, hipMemcpyDeviceToHost));
        if (qc && nb) HIP_TRY(c, hipMemcpy(qc, c->d_dbg.p + padded, nb, hipMemcpyDeviceToHost));
        if (low && nb) HIP_TRY(c, hipMemcpy(low, c->d_dbg.p + 2 * padded, nb, hipMemcpyDeviceToHost));
        if (state && c->extent) HIP_TRY(c, hipMemcpy(state, c->d_state.p, c->extent, hipMemcpyDeviceToHost));
        return CL_OK;
    });
}

// What cl_contig_depth_profile, cl_contig_depth_runs and cl_contig_targets (`who`) refuse alike, in the order they have
// always refused it: the context's kind, the call's own arguments, the contig's state (`collected`: the call reads the
// intervals too); behind it the device is current.  The arguments' checks look at nothing of the context, so the caller
// makes them first and hands over what they gave (`args`): their place is decided here, a later fail() replaces their message.
static cl_status depth_call_ready(cl_ctx *c, const char *who, bool collected, cl_status args)
{
    if (c->host_only) return fail(c, CL_ERR_DEVICE, "a host-only context has no device");
    if (!c->bits) return fail(c, CL_ERR_INVALID, std::string(who) + " serves the pass-bit form only (the context runs DUT_QUAL_FORM=bytes)");
    if (args != CL_OK) return args;
    if (!c->uploaded || !c->ran || (collected && !c->collected) || c->form != 3)
        return fail(c, CL_ERR_INVALID, std::string(who) + (collected ? " needs a contig that has been collected since its last run (cl_contig_collect or cl_contig_finish)"
                                                                      : " needs a contig that has been run"));
    if (c->bounds_err & kErrRange) return fail(c, CL_ERR_RANGE, "a read ends beyond the engine's 32-bit coordinate range");
    HIP_TRY(c, hipSetDevice(c->device));
    return CL_OK;
}

#pragma clang diagnostic push                              // (argument records in member order, as rows_args)
#pragma clang diagnostic error "-Wmissing-field-initializers"

// The depth distribution of the resident contig (include/callable_loci.h): one extra launch of k_depth_profile over the
// residents of the last run, a few KB back.  Nothing of a run is touched: summary, intervals and window partials stay.
cl_status cl_contig_depth_profile_ms(cl_ctx *c, double *kernel_ms)
{
    if (!c || !kernel_ms) return CL_ERR_INVALID;
    *kernel_ms = c->t_prof.ms;
    return CL_OK;
}

cl_status cl_contig_depth_profile(cl_ctx *c, uint32_t n_bins, uint32_t window, cl_depth_profile *out)
{
    return guarded(c, [&]() -> cl_status {
        if (!c) return CL_ERR_INVALID;
        if (!out) return fail(c, CL_ERR_INVALID, "cl_contig_depth_profile: null result");
        memset(out, 0, sizeof(*out));
        const cl_status ready = depth_call_ready(c, "cl_contig_depth_profile", false, [&]() -> cl_status {
            if (n_bins < CL_DEPTH_MIN_BINS || n_bins > CL_DEPTH_MAX_BINS) return fail(c, CL_ERR_INVALID, "cl_contig_depth_profile: n_bins outside [2, 4096]");
            if (window != 0 && window < CL_DEPTH_MIN_WINDOW) return fail(c, CL_ERR_INVALID, "cl_contig_depth_profile: a window of 1 to 15 positions (0 = no window table, else at least 16)");
            return CL_OK;
        }());
        if (ready != CL_OK) return ready;
        const uint64_t n_windows = window ? ((uint64_t)c->extent + window - 1) / window : 0;
        const size_t n_words = 2 + 2 * (size_t)n_bins + 2 * (size_t)n_windows;
        HIP_TRY(c, c->d_prof.reserve(n_words));
        c->h_prof.assign(n_words, 0ull);
        HIP_TRY(c, hipMemsetAsync(c->d_prof.p, 0, n_words * sizeof(unsigned long long), c->stream));
        if (c->n_win) {
            const DepthArgs a{depth_residents(c), n_bins, window, c->d_prof.p + 2, c->d_prof.p + 2 + 2 * (size_t)n_bins, n_windows, c->d_prof.p};
            const size_t lds = 2u * (size_t)n_bins * sizeof(uint32_t);
            // workgroups that stay: a histogram is flushed once per workgroup
            const uint32_t grid = std::min<uint32_t>(c->n_win, 2048u);
            if (c->profiling) HIP_TRY(c, c->t_prof.start(c->stream));
            hipLaunchKernelGGL(depth_kernel(c, kDepthProfileKernels), dim3(grid), dim3(kDepthBlock), lds, c->stream, a);
            HIP_TRY(c, hipGetLastError());
            if (c->profiling) HIP_TRY(c, c->t_prof.stop(c->stream));
            HIP_TRY(c, hipMemcpyAsync(c->h_prof.data(), c->d_prof.p, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->t_prof.ms = 0.0;
        if (c->profiling && c->n_win) HIP_TRY(c, c->t_prof.read());
        // (no window of the engine: every position of [0, extent) -- there is none -- is in bin 0)
        const uint64_t *h = reinterpret_cast<const uint64_t *>(c->h_prof.data());
        out->n_bins = n_bins; out->window = window; out->n_windows = n_windows; out->extent = c->extent;
        out->sum_raw = h[0]; out->sum_qc = h[1];
        out->hist_raw = h + 2; out->hist_qc = h + 2 + n_bins;
        out->win_raw = window ? h + 2 + 2 * (size_t)n_bins : nullptr;
        out->win_qc = window ? h + 2 + 2 * (size_t)n_bins + n_windows : nullptr;
        return CL_OK;
    });
}

// Both depths of the resident contig by the GC content around each position (include/callable_loci.h): the caller's
// reference bytes become the two bit planes of gc_bits.h on their way through the staging ring, one launch of k_gc_bias
// over them and the residents of the last run, 3.2 KB back.  Nothing of a run is touched: summary, intervals and
// window partials stay.  The planes are packed and sent by every call; nothing is kept across calls.
cl_status cl_contig_gc_bias_ms(cl_ctx *c, double *kernel_ms, double *upload_ms)
{
    if (!c || !kernel_ms) return CL_ERR_INVALID;
    *kernel_ms = c->t_gc.ms;
    if (upload_ms) *upload_ms = c->gc_upload_ms;
    return CL_OK;
}

cl_status cl_contig_gc_bias(cl_ctx *c, const uint8_t *ref, uint64_t ref_len, uint32_t window, uint32_t max_invalid, cl_gc_bias *out)
{
    static_assert(CL_GC_BINS == kGcBins && CL_GC_MAX_WINDOW == 2 * kGcPad, "the kernel's bins and halo");
    return guarded(c, [&]() -> cl_status {
        if (!c) return CL_ERR_INVALID;
        if (!out) return fail(c, CL_ERR_INVALID, "cl_contig_gc_bias: null result");
        memset(out, 0, sizeof(*out));
        const cl_status ready = depth_call_ready(c, "cl_contig_gc_bias", false, [&]() -> cl_status {
            if (!ref && ref_len) return fail(c, CL_ERR_INVALID, "cl_contig_gc_bias: null reference with a length");
            if (window < 1 || window > CL_GC_MAX_WINDOW) return fail(c, CL_ERR_INVALID, "cl_contig_gc_bias: window outside [1, 1024]");
            if (max_invalid >= window) return fail(c, CL_ERR_INVALID, "cl_contig_gc_bias: max_invalid is not below the window");
            return CL_OK;
        }());
        if (ready != CL_OK) return ready;
        c->t_gc.ms = 0.0; c->gc_upload_ms = 0.0;
        out->window = window; out->max_invalid = max_invalid; out->extent = c->extent;
        if (c->n_win == 0) { HIP_TRY(c, hipStreamSynchronize(c->stream)); return CL_OK; }   // (no position: nothing is counted or skipped)
        // ---- the planes: pair k is {gc, valid} of the positions [64 k - kGcPad, 64 k - kGcPad + 64); the pairs in front
        // of position 0 and every base at or beyond ref_len are invalid; no base at or beyond the padded extent is read ----
        const uint64_t padded = (uint64_t)c->n_win * kT;
        const uint64_t n_pairs = (padded + 2 * kGcPad) / 64, front = kGcPad / 64;
        const uint64_t nref = std::min<uint64_t>(ref_len, padded);
        HIP_TRY(c, c->d_gc_bits.reserve(n_pairs));
        HIP_TRY(c, c->d_gc_out.reserve(kGcOutWords));
        drop_prefetch(c);                                  // (an unclaimed prefetch of this context holds the ring)
        const double t0 = StageTimer::now();
        cl_status rs = ring_start(c, reinterpret_cast<uint8_t *>(c->d_gc_bits.p), n_pairs * 16, [ref, nref, front](uint64_t off, uint64_t len, uint8_t *dst) {
            // (a buffer of the ring is a whole number of pairs: 4 MB, and the transfer is n_pairs * 16 bytes)
            uint64_t k = off / 16, n = len / 16;
            uint64_t *w = reinterpret_cast<uint64_t *>(dst);
            for (; n && k < front; ++k, --n, w += 2) w[0] = w[1] = 0ull;
            if (!n) return;
            const uint64_t p = (k - front) * 64;
            dut::gc_bit_words(p < nref ? ref + p : nullptr, p < nref ? nref - p : 0, n, w, w + 1, 2, dut::gc_bits_level());
        });
        if (rs == CL_OK) rs = ring_finish(c); else (void)ring_finish(c);
        if (rs != CL_OK) return rs;
        c->gc_upload_ms = (StageTimer::now() - t0) * 1e3;
        HIP_TRY(c, hipMemsetAsync(c->d_gc_out.p, 0, kGcOutWords * sizeof(unsigned long long), c->stream));
        const GcArgs a{depth_residents(c), c->d_gc_bits.p, window, max_invalid, c->d_gc_out.p};
        // workgroups that stay: the bins are flushed once per workgroup (gc_bias.hip.h has what their widths rest on)
        const uint32_t grid = std::min<uint32_t>(c->n_win, 2048u);
        if (c->profiling) HIP_TRY(c, c->t_gc.start(c->stream));
        hipLaunchKernelGGL(depth_kernel(c, kGcBiasKernels), dim3(grid), dim3(kDepthBlock), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        if (c->profiling) HIP_TRY(c, c->t_gc.stop(c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->h_gc_out, c->d_gc_out.p, kGcOutWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (c->profiling) HIP_TRY(c, c->t_gc.read());
        const unsigned long long *h = c->h_gc_out;
        out->n_skipped = h[kGcBins];
        for (int b = 0; b < kGcBins; ++b) {
            out->positions[b] = h[b]; out->zero_raw[b] = h[kGcBins + 1 + b];
            out->sum_raw[b] = h[2 * kGcBins + 1 + b]; out->sum_qc[b] = h[3 * kGcBins + 1 + b];
        }
        return CL_OK;
    });
}

// The per-position depth of the resident contig as runs (include/callable_loci.h): k_depth_runs counts the run starts
// per window, k_depth_runs_scan turns the counts into offsets, k_depth_runs again stores the runs at them
// (depth_runs.hip.h).  The output buffers are sized from the scan's total, between the two passes.  Nothing of a run is
// touched: summary, intervals and window partials stay.
cl_status cl_contig_depth_runs_ms(cl_ctx *c, double *kernel_ms)
{
    if (!c || !kernel_ms) return CL_ERR_INVALID;
    *kernel_ms = c->dr_ms;
    return CL_OK;
}

cl_status cl_contig_depth_runs(cl_ctx *c, uint32_t kind, const uint32_t *edges, uint32_t n_edges, cl_depth_runs *out)
{
    return guarded(c, [&]() -> cl_status {
        if (!c) return CL_ERR_INVALID;
        if (!out) return fail(c, CL_ERR_INVALID, "cl_contig_depth_runs: null result");
        memset(out, 0, sizeof(*out));
        const cl_status ready = depth_call_ready(c, "cl_contig_depth_runs", false, [&]() -> cl_status {
            if (kind != CL_DEPTH_RAW && kind != CL_DEPTH_QC) return fail(c, CL_ERR_INVALID, "cl_contig_depth_runs: unknown depth kind (CL_DEPTH_RAW or CL_DEPTH_QC)");
            if (n_edges > CL_RUNS_MAX_EDGES) return fail(c, CL_ERR_INVALID, "cl_contig_depth_runs: more than 64 edges");
            if (n_edges && !edges) return fail(c, CL_ERR_INVALID, "cl_contig_depth_runs: null edges");
            if (n_edges && edges[0] == 0u) return fail(c, CL_ERR_INVALID, "cl_contig_depth_runs: the first edge is 0 (the first band starts at depth 0 by itself)");
            for (uint32_t i = 1; i < n_edges; ++i)
                if (edges[i] <= edges[i - 1]) return fail(c, CL_ERR_INVALID, "cl_contig_depth_runs: the edges are not strictly ascending");
            return CL_OK;
        }());
        if (ready != CL_OK) return ready;
        c->dr_ms = 0.0;
        unsigned long long total = 0ull;
        uint32_t err = 0u;
        if (c->n_win && c->extent) {
            const size_t nw = c->n_win;
            HIP_TRY(c, c->d_dr_win.reserve(3 * nw + 1));
            HIP_TRY(c, c->d_dr_off.reserve(nw + 1));
            // (the count pass writes nothing through start and value; the edges follow)
            RunsArgs a{depth_residents(c), n_edges, 0u, c->d_dr_win.p, c->d_dr_win.p + nw, c->d_dr_win.p + 2 * nw, c->d_dr_off.p,
                       nullptr, nullptr, 0ull, c->d_dr_win.p + 3 * nw, {}};
            for (uint32_t i = 0; i < n_edges; ++i) a.edges[i] = edges[i];
            const uint32_t grid = std::min<uint32_t>(c->n_win, 65536u);
            const DepthKernel<RunsArgs> kernel = depth_kernel(c, kind == CL_DEPTH_RAW ? kDepthRunsRawKernels : kDepthRunsQcKernels);
            auto launch = [&]() { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kDepthBlock), 0, c->stream, a); };
            // ---- count, scan: how many runs there are ----
            HIP_TRY(c, hipMemsetAsync(a.err, 0, sizeof(uint32_t), c->stream));
            if (c->profiling) HIP_TRY(c, c->t_dr_count.start(c->stream));
            launch();
            HIP_TRY(c, hipGetLastError());
            hipLaunchKernelGGL(k_depth_runs_scan, dim3(1), dim3(kRunsScanBlock), 0, c->stream, a.cnt, a.first, a.last, c->n_win, c->d_dr_off.p, c->d_dr_off.p + nw);
            HIP_TRY(c, hipGetLastError());
            if (c->profiling) HIP_TRY(c, c->t_dr_count.stop(c->stream));
            HIP_TRY(c, hipMemcpyAsync(&total, c->d_dr_off.p + nw, sizeof(total), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (total == 0ull || total > (unsigned long long)c->extent) return fail(c, CL_ERR_INTERNAL, "cl_contig_depth_runs: the count pass gave an impossible number of runs");
            // ---- write: into buffers of exactly that many slots ----
            HIP_TRY(c, c->d_dr_out.reserve(2 * (size_t)total));
            HIP_TRY(c, c->h_dr_out.reserve(2 * (size_t)total));
            a.write = 1u; a.start = c->d_dr_out.p; a.value = c->d_dr_out.p + total; a.cap = total;
            if (c->profiling) HIP_TRY(c, c->t_dr_write.start(c->stream));
            launch();
            HIP_TRY(c, hipGetLastError());
            if (c->profiling) HIP_TRY(c, c->t_dr_write.stop(c->stream));
            HIP_TRY(c, hipMemcpyAsync(c->h_dr_out.p, c->d_dr_out.p, 2 * (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(&err, a.err, sizeof(err), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (c->profiling) {
                HIP_TRY(c, c->t_dr_count.read());
                HIP_TRY(c, c->t_dr_write.read());
                c->dr_ms = c->t_dr_count.ms + c->t_dr_write.ms;
            }
            if (err) return fail(c, CL_ERR_INTERNAL, "cl_contig_depth_runs: the write pass met a slot outside the counted runs");
        } else {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        out->kind = kind; out->n_edges = n_edges; out->extent = c->extent; out->n_runs = total;
        out->start = total ? c->h_dr_out.p : nullptr;
        out->value = total ? c->h_dr_out.p + total : nullptr;
        return CL_OK;
    });
}

// Depth and state summaries of the resident contig over a list of targets (include/callable_loci.h): the host sorts the
// distinct query points that lie inside a window, k_target_depth takes the windows' totals and the prefixes at the points,
// k_target_scan the offsets, k_target_finish the records (depth_targets.hip.h).  Nothing of a run is touched: summary,
// intervals and window partials stay.
cl_status cl_contig_targets_ms(cl_ctx *c, double *kernel_ms, double launch_ms[3])
{
    if (!c || !kernel_ms) return CL_ERR_INVALID;
    *kernel_ms = c->tg_ms[0] + c->tg_ms[1] + c->tg_ms[2];
    if (launch_ms) for (int i = 0; i < 3; ++i) launch_ms[i] = c->tg_ms[i];
    return CL_OK;
}

cl_status cl_contig_targets(cl_ctx *c, const uint32_t *starts, const uint32_t *ends, size_t n_targets,
                            const uint32_t *thresholds, uint32_t n_thresholds, const cl_target_stats **out)
{
    return guarded(c, [&]() -> cl_status {
        if (!c) return CL_ERR_INVALID;
        if (!out) return fail(c, CL_ERR_INVALID, "cl_contig_targets: null result");
        *out = nullptr;
        const cl_status ready = depth_call_ready(c, "cl_contig_targets", true, [&]() -> cl_status {
            if (n_targets > CL_TARGETS_MAX) return fail(c, CL_ERR_INVALID, "cl_contig_targets: more than 2^24 targets");
            if (n_targets && (!starts || !ends)) return fail(c, CL_ERR_INVALID, "cl_contig_targets: null starts or ends");
            if (n_thresholds > CL_TARGET_MAX_THRESHOLDS) return fail(c, CL_ERR_INVALID, "cl_contig_targets: more than 8 thresholds");
            if (n_thresholds && !thresholds) return fail(c, CL_ERR_INVALID, "cl_contig_targets: null thresholds");
            if (n_thresholds && thresholds[0] == 0u) return fail(c, CL_ERR_INVALID, "cl_contig_targets: the first threshold is 0 (every position has a depth of at least 0)");
            for (uint32_t i = 1; i < n_thresholds; ++i)
                if (thresholds[i] <= thresholds[i - 1]) return fail(c, CL_ERR_INVALID, "cl_contig_targets: the thresholds are not strictly ascending");
            for (size_t i = 0; i < n_targets; ++i)
                if (starts[i] > ends[i]) return fail(c, CL_ERR_INVALID, "cl_contig_targets: target " + std::to_string(i) + " has start > end");
            return CL_OK;
        }());
        if (ready != CL_OK) return ready;
        for (double &m : c->tg_ms) m = 0.0;
        if (n_targets == 0) { HIP_TRY(c, hipStreamSynchronize(c->stream)); return CL_OK; }
        const size_t n = n_targets, nw = c->n_win;
        const uint32_t K = n_thresholds, V = 2u + 2u * K, extent = c->extent;
        try { c->h_tg_out.assign(n, cl_target_stats{}); } catch (const std::bad_alloc &) { return fail(c, CL_ERR_NOMEM, "cl_contig_targets: the records"); }
        static_assert(sizeof(cl_target_stats) == kTargetWords * sizeof(uint32_t), "record layout");
        const size_t niv = c->h_sum.n_intervals;
        // ---- the query points inside a window, ascending and distinct; per window its range of them; per target its two slots ----
        std::vector<uint32_t> &h = c->h_tg_in;
        std::vector<uint32_t> pts;
        size_t n_live = 0;
        try {
            pts.reserve(2 * n);
            for (size_t i = 0; i < n; ++i) {
                const uint32_t e = std::min(ends[i], extent), s = std::min(starts[i], e);
                if (s == e) continue;
                ++n_live;
                if (s % kT) pts.push_back(s);
                if (e % kT) pts.push_back(e);
            }
            std::sort(pts.begin(), pts.end());
            pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
            // layout of the upload: pt[n_pt], pt_first[nw + 1], tg[n][4]
            h.assign(pts.size() + nw + 1 + 4 * n, 0u);
        } catch (const std::bad_alloc &) { return fail(c, CL_ERR_NOMEM, "cl_contig_targets: the query points"); }
        const size_t n_pt = pts.size();
        if (n_pt) memcpy(h.data(), pts.data(), n_pt * sizeof(uint32_t));
        uint32_t *pt_first = h.data() + n_pt, *tg = pt_first + nw + 1;
        {
            size_t j = 0;
            for (size_t w = 0; w <= nw; ++w) {             // (every point is below extent <= nw * kT, or extent itself inside the last window)
                while (j < n_pt && pts[j] < (uint64_t)w * kT) ++j;
                pt_first[w] = (uint32_t)j;
            }
            pt_first[nw] = (uint32_t)n_pt;
        }
        auto slot_of = [&](uint32_t q) -> uint32_t {
            if (q % kT == 0) return kTargetNoSlot;
            return (uint32_t)(std::lower_bound(pts.begin(), pts.end(), q) - pts.begin());
        };
        for (size_t i = 0; i < n; ++i) {
            const uint32_t e = std::min(ends[i], extent), s = std::min(starts[i], e);
            tg[4 * i] = s; tg[4 * i + 1] = e;
            tg[4 * i + 2] = s == e ? kTargetNoSlot : slot_of(s);   // (an empty target asks nothing)
            tg[4 * i + 3] = s == e ? kTargetNoSlot : slot_of(e);
        }
        uint32_t err = 0u;
        if (n_live == 0 || nw == 0) {
            // (nothing to measure: every record is its clipped ends and zeros)
            for (size_t i = 0; i < n; ++i) { c->h_tg_out[i].start = tg[4 * i]; c->h_tg_out[i].end = tg[4 * i + 1]; }
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            *out = c->h_tg_out.data();
            return CL_OK;
        }
        // (none cannot cover the positions; the finish kernel indexes the intervals in 32 bits, 512 ahead)
        if (niv == 0 || niv > 0x7FFFFFFFu || niv > c->d_iv.cap) return fail(c, CL_ERR_INTERNAL, "cl_contig_targets: the collected contig has no interval, or more than the device holds");
        HIP_TRY(c, c->d_tg_in.reserve(h.size()));
        HIP_TRY(c, c->d_tg_win.reserve((size_t)(kTargetTotSlots / 2) * nw));
        HIP_TRY(c, c->d_tg_off.reserve((size_t)V * (nw + 1)));
        HIP_TRY(c, c->d_tg_pre.reserve((size_t)(kTargetPreWords / 4) * std::max<size_t>(n_pt, 1)));
        HIP_TRY(c, c->d_tg_out.reserve((size_t)kTargetWords * n + 1));
        uint32_t *d_err = c->d_tg_out.p + (size_t)kTargetWords * n;
        HIP_TRY(c, hipMemcpyAsync(c->d_tg_in.p, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_tg_out.p, 0, ((size_t)kTargetWords * n + 1) * sizeof(uint32_t), c->stream));
        // (pt_first follows the points; the thresholds follow)
        TargetArgs a{depth_residents(c), (uint32_t)n_pt, 0u, c->d_tg_in.p, c->d_tg_win.p, c->d_tg_pre.p, d_err, {}};
        for (uint32_t k = 0; k < CL_TARGET_MAX_THRESHOLDS; ++k) a.thr[k] = k < K ? thresholds[k] : 0xFFFFFFFFu;
        // workgroups that stay, as k_depth_profile's: a window is a few microseconds of work
        const uint32_t grid = std::min<uint32_t>(c->n_win, 2048u);
        if (c->profiling) HIP_TRY(c, c->t_tg[0].start(c->stream));
        hipLaunchKernelGGL(depth_kernel(c, kTargetDepthKernels), dim3(grid), dim3(kDepthBlock), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        if (c->profiling) { HIP_TRY(c, c->t_tg[0].stop(c->stream)); HIP_TRY(c, c->t_tg[1].start(c->stream)); }
        unsigned long long *d_off = c->d_tg_off.p;
        hipLaunchKernelGGL(k_target_scan, dim3(V), dim3(kTargetScanBlock), 0, c->stream, reinterpret_cast<const unsigned long long *>(c->d_tg_win.p), c->n_win, K, d_off);
        HIP_TRY(c, hipGetLastError());
        if (c->profiling) { HIP_TRY(c, c->t_tg[1].stop(c->stream)); HIP_TRY(c, c->t_tg[2].start(c->stream)); }
        TargetFinishArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.tg = c->d_tg_in.p + n_pt + nw + 1; fa.n = (uint32_t)n; fa.n_pt = (uint32_t)n_pt; fa.n_thr = K; fa.n_win = c->n_win;
        fa.off = d_off; fa.pre = reinterpret_cast<const uint32_t *>(c->d_tg_pre.p); fa.iv = c->d_iv.p; fa.n_iv = (uint32_t)std::min<size_t>(niv, c->d_iv.cap); fa.extent = extent;
        fa.out = c->d_tg_out.p; fa.err = d_err;
        const uint32_t per = (uint32_t)(kTargetFinishBlock / 64);
        hipLaunchKernelGGL(k_target_finish, dim3((uint32_t)((n + per - 1) / per)), dim3(kTargetFinishBlock), 0, c->stream, fa);
        HIP_TRY(c, hipGetLastError());
        if (c->profiling) HIP_TRY(c, c->t_tg[2].stop(c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->h_tg_out.data(), c->d_tg_out.p, n * sizeof(cl_target_stats), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (c->profiling)
            for (int i = 0; i < 3; ++i) { HIP_TRY(c, c->t_tg[i].read()); c->tg_ms[i] = c->t_tg[i].ms; }
        if (err) return fail(c, CL_ERR_INTERNAL, "cl_contig_targets: a device-side check of the uploaded points, slots or intervals failed");
        *out = c->h_tg_out.data();
        return CL_OK;
    });
}

// Minimum, quartiles and maximum of both depths of the resident contig over a list of targets (include/callable_loci.h):
// the host cuts the targets at the windows into pieces (target_pieces.h); k_target_order takes the extremes, then, once
// the host has read the largest raw depth of any target, one round per bit of it; k_target_order_step settles a round
// (target_order.hip.h).  Nothing of a run is touched, and nothing but its residents is read: the contig need not be collected.
cl_status cl_contig_target_order_ms(cl_ctx *c, double *kernel_ms, uint32_t *n_rounds)
{
    if (!c || !kernel_ms) return CL_ERR_INVALID;
    *kernel_ms = c->to_ms;
    if (n_rounds) *n_rounds = c->to_rounds;
    return CL_OK;
}

cl_status cl_contig_target_order(cl_ctx *c, const uint32_t *starts, const uint32_t *ends, size_t n_targets, const cl_target_order **out)
{
    return guarded(c, [&]() -> cl_status {
        if (!c) return CL_ERR_INVALID;
        if (!out) return fail(c, CL_ERR_INVALID, "cl_contig_target_order: null result");
        *out = nullptr;
        const cl_status ready = depth_call_ready(c, "cl_contig_target_order", false, [&]() -> cl_status {
            if (n_targets > CL_TARGETS_MAX) return fail(c, CL_ERR_INVALID, "cl_contig_target_order: more than 2^24 targets");
            if (n_targets && (!starts || !ends)) return fail(c, CL_ERR_INVALID, "cl_contig_target_order: null starts or ends");
            for (size_t i = 0; i < n_targets; ++i)
                if (starts[i] > ends[i]) return fail(c, CL_ERR_INVALID, "cl_contig_target_order: target " + std::to_string(i) + " has start > end");
            return CL_OK;
        }());
        if (ready != CL_OK) return ready;
        c->to_ms = 0.0; c->to_rounds = 0u;
        if (n_targets == 0) { HIP_TRY(c, hipStreamSynchronize(c->stream)); return CL_OK; }
        const size_t n = n_targets, nw = c->n_win;
        const uint32_t extent = c->extent;
        // (counted before a byte of the list is allocated)
        const uint64_t n_pc64 = target_piece_count(starts, ends, n, extent);
        if (n_pc64 > CL_TARGET_ORDER_MAX_PIECES)
            return fail(c, CL_ERR_INVALID, "cl_contig_target_order: the targets cut at the windows are " + std::to_string(n_pc64) +
                                           " pieces, more than the " + std::to_string(CL_TARGET_ORDER_MAX_PIECES) + " the call takes");
        static_assert(sizeof(cl_target_order) == kOrderWords * sizeof(uint32_t), "record layout");
        try {
            c->h_to_out.assign(n, cl_target_order{});
            c->h_to_tg.resize(2 * n);
        } catch (const std::bad_alloc &) { return fail(c, CL_ERR_NOMEM, "cl_contig_target_order: the records"); }
        for (size_t i = 0; i < n; ++i) {
            const ClippedTarget t = clip_target(starts[i], ends[i], extent);
            c->h_to_tg[2 * i] = t.s; c->h_to_tg[2 * i + 1] = t.e;
            c->h_to_out[i].start = t.s; c->h_to_out[i].end = t.e; c->h_to_out[i].len = t.e - t.s;
        }
        if (n_pc64 == 0 || nw == 0) {
            // (nothing to measure: every record is its clipped ends and zeros)
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            *out = c->h_to_out.data();
            return CL_OK;
        }
        try {
            if (!target_pieces_build(starts, ends, n, extent, c->n_win, c->h_to_pc, c->h_to_first))
                return fail(c, CL_ERR_INTERNAL, "cl_contig_target_order: the windows do not cover the extent");
        } catch (const std::bad_alloc &) { return fail(c, CL_ERR_NOMEM, "cl_contig_target_order: the pieces"); }
        const size_t n_pc = c->h_to_pc.size();
        // layout of the upload: pc[n_pc] (two words each), pc_first[nw + 1], tg[n][2]
        HIP_TRY(c, c->d_to_in.reserve(2 * n_pc + nw + 1 + 2 * n));
        HIP_TRY(c, c->d_to_st.reserve((size_t)kOrderStateWords * n + 2));
        HIP_TRY(c, c->d_to_out.reserve((size_t)kOrderWords * n));
        uint32_t *d_first = c->d_to_in.p + 2 * n_pc, *d_tg = d_first + nw + 1;
        uint32_t *d_max = c->d_to_st.p + (size_t)kOrderStateWords * n, *d_err = d_max + 1;
        HIP_TRY(c, hipMemcpyAsync(c->d_to_in.p, c->h_to_pc.data(), n_pc * sizeof(TargetPiece), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_first, c->h_to_first.data(), (nw + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_tg, c->h_to_tg.data(), 2 * n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_to_st.p, 0, ((size_t)kOrderStateWords * n + 2) * sizeof(uint32_t), c->stream));
        OrderArgs a{depth_residents(c), (uint32_t)n_pc, (uint32_t)n, reinterpret_cast<const uint2 *>(c->d_to_in.p), d_first, c->d_to_st.p, d_err, 0u, 0u};
        OrderStepArgs sa{d_tg, (uint32_t)n, extent, c->d_to_st.p, c->d_to_out.p, d_max, d_err, 1u, 0u, 0u, 0u};
        // workgroups that stay, as k_target_depth's; eight threads per target in the step
        const uint32_t grid = std::min<uint32_t>(c->n_win, 2048u);
        const uint32_t step_grid = (uint32_t)((8 * (uint64_t)n + kOrderStepBlock - 1) / kOrderStepBlock);
        // ---- the extremes, the ranks, the largest raw depth of any target ----
        if (c->profiling) HIP_TRY(c, c->t_to[0].start(c->stream));
        hipLaunchKernelGGL(depth_kernel(c, kTargetOrderFirstKernels), dim3(grid), dim3(kDepthBlock), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(k_target_order_step, dim3(step_grid), dim3(kOrderStepBlock), 0, c->stream, sa);
        HIP_TRY(c, hipGetLastError());
        if (c->profiling) HIP_TRY(c, c->t_to[0].stop(c->stream));
        uint32_t max_raw = 0u, err = 0u;
        HIP_TRY(c, hipMemcpyAsync(&max_raw, d_max, sizeof(max_raw), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        // ---- one round per bit of it, the most significant first ----
        uint32_t B = 0u;
        while (B < 32u && (max_raw >> B)) ++B;
        sa.first = 0u;
        if (B && c->profiling) HIP_TRY(c, c->t_to[1].start(c->stream));
        for (uint32_t bit = B; bit-- > 0u;) {
            a.bit = bit; sa.bit = bit; sa.last = bit == 0u ? 1u : 0u;
            hipLaunchKernelGGL(depth_kernel(c, kTargetOrderRoundKernels), dim3(grid), dim3(kDepthBlock), 0, c->stream, a);
            HIP_TRY(c, hipGetLastError());
            hipLaunchKernelGGL(k_target_order_step, dim3(step_grid), dim3(kOrderStepBlock), 0, c->stream, sa);
            HIP_TRY(c, hipGetLastError());
        }
        if (B && c->profiling) HIP_TRY(c, c->t_to[1].stop(c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->h_to_out.data(), c->d_to_out.p, n * sizeof(cl_target_order), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->to_rounds = B;
        if (c->profiling) {
            HIP_TRY(c, c->t_to[0].read());
            c->to_ms = c->t_to[0].ms;
            if (B) { HIP_TRY(c, c->t_to[1].read()); c->to_ms += c->t_to[1].ms; }
        }
        if (err) return fail(c, CL_ERR_INTERNAL, "cl_contig_target_order: a device-side check of the uploaded pieces or targets failed");
        *out = c->h_to_out.data();
        return CL_OK;
    });
}
#pragma clang diagnostic pop

} // extern "C"
