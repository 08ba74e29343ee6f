// depth_runs.hip.h -- k_depth_runs: the per-position depth of the resident contig as runs of equal value, built on the
// device (cl_contig_depth_runs, include/callable_loci.h).  Included by callable_loci.hip behind depth_profile.hip.h.
//
// A sibling of k_depth_profile, a kernel of its own: it reads the same residents (window records, heads, wide list, rows)
// and rebuilds a depth per position with the same code (window_depths.hip.h) -- bit-sliced counter planes for qc, the
// scanned +-1 difference array for raw; 128 threads, a window of 2048, 16 positions per thread --, but only the kind the
// call asked for (QC: the raw kind reads no row, the qc kind no head), and instead of counting the depths it turns them
// into runs.  No per-position array reaches HBM.
//
//   value      no edges: the depth.  Edges e_0 < e_1 < ...: the number of edges <= depth (0 .. n_edges), looked up in a
//              copy of the edges in LDS, once per change of depth among a thread's positions
//   run start  position p < extent with p == 0 or value(p) != value(p - 1).  A thread's first position looks at the
//              previous thread's last value (through LDS); a window's first position is a provisional start
//   two passes over the windows (a.write = 0, then 1), both of which recompute the window:
//     count    cnt[w] = the window's starts (the provisional one included), first[w] and last[w] = the values at the
//              window's first and last position
//     (k_depth_runs_scan: exclusive scan of cnt[w] - drop(w) into 64-bit offsets, drop(w) = w > 0 and cnt[w] > 0 and
//              last[w - 1] == first[w]: the provisional start of a window that continues its predecessor's run)
//     write    start j of window w (j = 0: the provisional one, skipped when dropped) goes to slot off[w] + j - drop(w)
// Slots follow window order and position order inside a window: the output is ascending and the same on every call.  The
// write pass checks every slot against the capacity the host derived from the scan's total and raises *err instead of
// storing beyond it.
#pragma once

namespace clk {

constexpr int kRunsMaxEdges = 64;                          // CL_RUNS_MAX_EDGES
constexpr int kRunsScanBlock = 1024;

struct RunsArgs {
    DepthResidents res;
    uint32_t n_edges, write;
    uint32_t *cnt, *first, *last;      // [n_win] each: written by the count pass, read by the scan and the write pass
    const unsigned long long *off;     // [n_win]: the scan's offsets (write pass)
    uint32_t *start, *value;           // [cap] each (write pass)
    unsigned long long cap;
    uint32_t *err;                     // raised when a slot falls outside [0, cap)
    uint32_t edges[kRunsMaxEdges];
};

template <int NP, bool QC, bool HEAD4>
__global__ __launch_bounds__(kDepthBlock) void k_depth_runs(RunsArgs a)
{
    constexpr int T = kDepthT, BS = kDepthBlock, PER = kDepthPer;
    __shared__ __attribute__((aligned(16))) uint32_t s_diff[QC ? 4 : T];
    __shared__ uint32_t s_pl[QC ? NP : 1][64];             // wave 1's planes, then the window's (written by wave 0)
    __shared__ uint32_t s_edges[2 * kRunsMaxEdges];        // the edges, then 0xFFFFFFFF (the search probes below 128)
    __shared__ uint32_t s_lastv[BS];                       // a thread's last value, for its successor
    __shared__ uint32_t s_tot;                             // wave 0's total: of the differences, later of the starts
    __shared__ uint32_t s_cnt[2];

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t ne = a.n_edges < (uint32_t)kRunsMaxEdges ? a.n_edges : (uint32_t)kRunsMaxEdges;
    s_edges[tid] = tid < ne ? a.edges[tid & (uint32_t)(kRunsMaxEdges - 1)] : 0xFFFFFFFFu;
    // (read behind the barriers of the first window)
    auto value_of = [&](uint32_t d) -> uint32_t {
        uint32_t pos = 0u;
#pragma unroll
        for (uint32_t step = (uint32_t)kRunsMaxEdges; step; step >>= 1) {
            const uint32_t q = pos + step;                 // <= 127
            if (q <= ne && s_edges[q - 1u] <= d) pos = q;
        }
        return pos;
    };

    for (uint32_t w = blockIdx.x; w < a.res.n_win; w += gridDim.x) {
        const uint32_t W = w * (uint32_t)T;
        const WinMeta wm = a.res.win[w];
        uint32_t d[PER];
        if constexpr (!QC) {
            // ---- raw_depth (the raw kind reads no row) ----
            wd_clear(s_diff, tid);
            __syncthreads();
            wd_scatter<HEAD4>(a.res, wm, W, s_diff, tid);
            __syncthreads();
            const uint32_t excl = wd_diff_scan(d, s_diff, &s_tot, tid);
            __syncthreads();
            wd_diff_finish(d, excl, &s_tot, wv);
        } else {
            // ---- qc_depth (the qc kind reads no head) ----
            const RowLane rl = row_lane(a.res.rows, wm, lane, wv);
            uint32_t c[NP];
            wd_rows<NP>(c, rl, wm.rn, wv);
            if (wv != 0) wd_planes_put<NP>(c, s_pl, lane);
            __syncthreads();
            if (wv == 0) wd_planes_add<NP>(c, s_pl, lane);
            __syncthreads();
            wd_extract<NP>(d, s_pl, tid);
        }
        const DepthSpan sp = wd_span(W, tid, a.res.extent);
        const uint32_t p0 = sp.p0, n_ok = sp.n_ok;

        // ---- depth -> value (in place): a search per change of depth ----
        if (ne) {
            uint32_t pd = d[0], pv = value_of(pd);
            d[0] = pv;
#pragma unroll
            for (int i = 1; i < PER; ++i) {
                if (d[i] != pd) { pd = d[i]; pv = value_of(pd); }
                d[i] = pv;
            }
        }
        // ---- run starts among the positions below the extent: bit i of flags ----
        s_lastv[tid] = d[PER - 1];
        __syncthreads();
        uint32_t flags = 0u;
        {
            uint32_t prev = tid ? s_lastv[tid - 1u] : ~d[0];   // the window's first position: a provisional start
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if ((uint32_t)i < n_ok && d[i] != prev) flags |= 1u << i;
                prev = d[i];
            }
        }
        const uint32_t nloc = (uint32_t)__popc(flags);
        const uint32_t incl = dpp_incl_scan_u32(nloc);
        if (!a.write) {
            if (lane == 63u) s_cnt[wv] = incl;
            __syncthreads();
            if (tid == 0u) { a.cnt[w] = s_cnt[0] + s_cnt[1]; a.first[w] = d[0]; }
            if (tid == (uint32_t)BS - 1u) a.last[w] = d[PER - 1];
        } else {
            if (tid == 63u) s_tot = incl;
            __syncthreads();
            // (the very expression the scan took the offsets with)
            const uint32_t drop = (w > 0u && a.cnt[w] > 0u && a.last[w - 1u] == a.first[w]) ? 1u : 0u;
            const unsigned long long slot0 = a.off[w];
            uint32_t j = incl - nloc + (wv ? s_tot : 0u);  // this thread's first start among the window's
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if (flags & (1u << i)) {
                    if (j >= drop) {                       // (j == 0: the provisional start)
                        const unsigned long long slot = slot0 + (unsigned long long)(j - drop);
                        if (slot < a.cap) { a.start[slot] = p0 + (uint32_t)i; a.value[slot] = d[i]; }
                        else atomicOr(a.err, 1u);
                    }
                    ++j;
                }
            }
        }
        __syncthreads();                                   // the next window overwrites what this one read
    }
}

// The exclusive scan of the windows' start counts, less the dropped provisional starts, into 64-bit offsets; *total = the
// number of runs.  One workgroup, kRunsScanBlock windows per step (a step's sum is at most 2^10 * 2^11).
__global__ __launch_bounds__(kRunsScanBlock) void k_depth_runs_scan(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ first,
                                                                     const uint32_t *__restrict__ last, uint32_t n_win,
                                                                     unsigned long long *__restrict__ off, unsigned long long *__restrict__ total)
{
    __shared__ uint32_t s_w[kRunsScanBlock / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    unsigned long long run = 0ull;
    for (uint32_t base = 0; base < n_win; base += (uint32_t)kRunsScanBlock) {
        const uint32_t w = base + tid;
        uint32_t c = 0u;
        if (w < n_win) {
            c = cnt[w];
            if (w > 0u && c > 0u && last[w - 1u] == first[w]) c -= 1u;
        }
        const uint32_t inc = dpp_incl_scan_u32(c);
        if (lane == 63u) s_w[wv] = inc;
        __syncthreads();
        uint32_t o = inc - c, tot = 0u;
        for (uint32_t i = 0; i < (uint32_t)(kRunsScanBlock / 64); ++i) { const uint32_t v = s_w[i]; if (i < wv) o += v; tot += v; }
        if (w < n_win) off[w] = run + o;
        run += tot;
        __syncthreads();
    }
    if (tid == 0u) *total = run;
}

} // namespace clk
