// coverage_files.cpp -- the file-level `coverage` driver of include/dut_bam.h (dut_coverage_files,
// dut_coverage_files_multi; CoverageAnalyzer::run_analysis, api/coverage.rs:53-115): BAM + FASTA in, BED, figures and
// summary JSON / HTML out, over one engine context or several.  Orchestration only: the readers are bam_io.cpp's, the
// per-contig work host_coverage.cpp's and the device engine's.
#include "../../include/dut_bam.h"
#include "../../include/dut_report.h"
#include "coverage_hook.h"
#include "host_parallel.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace dut {
void bam_release_for_exit(dut_bam *b);          // bam_io.cpp
}

namespace {

void set_err(char *err, size_t n, const std::string &m)
{
    if (err && n) { snprintf(err, n, "%s", m.c_str()); }
}

using BamPtr = std::unique_ptr<dut_bam, decltype(&dut_bam_close)>;
using FastaPtr = std::unique_ptr<dut_fasta, decltype(&dut_fasta_close)>;
using CtxPtr = std::unique_ptr<cl_ctx, decltype(&cl_destroy)>;

// a BAM and a FASTA reader of the two files; false, with the caller's message, when either cannot be opened
bool open_pair(const char *bam_path, const char *fasta_path, BamPtr &b, FastaPtr &f, std::string &msg)
{
    char e[512] = {0};
    b.reset(dut_bam_open(bam_path, e, sizeof(e)));
    if (!b) { msg = std::string("Failed to open BAM file: ") + e; return false; }             // api/coverage.rs:69-70
    f.reset(dut_fasta_open(fasta_path, e, sizeof(e)));
    if (!f) { b.reset(); msg = std::string("Failed to open reference: ") + e; return false; }   // :73-74
    return true;
}

// Contigs dealt to devices by longest-processing-time-first: the heaviest contig next, to the device with the least
// load so far (weights: the index's mapped-read counts when it records them, the contig lengths otherwise).
std::vector<int> lpt_deal(const std::vector<uint64_t> &weight, size_t n_dev)
{
    std::vector<size_t> order(weight.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weight[a] > weight[b]; });
    std::vector<uint64_t> load(n_dev, 0);
    std::vector<int> owner(weight.size(), 0);
    for (size_t i : order) {
        size_t best = 0;
        for (size_t d = 1; d < n_dev; ++d) if (load[d] < load[best]) best = d;
        owner[i] = (int)best; load[best] += weight[i] + 1;
    }
    return owner;
}

// what ended a device's contigs early: the status and the caller's message
struct Stop { int rc = CL_OK; std::string msg; };
// one contig's result on its way to the BED (the intervals are the engine's until its context's next contig)
struct Result { dut_contig_stats st{}; uint64_t counts[6] = {0}; const cl_interval *iv = nullptr; size_t n_iv = 0; };

int coverage_files(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                   const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                   const int *devices, size_t n_devices, unsigned flags, char *err, size_t err_len, const dut::ContigHook *hook)
{
    if (!bam_path || !fasta_path || !bed_path || !opt || !devices || n_devices == 0) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    const bool leave = (flags & DUT_FILES_LEAVE_TO_EXIT) != 0;
    // the engine's default form wants one bit per base (cl_create reads the same variable): the reader then takes the
    // base-quality test while it parses the records and no quality byte leaves it
    const char *qf = getenv("DUT_QUAL_FORM");
    const char *pr = getenv("DUT_PACKED_READER");                   // =0: bytes from the reader, tested in cl_push_reads (for A/B timing)
    const bool use_bits = !(qf && strcmp(qf, "bytes") == 0) && !(pr && pr[0] == '0');
    const char *pe = getenv("DUT_PIPELINE");
    char e[512] = {0};
    double tm = dut::now_s();
    std::unique_ptr<dut_bam_stats, decltype(&dut_bam_stats_free)> bstats(dut_bam_stats_new(10000), dut_bam_stats_free);   // api/coverage.rs:56-59
    if (dut_bam_stats_collect(bstats.get(), bam_path, e, sizeof(e)) != CL_OK) { set_err(err, err_len, std::string("Failed to collect BAM stats: ") + e); return CL_ERR_INVALID; }
    BamPtr bam(nullptr, dut_bam_close);
    FastaPtr fa(nullptr, dut_fasta_close);
    std::string msg;
    if (!open_pair(bam_path, fasta_path, bam, fa, msg)) { set_err(err, err_len, msg); return CL_ERR_INVALID; }
    if (hook && hook->header) {
        std::vector<const char *> refs;
        for (int t = 0; t < dut_bam_n_ref(bam.get()); ++t) refs.push_back(dut_bam_ref_name(bam.get(), t));
        const int hrc = hook->header(hook->user, refs.data(), refs.size());
        if (hrc != CL_OK) { set_err(err, err_len, "the hook refused the BAM header"); return hrc; }
    }
    // initialize_contig_stats / validate_contig_selection, api/coverage.rs:149-204
    std::vector<int> tids;
    std::vector<uint64_t> weight;
    for (int t = 0; t < dut_bam_n_ref(bam.get()); ++t) {
        bool take = contigs == nullptr;
        for (size_t i = 0; !take && i < n_contigs; ++i) take = strcmp(contigs[i], dut_bam_ref_name(bam.get(), t)) == 0;
        if (!take) continue;
        const int64_t m = dut_bam_ref_mapped(bam.get(), t);
        tids.push_back(t); weight.push_back(m >= 0 ? (uint64_t)m : (uint64_t)dut_bam_ref_len(bam.get(), t));
    }
    const size_t n_dev = tids.empty() ? 1 : n_devices;
    const std::vector<int> owner = lpt_deal(weight, n_dev);
    std::vector<CtxPtr> ctx;
    for (size_t d = 0; d < n_dev; ++d) ctx.emplace_back(nullptr, cl_destroy);
    std::unique_ptr<dut_profiler, decltype(&dut_profiler_free)> prof(nullptr, dut_profiler_free);
    std::vector<dut_contig_stats> stats;
    std::vector<std::string> names;
    std::vector<uint64_t> counts;                                  // 6 per contig

    // the BED writer, its figures sized by the longest selected contig but chrM (api/coverage.rs:210-215)
    auto open_bed = [&]() -> Stop {
        prof.reset(dut_profiler_new(bed_path));
        if (!prof) return {CL_ERR_INVALID, std::string("Failed to create CallableProfiler: cannot create ") + bed_path};
        uint32_t largest = 0;
        for (int t : tids) if (strcmp(dut_bam_ref_name(bam.get(), t), "chrM") != 0) largest = std::max(largest, dut_bam_ref_len(bam.get(), t));
        dut_profiler_enable_plots(prof.get(), largest);
        return {};
    };
    // selected contig i's BED lines and figure (finish_contig, :64-84), in tid order, and its line of the summary
    auto write_bed = [&](size_t i, const Result &r) -> int {
        const char *nm = dut_bam_ref_name(bam.get(), tids[i]);
        double tb = dut::now_s();
        int rc = dut_profiler_feed_contig(prof.get(), nm, r.iv, r.n_iv, r.counts);
        if (rc == CL_OK && dut_profiler_finish_plot(prof.get(), nm, dut_bam_ref_len(bam.get(), tids[i])) < 0) rc = CL_ERR_INVALID;
        dut::stage_lap("BED lines", tb);
        if (rc != CL_OK) return rc;
        uint64_t c6[6];
        dut_profiler_contig_counts(prof.get(), nm, c6);
        stats.push_back(r.st); names.push_back(nm); counts.insert(counts.end(), c6, c6 + 6);
        if (hook && hook->deliver) return hook->deliver(hook->user, i, nm);   // (what `resident` took of it: in tid order too)
        return CL_OK;
    };
    // a contig's records beside its reference bases (one thread: read + strip the line ends); a zero-length contig
    // fetches no bases: the reference's loops over it run zero times (mod.rs:65-147), so a FASTA may lack its @SQ
    struct Slot { dut_bam *b; dut_fasta *f; dut_records rec{}; const uint8_t *bases = nullptr; uint64_t blen = 0; int rc = CL_OK, frc = CL_OK; };
    auto fetch = [&](Slot &s, int t) {
        s.bases = nullptr; s.blen = 0; s.frc = CL_OK;
        dut::Thread fb;
        if (dut_bam_ref_len(s.b, t) > 0) fb = dut::spawn_or_run([&]() { s.frc = dut_fasta_fetch(s.f, dut_bam_ref_name(s.b, t), &s.bases, &s.blen); });
        s.rc = use_bits ? dut_bam_read_contig_bits(s.b, t, opt->min_base_quality, &s.rec) : dut_bam_read_contig(s.b, t, &s.rec, nullptr, nullptr);
        if (fb.joinable()) fb.join();
    };
    // Device d's contigs in ascending tid order (api/coverage.rs:229-234), through the reader pair (b, f), opened here
    // when empty, and ctx[d], which comes up on its own thread while the first contig is read.  One device with an index
    // and more than one contig reads the next contig on a second reader pair, on its own thread, while the current one is
    // admitted, pushed, run and written (DUT_PIPELINE=0: off).  ready() once the context is up, put(i, result) for every
    // contig; both return a status.  Stage laps on *t0 when given.
    auto work = [&](size_t d, BamPtr &b, FastaPtr &f, double *t0, auto &&ready, auto &&put) -> Stop {
        auto lap = [&](const char *what) { if (t0) dut::stage_lap(what, *t0); };
        std::vector<size_t> mine;
        for (size_t i = 0; i < tids.size(); ++i) if (owner[i] == (int)d) mine.push_back(i);
        int crc = CL_OK;
        dut::Thread init = dut::spawn_or_run([&]() { cl_ctx *c = nullptr; crc = cl_create(opt, devices[d], nullptr, &c); ctx[d].reset(c); });
        std::string open_msg, unused;
        const bool opened = b || open_pair(bam_path, fasta_path, b, f, open_msg);
        BamPtr b2(nullptr, dut_bam_close);
        FastaPtr f2(nullptr, dut_fasta_close);
        const bool ahead = n_dev == 1 && mine.size() > 1 && dut_bam_has_index(b.get()) && !(pe && *pe == '0') &&
                           open_pair(bam_path, fasta_path, b2, f2, unused);   // (no second pair, e.g. out of file handles: in line)
        Slot slot[2] = {{b.get(), f.get()}, {b2.get(), f2.get()}};
        lap("(before contigs)");
        if (opened && !mine.empty()) fetch(slot[0], tids[mine[0]]);
        if (init.joinable()) init.join();
        if (crc != CL_OK) return {crc, "no usable HIP device (the engine has no CPU fallback)"};
        if (!opened) return {CL_ERR_INVALID, open_msg};
        if (Stop s = ready(); s.rc != CL_OK) return s;
        for (size_t k = 0; k < mine.size(); ++k) {
            const size_t i = mine[k];
            const int t = tids[i];
            Slot &cur = slot[ahead ? k & 1 : 0];
            if (k > 0 && !ahead) fetch(cur, t);
            lap(ahead && k > 0 ? "wait for the read-ahead" : "BAM read + decode, FASTA fetch");
            dut::Thread next;                                       // (joined at the end of the iteration, on every path)
            if (ahead && k + 1 < mine.size()) { Slot &nx = slot[(k + 1) & 1]; const int tn = tids[mine[k + 1]]; next = dut::spawn_or_run([&fetch, &nx, tn]() { fetch(nx, tn); }); }
            if (cur.rc != CL_OK) return {cur.rc, std::string("Error processing contig: ") + dut_bam_error(cur.b)};
            if (cur.frc != CL_OK) return {cur.frc, std::string("Error processing contig: ") + dut_fasta_error(cur.f)};   // fetch_seq(..)?, mod.rs:79
            Result r;
            int rc = dut_process_single_contig_runs(ctx[d].get(), &r.st, opt, t, dut_bam_ref_len(b.get(), t), cur.bases, cur.blen, &cur.rec, r.counts, &r.iv, &r.n_iv);
            // (the contig is still resident: what else a caller wants of it is taken here, on the device's thread)
            if (rc == CL_OK && hook && hook->resident) rc = hook->resident(hook->user, ctx[d].get(), i, dut_bam_ref_name(b.get(), t));
            if (rc == CL_OK && hook && hook->resident_ref) rc = hook->resident_ref(hook->user, ctx[d].get(), i, dut_bam_ref_name(b.get(), t), cur.bases, cur.blen);
            if (rc == CL_OK) rc = put(i, r);
            if (rc != CL_OK) {
                const char *m = cl_last_error(ctx[d].get());
                return {rc, std::string("Error processing contig: ") + ((m && *m) ? m : (rc == CL_ERR_UNSORTED ? "the input is not sorted" : "failed"))};
            }
        }
        return {};
    };

    Stop s;
    if (contigs && tids.empty()) {
        std::string list;
        for (size_t i = 0; i < n_contigs; ++i) { if (i) list += ", "; list += contigs[i]; }
        s = {CL_ERR_INVALID, "None of the specified contigs (" + list + ") were found in the BAM file"};
    } else if (n_dev == 1) {
        s = work(0, bam, fa, &tm, open_bed, write_bed);          // one device: each contig's BED lines as soon as it is done
    } else {
        // ---- several devices: one host thread, one reader pair (the first device's: the one opened above) and one engine
        //      context per device; the contigs dealt by LPT; every contig's runs, counts and statistics come back through
        //      host memory and the BED is written here, in tid order (api/coverage.rs:229-234 is a serial loop with no
        //      cross-contig state but the BED writer's pending line, callable_profiler.rs:64-66).  No collective. ----
        dut::stage_lap("(before contigs)", tm);
        s = open_bed();
        struct Handed { bool done = false; Stop stop; Result r; std::vector<cl_interval> iv; };
        std::vector<Handed> res(tids.size());
        std::mutex mu;
        std::condition_variable cv;
        std::atomic<bool> stop{false};
        auto hand_over = [&](size_t i, const Result &r) {
            { std::lock_guard<std::mutex> g(mu); res[i].r = r; res[i].iv.assign(r.iv, r.iv + r.n_iv); res[i].done = true; }
            cv.notify_all();
            return stop.load() ? CL_ERR_INVALID : CL_OK;               // the caller has met an error: the rest is abandoned
        };
        std::vector<dut::Thread> workers;
        for (size_t d = 0; s.rc == CL_OK && d < n_dev; ++d)
            workers.push_back(dut::spawn_or_run([&, d]() {
                BamPtr b(nullptr, dut_bam_close);
                FastaPtr f(nullptr, dut_fasta_close);
                Stop ws;
                try { ws = work(d, d ? b : bam, d ? f : fa, nullptr, [] { return Stop(); }, hand_over); }
                catch (...) { ws = {CL_ERR_NOMEM, "out of memory or internal error"}; }
                {   // (its contigs before the failing one are all handed over)
                    std::lock_guard<std::mutex> g(mu);
                    for (size_t i = 0; ws.rc != CL_OK && i < tids.size(); ++i)
                        if (owner[i] == (int)d && !res[i].done) { res[i].stop = ws; res[i].done = true; }
                }
                cv.notify_all();
                if (leave) { dut::bam_release_for_exit(b.release()); (void)f.release(); }
                else ctx[d].reset();                               // beside the other devices' (its readers: on the way out)
            }));
        // the BED, in tid order, as each contig's result arrives; the first error in tid order ends it
        for (size_t i = 0; s.rc == CL_OK && i < tids.size(); ++i) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return res[i].done; });
            Handed h = std::move(res[i]);
            lk.unlock();
            if (h.stop.rc != CL_OK) { s = h.stop; break; }
            h.r.iv = h.iv.data();
            const int rc = write_bed(i, h.r);
            if (rc != CL_OK) s = {rc, std::string("cannot write ") + bed_path};
        }
        stop.store(true);
        workers.clear();                                           // joins
        dut::stage_lap("contigs over the devices", tm);
    }

    int rc = s.rc;
    if (rc != CL_OK) set_err(err, err_len, s.msg);
    else if (hook && hook->finish && (rc = hook->finish(hook->user)) != CL_OK) set_err(err, err_len, "cannot write the depth profile files");
    if (rc == CL_OK && (summary_json || summary_html)) {
        // collect_coverage_plots (api/coverage.rs:263-274): the figures that exist relative to the working directory
        // (they are written beside the BED file); listed in tid order here, in HashMap order there
        std::vector<std::string> plots;
        std::vector<const char *> nm, plot_ptrs;
        for (const std::string &n : names) {
            nm.push_back(n.c_str());
            if (FILE *pf = fopen((n + "_coverage.svg").c_str(), "rb")) { fclose(pf); plots.push_back(n + "_coverage.svg"); }
        }
        for (const std::string &q : plots) plot_ptrs.push_back(q.c_str());
        dut_export_meta meta;
        memset(&meta, 0, sizeof(meta));
        meta.aligner = dut_bam_stats_aligner(bstats.get());
        meta.reference_build = dut_bam_stats_reference_build(bstats.get());
        meta.sequencing_platform = dut_bam_stats_infer_platform(bstats.get());
        meta.read_length = dut_bam_stats_average_read_length(bstats.get());
        meta.bed_file = bed_path;
        meta.summary_html = summary_html ? summary_html : "summary.html";
        meta.coverage_plots = plot_ptrs.data(); meta.n_coverage_plots = plot_ptrs.size();
        if (summary_html) {                                       // api/coverage.rs:104
            rc = dut_write_html_report(stats.data(), nm.data(), counts.data(), stats.size(), &meta, 10000, summary_html);
            if (rc != CL_OK) set_err(err, err_len, std::string("cannot create ") + summary_html);
        }
        if (rc == CL_OK && summary_json) {                        // CoverageOutput as main.rs:68-69 serialises it
            char *js = nullptr; size_t jl = 0;
            rc = dut_coverage_output_json(stats.data(), nm.data(), counts.data(), stats.size(), &meta, &js, &jl);
            std::unique_ptr<char, decltype(&dut_free)> json(js, dut_free);
            FILE *jf = nullptr;
            if (rc != CL_OK) set_err(err, err_len, "cannot build the summary");
            else if (!(jf = fopen(summary_json, "wb"))) { set_err(err, err_len, std::string("cannot create ") + summary_json); rc = CL_ERR_INVALID; }
            else { fwrite(js, 1, jl, jf); fclose(jf); }
        }
    }
    dut::stage_lap("(since the last decode) + summary", tm);
    bstats.reset();
    prof.reset();
    if (leave) {
        // the caller is about to leave the process (DUT_FILES_LEAVE_TO_EXIT: the command line tool): every result is on
        // disk; the device contexts, the readers and their decode buffers are left to the exit -- giving them back one by
        // one costs a few hundred milliseconds of page-table and driver work that the exit does once, in one sweep
        dut::bam_release_for_exit(bam.release());
        (void)fa.release();
        for (CtxPtr &c : ctx) (void)c.release();
        dut::stage_lap("left to the exit", tm);
        return rc;
    }
    // giving the device memory back and unmapping the decode buffers take a few hundred ms at chr21 size: side by side,
    // and both joined -- a library call leaves no thread behind
    dut::Thread td = dut::spawn_or_run([&]() { for (CtxPtr &c : ctx) c.reset(); });
    fa.reset();
    bam.reset();
    dut::stage_lap("readers closed", tm);
    if (td.joinable()) td.join();
    dut::stage_lap("engine destroyed", tm);
    return rc;
}

} // namespace

int dut::coverage_files_hooked(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                               const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                               const int *devices, size_t n_devices, unsigned flags, char *err, size_t err_len, const ContigHook *hook)
{
    // no exception leaves the library through the C ABI
    try { return coverage_files(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, err, err_len, hook); }
    catch (const std::bad_alloc &) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_NOMEM; }
    catch (...) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_INVALID; }
}

extern "C" int dut_coverage_files(const char *bam_path, const char *fasta_path, const char *bed_path,
                                  const char *summary_json, const char *summary_html, const cl_options *opt,
                                  const char *const *contigs, size_t n_contigs, int device_id, char *err, size_t err_len)
{
    return dut_coverage_files_multi(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, &device_id, 1, 0u, err, err_len);
}

extern "C" int dut_coverage_files_multi(const char *bam_path, const char *fasta_path, const char *bed_path,
                                        const char *summary_json, const char *summary_html, const cl_options *opt,
                                        const char *const *contigs, size_t n_contigs, const int *devices, size_t n_devices,
                                        unsigned flags, char *err, size_t err_len)
{
    return dut::coverage_files_hooked(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, err, err_len, nullptr);
}
