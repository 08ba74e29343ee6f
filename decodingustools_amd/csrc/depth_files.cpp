// depth_files.cpp -- dut_coverage_files_ex / _ex2 (include/dut_bam.h): the file-level coverage run that also takes every
// contig's depth profile (cl_contig_depth_profile) and / or its per-base depth runs (cl_contig_depth_runs) while the
// contig is resident, and writes the distribution, window and summary files and the depth BED of include/dut_coverage.h
// beside the BED.  The driver is coverage_files.cpp's; this file is its hook: two users (DepthRun, BedRun), composed in
// Both when a run asks for both.
#include "coverage_hook.h"
#include "../../include/dut_coverage.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace {

// one contig's profile on its way from its device's thread to the accumulator (the engine's arrays live until the
// context's next profile or contig)
struct Taken {
    cl_depth_profile p{};
    std::vector<uint64_t> data;          // hist_raw, hist_qc, win_raw, win_qc
};

struct DepthRun {
    dut_depth_options o{};
    dut_depth_acc *acc = nullptr;
    std::mutex mu;
    std::map<size_t, Taken> taken;       // by selected-contig index
    std::string msg;                     // why deliver / finish failed (the calling thread's; the driver knows only the status)
    ~DepthRun() { dut_depth_acc_free(acc); }
};

int on_resident(void *user, cl_ctx *ctx, size_t i)
{
    DepthRun *r = static_cast<DepthRun *>(user);
    cl_depth_profile p;
    const int rc = cl_contig_depth_profile(ctx, r->o.n_bins, r->o.window, &p);
    if (rc != CL_OK) return rc;
    Taken t;
    t.p = p;
    t.data.reserve(2 * (size_t)p.n_bins + 2 * (size_t)p.n_windows);
    t.data.insert(t.data.end(), p.hist_raw, p.hist_raw + p.n_bins);
    t.data.insert(t.data.end(), p.hist_qc, p.hist_qc + p.n_bins);
    if (p.n_windows) {
        t.data.insert(t.data.end(), p.win_raw, p.win_raw + p.n_windows);
        t.data.insert(t.data.end(), p.win_qc, p.win_qc + p.n_windows);
    }
    std::lock_guard<std::mutex> g(r->mu);
    r->taken[i] = std::move(t);
    return CL_OK;
}

int on_deliver(void *user, size_t i, const char *name)
{
    DepthRun *r = static_cast<DepthRun *>(user);
    Taken t;
    {
        std::lock_guard<std::mutex> g(r->mu);
        auto it = r->taken.find(i);
        if (it == r->taken.end()) return CL_ERR_INVALID;
        t = std::move(it->second);
        r->taken.erase(it);
    }
    const uint64_t *d = t.data.data();
    t.p.hist_raw = d; t.p.hist_qc = d + t.p.n_bins;
    t.p.win_raw = t.p.n_windows ? d + 2 * (size_t)t.p.n_bins : nullptr;
    t.p.win_qc = t.p.n_windows ? d + 2 * (size_t)t.p.n_bins + t.p.n_windows : nullptr;
    const int rc = dut_depth_acc_add(r->acc, name, &t.p);
    if (rc != CL_OK)
        r->msg = rc == CL_ERR_NOMEM ? "out of memory" : std::string("cannot write ") + (r->o.windows_path ? r->o.windows_path : "the depth profile") + " (contig " + name + ")";
    return rc;
}

int on_finish(void *user)
{
    DepthRun *r = static_cast<DepthRun *>(user);
    const int rc = dut_depth_acc_finish(r->acc, r->o.dist_path, r->o.summary_path);
    if (rc != CL_OK) {
        r->msg = "cannot write the depth profile files:";
        for (const char *p : {r->o.windows_path, r->o.dist_path, r->o.summary_path}) if (p) r->msg += std::string(" ") + p;
    }
    return rc;
}

// ---- the depth BED: one contig's runs on their way from its device's thread to the file ----
struct TakenRuns {
    uint64_t extent = 0, n_runs = 0;
    std::vector<uint32_t> data;          // start[n_runs], value[n_runs]
};

struct BedRun {
    std::string path;
    uint32_t kind = CL_DEPTH_RAW;
    std::vector<uint32_t> edges;
    FILE *f = nullptr;
    std::mutex mu;
    std::map<size_t, TakenRuns> taken;   // by selected-contig index
    std::string msg;
    ~BedRun() { if (f) fclose(f); }
};

int bed_resident(void *user, cl_ctx *ctx, size_t i)
{
    BedRun *r = static_cast<BedRun *>(user);
    cl_depth_runs d;
    const int rc = cl_contig_depth_runs(ctx, r->kind, r->edges.data(), (uint32_t)r->edges.size(), &d);
    if (rc != CL_OK) return rc;
    TakenRuns t;
    t.extent = d.extent; t.n_runs = d.n_runs;
    t.data.reserve(2 * (size_t)d.n_runs);
    if (d.n_runs) {
        t.data.insert(t.data.end(), d.start, d.start + d.n_runs);
        t.data.insert(t.data.end(), d.value, d.value + d.n_runs);
    }
    std::lock_guard<std::mutex> g(r->mu);
    r->taken[i] = std::move(t);
    return CL_OK;
}

int bed_deliver(void *user, size_t i, const char *name)
{
    BedRun *r = static_cast<BedRun *>(user);
    TakenRuns t;
    {
        std::lock_guard<std::mutex> g(r->mu);
        auto it = r->taken.find(i);
        if (it == r->taken.end()) return CL_ERR_INVALID;
        t = std::move(it->second);
        r->taken.erase(it);
    }
    cl_depth_runs d{};
    d.kind = r->kind; d.n_edges = (uint32_t)r->edges.size(); d.extent = t.extent; d.n_runs = t.n_runs;
    d.start = t.data.data(); d.value = t.data.data() + t.n_runs;
    const int rc = dut_depth_bed_write(r->f, name, &d, r->edges.data());
    if (rc != CL_OK) r->msg = rc == CL_ERR_NOMEM ? "out of memory" : "cannot write " + r->path + " (contig " + name + ")";
    return rc;
}

int bed_finish(void *user)
{
    BedRun *r = static_cast<BedRun *>(user);
    const int rc = fclose(r->f) == 0 ? CL_OK : CL_ERR_INVALID;
    r->f = nullptr;
    if (rc != CL_OK) r->msg = "cannot write " + r->path;
    return rc;
}

// both users behind one hook: the profile first, then the runs
struct Both { DepthRun *depth; BedRun *bed; };
int both_resident(void *user, cl_ctx *ctx, size_t i)
{
    Both *b = static_cast<Both *>(user);
    const int rc = on_resident(b->depth, ctx, i);
    return rc != CL_OK ? rc : bed_resident(b->bed, ctx, i);
}
int both_deliver(void *user, size_t i, const char *name)
{
    Both *b = static_cast<Both *>(user);
    const int rc = on_deliver(b->depth, i, name);
    return rc != CL_OK ? rc : bed_deliver(b->bed, i, name);
}
int both_finish(void *user)
{
    Both *b = static_cast<Both *>(user);
    const int rc = on_finish(b->depth), rc2 = bed_finish(b->bed);  // (both files are closed either way)
    return rc != CL_OK ? rc : rc2;
}

void set_err(char *err, size_t n, const char *m) { if (err && n) snprintf(err, n, "%s", m); }

// the argument rules, before any file or device is touched
int check_options(const dut_depth_options *o, char *err, size_t err_len)
{
    if (o->n_bins < CL_DEPTH_MIN_BINS || o->n_bins > CL_DEPTH_MAX_BINS) { set_err(err, err_len, "depth profile: the number of bins (depth cap + 1) must be 2 to 4096"); return CL_ERR_INVALID; }
    if (o->windows_path && o->window < CL_DEPTH_MIN_WINDOW) { set_err(err, err_len, "depth profile: a window file needs a window of at least 16 positions"); return CL_ERR_INVALID; }
    return CL_OK;
}

int check_bed_options(const dut_depth_bed_options *o, char *err, size_t err_len)
{
    const char *m = nullptr;
    if (o->kind != CL_DEPTH_RAW && o->kind != CL_DEPTH_QC) m = "depth BED: unknown depth kind (raw or qc)";
    else if (o->n_edges > CL_RUNS_MAX_EDGES) m = "depth BED: more than 64 edges";
    else if (o->n_edges && !o->edges) m = "depth BED: null edges";
    else if (o->n_edges && o->edges[0] == 0u) m = "depth BED: the first edge is 0";
    for (uint32_t i = 1; !m && i < o->n_edges; ++i) if (o->edges[i] <= o->edges[i - 1]) m = "depth BED: the edges are not strictly ascending";
    if (m) { set_err(err, err_len, m); return CL_ERR_INVALID; }
    return CL_OK;
}

} // namespace

extern "C" int dut_coverage_files_ex(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                                     const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                                     const int *devices, size_t n_devices, unsigned flags, const dut_depth_options *depth,
                                     char *err, size_t err_len)
{
    return dut_coverage_files_ex2(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, depth, nullptr, err, err_len);
}

extern "C" int dut_coverage_files_ex2(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                                      const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                                      const int *devices, size_t n_devices, unsigned flags, const dut_depth_options *depth,
                                      const dut_depth_bed_options *bed, char *err, size_t err_len)
{
    const bool any = depth && (depth->dist_path || depth->windows_path || depth->summary_path);
    const bool any_bed = bed && bed->path;
    if (!any && !any_bed)
        return dut_coverage_files_multi(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, err, err_len);
    if (any && check_options(depth, err, err_len) != CL_OK) return CL_ERR_INVALID;
    if (any_bed && check_bed_options(bed, err, err_len) != CL_OK) return CL_ERR_INVALID;
    // the byte forms have neither (cl_contig_depth_profile, cl_contig_depth_runs): said before anything is read
    { const char *qf = getenv("DUT_QUAL_FORM"); if (qf && strcmp(qf, "bytes") == 0) { set_err(err, err_len, any ? "depth profile: pass-bit form only (DUT_QUAL_FORM=bytes is set)" : "depth BED: pass-bit form only (DUT_QUAL_FORM=bytes is set)"); return CL_ERR_INVALID; } }
    try {
        DepthRun run;
        BedRun brun;
        if (any) {
            run.o = *depth;
            if (!run.o.windows_path) run.o.window = 0;             // no window file: no window table is taken
            run.acc = dut_depth_acc_new(run.o.n_bins, run.o.window, run.o.windows_path);
            if (!run.acc) { set_err(err, err_len, run.o.windows_path ? (std::string("cannot create ") + run.o.windows_path).c_str() : "out of memory"); return CL_ERR_INVALID; }
        }
        if (any_bed) {
            brun.path = bed->path; brun.kind = bed->kind;
            brun.edges.assign(bed->edges, bed->edges + bed->n_edges);
            brun.f = fopen(bed->path, "wb");
            if (!brun.f) { set_err(err, err_len, ("cannot create " + brun.path).c_str()); return CL_ERR_INVALID; }
        }
        Both both = {&run, &brun};
        const dut::ContigHook hook = any && any_bed ? dut::ContigHook{both_resident, both_deliver, both_finish, &both}
                                     : any        ? dut::ContigHook{on_resident, on_deliver, on_finish, &run}
                                                  : dut::ContigHook{bed_resident, bed_deliver, bed_finish, &brun};
        const int rc = dut::coverage_files_hooked(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, err, err_len, &hook);
        // the failure was this file's: its own words
        if (rc != CL_OK && !run.msg.empty()) set_err(err, err_len, run.msg.c_str());
        else if (rc != CL_OK && !brun.msg.empty()) set_err(err, err_len, brun.msg.c_str());
        return rc;
    } catch (...) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_NOMEM; }
}
