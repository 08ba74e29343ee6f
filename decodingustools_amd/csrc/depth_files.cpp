// depth_files.cpp -- dut_coverage_files_ex (include/dut_bam.h): the file-level coverage run that also takes every
// contig's depth profile (cl_contig_depth_profile) while the contig is resident, and writes the distribution, window and
// summary files of include/dut_coverage.h beside the BED.  The driver is coverage_files.cpp's; this file is its hook.
#include "coverage_hook.h"

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

void set_err(char *err, size_t n, const char *m) { if (err && n) snprintf(err, n, "%s", m); }

// the argument rules, before any file or device is touched
int check_options(const dut_depth_options *o, char *err, size_t err_len)
{
    if (o->n_bins < CL_DEPTH_MIN_BINS || o->n_bins > CL_DEPTH_MAX_BINS) { set_err(err, err_len, "depth profile: the number of bins (depth cap + 1) must be 2 to 4096"); return CL_ERR_INVALID; }
    if (o->windows_path && o->window < CL_DEPTH_MIN_WINDOW) { set_err(err, err_len, "depth profile: a window file needs a window of at least 16 positions"); return CL_ERR_INVALID; }
    return CL_OK;
}

} // namespace

extern "C" int dut_coverage_files_ex(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                                     const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                                     const int *devices, size_t n_devices, unsigned flags, const dut_depth_options *depth,
                                     char *err, size_t err_len)
{
    const bool any = depth && (depth->dist_path || depth->windows_path || depth->summary_path);
    if (!any)
        return dut_coverage_files_multi(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, err, err_len);
    if (check_options(depth, err, err_len) != CL_OK) return CL_ERR_INVALID;
    // the byte forms have no depth profile (cl_contig_depth_profile): said before anything is read
    { const char *qf = getenv("DUT_QUAL_FORM"); if (qf && strcmp(qf, "bytes") == 0) { set_err(err, err_len, "depth profile: pass-bit form only (DUT_QUAL_FORM=bytes is set)"); return CL_ERR_INVALID; } }
    try {
        DepthRun run;
        run.o = *depth;
        if (!run.o.windows_path) run.o.window = 0;             // no window file: no window table is taken
        run.acc = dut_depth_acc_new(run.o.n_bins, run.o.window, run.o.windows_path);
        if (!run.acc) { set_err(err, err_len, run.o.windows_path ? (std::string("cannot create ") + run.o.windows_path).c_str() : "out of memory"); return CL_ERR_INVALID; }
        const dut::ContigHook hook = {on_resident, on_deliver, on_finish, &run};
        const int rc = dut::coverage_files_hooked(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, err, err_len, &hook);
        if (rc != CL_OK && !run.msg.empty()) set_err(err, err_len, run.msg.c_str());   // the failure was this file's: its own words
        return rc;
    } catch (...) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_NOMEM; }
}
