// depth_files.cpp -- dut_coverage_files_ex / _ex2 / _ex3 / _ex4 / _ex5 (include/dut_bam.h): the file-level coverage run that also takes
// every contig's depth profile (cl_contig_depth_profile), its per-base depth runs (cl_contig_depth_runs) and / or the
// summaries of its targets (cl_contig_targets) while the contig is resident, and writes the distribution, window and
// summary files, the depth BED and the per-target table of include/dut_coverage.h beside the BED.  The driver is
// coverage_files.cpp's; this file is its hook: three users (DepthRun, BedRun, TargetRun), as many of them as a run asks
// for behind one hook that calls them in that order (Many).  A fourth user, GcRun, takes the contig's GC-bias record
// (cl_contig_gc_bias) from the bases the driver holds and writes the bias table and summary.
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

int on_resident(void *user, cl_ctx *ctx, size_t i, const char *)
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

int bed_resident(void *user, cl_ctx *ctx, size_t i, const char *)
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

// ---- the per-target table: one contig's records on their way from its device's thread to the file ----
struct TargetRun {
    std::string bed_path, out_path;
    std::vector<uint32_t> thr;
    std::unique_ptr<dut_targets, decltype(&dut_targets_free)> tg{nullptr, dut_targets_free};
    std::map<std::string, size_t> by_name;               // contig name -> its index in tg
    FILE *f = nullptr;
    dut_target_total total{};
    std::mutex mu;
    std::map<size_t, std::vector<cl_target_stats>> taken;   // by selected-contig index (contigs with targets only)
    bool order = false;                                  // DUT_TARGETS_ORDER: the ten columns of cl_contig_target_order too
    std::map<size_t, std::vector<cl_target_order>> taken_order;
    std::string msg;
    ~TargetRun() { if (f) fclose(f); }
};

// every contig of the regions must be one of the BAM's: a misspelt contig would otherwise silently report nothing
int tg_header(void *user, const char *const *refs, size_t n_refs)
{
    TargetRun *r = static_cast<TargetRun *>(user);
    for (size_t c = 0; c < dut_targets_n_contigs(r->tg.get()); ++c) {
        const char *name = dut_targets_contig(r->tg.get(), c, nullptr);
        bool found = false;
        for (size_t t = 0; !found && t < n_refs; ++t) found = strcmp(refs[t], name) == 0;
        if (!found) {
            const uint32_t *lines = nullptr;
            dut_targets_get(r->tg.get(), c, nullptr, nullptr, nullptr, &lines);
            r->msg = r->bed_path + ": line " + std::to_string(lines[0]) + ": contig '" + name + "' is not in the BAM header";
            return CL_ERR_INVALID;
        }
    }
    return CL_OK;
}

int tg_resident(void *user, cl_ctx *ctx, size_t i, const char *name)
{
    TargetRun *r = static_cast<TargetRun *>(user);
    const auto it = r->by_name.find(name);
    if (it == r->by_name.end()) return CL_OK;             // no target on this contig: no launch, no line
    size_t n = 0;
    const uint32_t *s = nullptr, *e = nullptr;
    dut_targets_contig(r->tg.get(), it->second, &n);
    dut_targets_get(r->tg.get(), it->second, &s, &e, nullptr, nullptr);
    const cl_target_stats *st = nullptr;
    const int rc = cl_contig_targets(ctx, s, e, n, r->thr.data(), (uint32_t)r->thr.size(), &st);
    if (rc != CL_OK) return rc;
    std::vector<cl_target_stats> copy(st, st + n);
    std::vector<cl_target_order> ocopy;
    if (r->order) {
        const cl_target_order *ord = nullptr;
        const int rc2 = cl_contig_target_order(ctx, s, e, n, &ord);
        if (rc2 != CL_OK) return rc2;
        ocopy.assign(ord, ord + n);
    }
    std::lock_guard<std::mutex> g(r->mu);
    r->taken[i] = std::move(copy);
    if (r->order) r->taken_order[i] = std::move(ocopy);
    return CL_OK;
}

int tg_deliver(void *user, size_t i, const char *name)
{
    TargetRun *r = static_cast<TargetRun *>(user);
    const auto cit = r->by_name.find(name);
    if (cit == r->by_name.end()) return CL_OK;
    std::vector<cl_target_stats> st;
    std::vector<cl_target_order> ord;
    {
        std::lock_guard<std::mutex> g(r->mu);
        auto it = r->taken.find(i);
        if (it == r->taken.end()) return CL_ERR_INVALID;
        st = std::move(it->second);
        r->taken.erase(it);
        if (r->order) {
            auto ot = r->taken_order.find(i);
            if (ot == r->taken_order.end() || ot->second.size() != st.size()) return CL_ERR_INVALID;
            ord = std::move(ot->second);
            r->taken_order.erase(ot);
        }
    }
    const char *const *names = nullptr;
    dut_targets_get(r->tg.get(), cit->second, nullptr, nullptr, &names, nullptr);
    const int rc = dut_targets_write_ex(r->f, name, st.data(), r->order ? ord.data() : nullptr, names, st.size(), (uint32_t)r->thr.size(), &r->total);
    if (rc != CL_OK) r->msg = "cannot write " + r->out_path + " (contig " + name + ")";
    return rc;
}

int tg_finish(void *user)
{
    TargetRun *r = static_cast<TargetRun *>(user);
    int rc = dut_targets_write_total_ex(r->f, &r->total, (uint32_t)r->thr.size(), r->order ? 1 : 0);
    if (fclose(r->f) != 0) rc = CL_ERR_INVALID;
    r->f = nullptr;
    if (rc != CL_OK) r->msg = "cannot write " + r->out_path;
    return rc;
}

// ---- GC bias: one contig's record on its way from its device's thread to the two files ----
struct GcRun {
    dut_gc_options o{};
    FILE *fb = nullptr, *fs = nullptr;
    cl_gc_bias total{};
    std::mutex mu;
    std::map<size_t, cl_gc_bias> taken;  // by selected-contig index
    std::string msg;
    ~GcRun() { if (fb) fclose(fb); if (fs) fclose(fs); }
};

int gc_resident(void *, cl_ctx *, size_t, const char *) { return CL_OK; }   // (the record wants the bases: gc_resident_ref)

int gc_resident_ref(void *user, cl_ctx *ctx, size_t i, const char *, const uint8_t *ref, uint64_t ref_len)
{
    GcRun *r = static_cast<GcRun *>(user);
    cl_gc_bias g;
    const int rc = cl_contig_gc_bias(ctx, ref_len ? ref : nullptr, ref_len, r->o.window, r->o.max_invalid, &g);
    if (rc != CL_OK) return rc;
    std::lock_guard<std::mutex> lk(r->mu);
    r->taken[i] = g;
    return CL_OK;
}

int gc_deliver(void *user, size_t i, const char *name)
{
    GcRun *r = static_cast<GcRun *>(user);
    cl_gc_bias g;
    {
        std::lock_guard<std::mutex> lk(r->mu);
        auto it = r->taken.find(i);
        if (it == r->taken.end()) return CL_ERR_INVALID;
        g = it->second;
        r->taken.erase(it);
    }
    int rc = dut_gc_bias_add(&r->total, &g);
    if (rc == CL_OK && r->fb) rc = dut_gc_bias_write(r->fb, name, &g);
    if (rc == CL_OK && r->fs) rc = dut_gc_summary_write(r->fs, name, &g);
    if (rc != CL_OK) r->msg = std::string("cannot write the GC bias files (contig ") + name + ")";
    return rc;
}

int gc_finish(void *user)
{
    GcRun *r = static_cast<GcRun *>(user);
    // (no contig: the total still says which window it would have had)
    if (r->total.window == 0) { r->total.window = r->o.window; r->total.max_invalid = r->o.max_invalid; }
    int rc = CL_OK;
    if (r->fb) { rc = dut_gc_bias_write(r->fb, "total", &r->total); if (fclose(r->fb) != 0) rc = CL_ERR_INVALID; r->fb = nullptr; }
    if (r->fs) { const int r2 = dut_gc_summary_write(r->fs, "total", &r->total); if (rc == CL_OK) rc = r2; if (fclose(r->fs) != 0) rc = CL_ERR_INVALID; r->fs = nullptr; }
    if (rc != CL_OK) r->msg = "cannot write the GC bias files";
    return rc;
}

// several users behind one hook, called in the order of the list
struct Many { std::vector<dut::ContigHook> hooks; };
int many_header(void *user, const char *const *refs, size_t n_refs)
{
    for (const dut::ContigHook &h : static_cast<Many *>(user)->hooks)
        if (h.header) { const int rc = h.header(h.user, refs, n_refs); if (rc != CL_OK) return rc; }
    return CL_OK;
}
int many_resident(void *user, cl_ctx *ctx, size_t i, const char *name)
{
    for (const dut::ContigHook &h : static_cast<Many *>(user)->hooks) { const int rc = h.resident(h.user, ctx, i, name); if (rc != CL_OK) return rc; }
    return CL_OK;
}
int many_resident_ref(void *user, cl_ctx *ctx, size_t i, const char *name, const uint8_t *ref, uint64_t ref_len)
{
    for (const dut::ContigHook &h : static_cast<Many *>(user)->hooks)
        if (h.resident_ref) { const int rc = h.resident_ref(h.user, ctx, i, name, ref, ref_len); if (rc != CL_OK) return rc; }
    return CL_OK;
}
int many_deliver(void *user, size_t i, const char *name)
{
    for (const dut::ContigHook &h : static_cast<Many *>(user)->hooks) { const int rc = h.deliver(h.user, i, name); if (rc != CL_OK) return rc; }
    return CL_OK;
}
int many_finish(void *user)
{
    int rc = CL_OK;
    for (const dut::ContigHook &h : static_cast<Many *>(user)->hooks) { const int r1 = h.finish(h.user); if (rc == CL_OK) rc = r1; }   // (every file is closed either way)
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

int check_target_options(const dut_target_options *o, char *err, size_t err_len)
{
    const char *m = nullptr;
    if (!o->out_path) m = "targets: no output file for the table";
    else if (o->n_thresholds > CL_TARGET_MAX_THRESHOLDS) m = "targets: more than 8 thresholds";
    else if (o->n_thresholds && !o->thresholds) m = "targets: null thresholds";
    else if (o->n_thresholds && o->thresholds[0] == 0u) m = "targets: the first threshold is 0";
    for (uint32_t i = 1; !m && i < o->n_thresholds; ++i) if (o->thresholds[i] <= o->thresholds[i - 1]) m = "targets: the thresholds are not strictly ascending";
    if (m) { set_err(err, err_len, m); return CL_ERR_INVALID; }
    return CL_OK;
}

int check_gc_options(const dut_gc_options *o, char *err, size_t err_len)
{
    const char *m = nullptr;
    if (o->window < 1 || o->window > CL_GC_MAX_WINDOW) m = "GC bias: the window must be 1 to 1024 positions";
    else if (o->max_invalid >= o->window) m = "GC bias: the number of invalid bases allowed must be below the window";
    if (m) { set_err(err, err_len, m); return CL_ERR_INVALID; }
    return CL_OK;
}

} // namespace

extern "C" int dut_coverage_files_ex(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                                     const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                                     const int *devices, size_t n_devices, unsigned flags, const dut_depth_options *depth,
                                     char *err, size_t err_len)
{
    return dut_coverage_files_ex3(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, depth, nullptr, nullptr, err, err_len);
}

extern "C" int dut_coverage_files_ex2(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                                      const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                                      const int *devices, size_t n_devices, unsigned flags, const dut_depth_options *depth,
                                      const dut_depth_bed_options *bed, char *err, size_t err_len)
{
    return dut_coverage_files_ex3(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, depth, bed, nullptr, err, err_len);
}

extern "C" int dut_coverage_files_ex3(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                                      const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                                      const int *devices, size_t n_devices, unsigned flags, const dut_depth_options *depth,
                                      const dut_depth_bed_options *bed, const dut_target_options *targets, char *err, size_t err_len)
{
    return dut_coverage_files_ex4(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, depth, bed, targets, 0u, err, err_len);
}

extern "C" int dut_coverage_files_ex4(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                                      const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                                      const int *devices, size_t n_devices, unsigned flags, const dut_depth_options *depth,
                                      const dut_depth_bed_options *bed, const dut_target_options *targets, unsigned target_flags,
                                      char *err, size_t err_len)
{
    return dut_coverage_files_ex5(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, depth, bed, targets, target_flags, nullptr, err, err_len);
}

extern "C" int dut_coverage_files_ex5(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                                      const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                                      const int *devices, size_t n_devices, unsigned flags, const dut_depth_options *depth,
                                      const dut_depth_bed_options *bed, const dut_target_options *targets, unsigned target_flags,
                                      const dut_gc_options *gc, char *err, size_t err_len)
{
    if (target_flags & ~DUT_TARGETS_ORDER) { set_err(err, err_len, "targets: unknown target flags"); return CL_ERR_INVALID; }
    if ((target_flags & DUT_TARGETS_ORDER) && !(targets && targets->bed_path)) { set_err(err, err_len, "targets: the quantile columns (DUT_TARGETS_ORDER) need a BED of regions"); return CL_ERR_INVALID; }
    const bool any = depth && (depth->dist_path || depth->windows_path || depth->summary_path);
    const bool any_bed = bed && bed->path;
    const bool any_tg = targets && targets->bed_path;
    const bool any_gc = gc && (gc->bias_path || gc->summary_path);
    if (!any && !any_bed && !any_tg && !any_gc)
        return dut_coverage_files_multi(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, err, err_len);
    if (any && check_options(depth, err, err_len) != CL_OK) return CL_ERR_INVALID;
    if (any_bed && check_bed_options(bed, err, err_len) != CL_OK) return CL_ERR_INVALID;
    // the byte forms have neither (cl_contig_depth_profile, cl_contig_depth_runs): said before anything is read
    if (any_tg && check_target_options(targets, err, err_len) != CL_OK) return CL_ERR_INVALID;
    if (any_gc && check_gc_options(gc, err, err_len) != CL_OK) return CL_ERR_INVALID;
    { const char *qf = getenv("DUT_QUAL_FORM"); if (qf && strcmp(qf, "bytes") == 0) { set_err(err, err_len, any ? "depth profile: pass-bit form only (DUT_QUAL_FORM=bytes is set)" : any_bed ? "depth BED: pass-bit form only (DUT_QUAL_FORM=bytes is set)" : any_tg ? "targets: pass-bit form only (DUT_QUAL_FORM=bytes is set)" : "GC bias: pass-bit form only (DUT_QUAL_FORM=bytes is set)"); return CL_ERR_INVALID; } }
    try {
        DepthRun run;
        BedRun brun;
        TargetRun trun;
        GcRun grun;
        if (any_tg) {
            // (the regions are read before any output is created: a malformed BED leaves nothing behind)
            trun.bed_path = targets->bed_path; trun.out_path = targets->out_path;
            trun.order = (target_flags & DUT_TARGETS_ORDER) != 0u;
            trun.thr.assign(targets->thresholds, targets->thresholds + targets->n_thresholds);
            char e[512] = {0};
            trun.tg.reset(dut_targets_read(targets->bed_path, e, sizeof(e)));
            if (!trun.tg) { set_err(err, err_len, e); return CL_ERR_INVALID; }
            for (size_t c = 0; c < dut_targets_n_contigs(trun.tg.get()); ++c) trun.by_name[dut_targets_contig(trun.tg.get(), c, nullptr)] = c;
        }
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
        if (any_tg) {
            trun.f = fopen(targets->out_path, "wb");
            if (!trun.f || dut_targets_write_header_ex(trun.f, trun.thr.data(), (uint32_t)trun.thr.size(), trun.order ? 1 : 0) != CL_OK) { set_err(err, err_len, ("cannot create " + trun.out_path).c_str()); return CL_ERR_INVALID; }
        }
        if (any_gc) {
            grun.o = *gc;
            if (gc->bias_path && (!(grun.fb = fopen(gc->bias_path, "wb")) || dut_gc_bias_write_header(grun.fb) != CL_OK)) { set_err(err, err_len, (std::string("cannot create ") + gc->bias_path).c_str()); return CL_ERR_INVALID; }
            if (gc->summary_path && (!(grun.fs = fopen(gc->summary_path, "wb")) || dut_gc_summary_write_header(grun.fs) != CL_OK)) { set_err(err, err_len, (std::string("cannot create ") + gc->summary_path).c_str()); return CL_ERR_INVALID; }
        }
        Many many;
        if (any) many.hooks.push_back(dut::ContigHook{nullptr, on_resident, on_deliver, on_finish, &run});
        if (any_bed) many.hooks.push_back(dut::ContigHook{nullptr, bed_resident, bed_deliver, bed_finish, &brun});
        if (any_tg) many.hooks.push_back(dut::ContigHook{tg_header, tg_resident, tg_deliver, tg_finish, &trun});
        if (any_gc) many.hooks.push_back(dut::ContigHook{nullptr, gc_resident, gc_deliver, gc_finish, &grun, gc_resident_ref});
        const dut::ContigHook hook = {many_header, many_resident, many_deliver, many_finish, &many, any_gc ? many_resident_ref : nullptr};
        const int rc = dut::coverage_files_hooked(bam_path, fasta_path, bed_path, summary_json, summary_html, opt, contigs, n_contigs, devices, n_devices, flags, err, err_len, &hook);
        // the failure was this file's: its own words
        if (rc != CL_OK && !run.msg.empty()) set_err(err, err_len, run.msg.c_str());
        else if (rc != CL_OK && !brun.msg.empty()) set_err(err, err_len, brun.msg.c_str());
        else if (rc != CL_OK && !trun.msg.empty()) set_err(err, err_len, trun.msg.c_str());
        else if (rc != CL_OK && !grun.msg.empty()) set_err(err, err_len, grun.msg.c_str());
        return rc;
    } catch (...) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_NOMEM; }
}
