// coverage_hook.h -- the seam between the file-level coverage driver (coverage_files.cpp) and what a caller wants of a
// contig beyond its runs, while it is resident on the device (depth_files.cpp: the depth profile, the depth BED, the
// per-target table).  The driver itself
// calls nothing of the engine that its existing entry points did not call; they pass no hook.
#pragma once
#include "../../include/dut_bam.h"

namespace dut {

struct ContigHook {
    // once, on the calling thread, with the names of all contigs of the BAM header, before any device is opened (may be
    // null).  A negative cl_status ends the analysis before it starts.
    int (*header)(void *user, const char *const *ref_names, size_t n_refs);
    // on the device's host thread, right after selected contig i (index in tid order) has been run and collected on ctx
    // and before the next contig replaces it.  A negative cl_status ends the analysis (message: cl_last_error(ctx)).
    int (*resident)(void *user, cl_ctx *ctx, size_t i, const char *contig_name);
    // on the calling thread, in tid order, after contig i's BED lines are written (one device or several)
    int (*deliver)(void *user, size_t i, const char *contig_name);
    // once, after the last contig of a run without error, before the summaries are written and the outputs are closed
    int (*finish)(void *user);
    void *user;
    // as `resident` and right behind it, with the contig's reference bases as the driver holds them (ref_len may differ
    // from the contig's length; null and 0 for a contig without bases).  May be null; the last member, so that a hook
    // that lists the five above leaves it so.
    int (*resident_ref)(void *user, cl_ctx *ctx, size_t i, const char *contig_name, const uint8_t *ref, uint64_t ref_len);
};

// dut_coverage_files_multi with a hook (null: exactly that call)
int coverage_files_hooked(const char *bam_path, const char *fasta_path, const char *bed_path, const char *summary_json,
                          const char *summary_html, const cl_options *opt, const char *const *contigs, size_t n_contigs,
                          const int *devices, size_t n_devices, unsigned flags, char *err, size_t err_len, const ContigHook *hook);

} // namespace dut
