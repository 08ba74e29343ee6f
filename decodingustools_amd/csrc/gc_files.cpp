// gc_files.cpp -- the host layer of the GC-bias profile (include/dut_coverage.h): records of cl_contig_gc_bias added up,
// their statistics in f64 and the two text files.  No device; the operation order is the header's, and tests/gc_ref.py
// restates it.
#include "../../include/dut_coverage.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

namespace {

// a / b in f64, or DUT_GC_NA without a denominator
double quot(uint64_t a, uint64_t b) { return b ? (double)a / (double)b : DUT_GC_NA; }

// 100 * sum over [b0, b1) of max(0, positions[b] / P - sum[b] / S)
double dropout(const uint64_t *positions, const uint64_t *sum, uint64_t P, uint64_t S, int b0, int b1)
{
    if (!P || !S) return DUT_GC_NA;
    double acc = 0.0;
    for (int b = b0; b < b1; ++b) {
        const double d = (double)positions[b] / (double)P - (double)sum[b] / (double)S;
        if (d > 0.0) acc += d;
    }
    return 100.0 * acc;
}

bool put(FILE *f, const char *fmt, double v)
{
    return (v < 0.0 ? fputs("NA", f) : fprintf(f, fmt, v)) >= 0;
}

} // namespace

extern "C" int dut_gc_bias_add(cl_gc_bias *total, const cl_gc_bias *part)
{
    if (!total || !part) return CL_ERR_INVALID;
    if (total->window == 0) { total->window = part->window; total->max_invalid = part->max_invalid; }
    else if (total->window != part->window || total->max_invalid != part->max_invalid) return CL_ERR_INVALID;
    const uint64_t e = (uint64_t)total->extent + part->extent;
    total->extent = e > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)e;
    total->n_skipped += part->n_skipped;
    for (int b = 0; b < CL_GC_BINS; ++b) {
        total->positions[b] += part->positions[b]; total->sum_raw[b] += part->sum_raw[b];
        total->sum_qc[b] += part->sum_qc[b]; total->zero_raw[b] += part->zero_raw[b];
    }
    return CL_OK;
}

extern "C" int dut_gc_bias_stats(const cl_gc_bias *g, dut_gc_stats *out)
{
    if (!g || !out) return CL_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    uint64_t P = 0, Sr = 0, Sq = 0;
    for (int b = 0; b < CL_GC_BINS; ++b) { P += g->positions[b]; Sr += g->sum_raw[b]; Sq += g->sum_qc[b]; }
    out->positions = P; out->sum_raw = Sr; out->sum_qc = Sq;
    out->total_mean_raw = quot(Sr, P); out->total_mean_qc = quot(Sq, P);
    for (int b = 0; b < CL_GC_BINS; ++b) {
        const uint64_t n = g->positions[b];
        out->mean_raw[b] = quot(g->sum_raw[b], n); out->mean_qc[b] = quot(g->sum_qc[b], n);
        out->zero_frac[b] = quot(g->zero_raw[b], n);
        out->norm_raw[b] = n && Sr ? out->mean_raw[b] / out->total_mean_raw : DUT_GC_NA;   // (n > 0: P > 0 too)
        out->norm_qc[b] = n && Sq ? out->mean_qc[b] / out->total_mean_qc : DUT_GC_NA;
    }
    out->at_dropout_raw = dropout(g->positions, g->sum_raw, P, Sr, 0, 51);
    out->gc_dropout_raw = dropout(g->positions, g->sum_raw, P, Sr, 51, CL_GC_BINS);
    out->at_dropout_qc = dropout(g->positions, g->sum_qc, P, Sq, 0, 51);
    out->gc_dropout_qc = dropout(g->positions, g->sum_qc, P, Sq, 51, CL_GC_BINS);
    return CL_OK;
}

extern "C" int dut_gc_bias_write_header(FILE *f)
{
    if (!f) return CL_ERR_INVALID;
    return fputs("#contig\tgc\tpositions\tmean_raw\tmean_qc\tnorm_raw\tnorm_qc\tzero_frac\n", f) >= 0 ? CL_OK : CL_ERR_INVALID;
}

extern "C" int dut_gc_bias_write(FILE *f, const char *contig, const cl_gc_bias *g)
{
    dut_gc_stats s;
    if (!f || !contig || dut_gc_bias_stats(g, &s) != CL_OK) return CL_ERR_INVALID;
    for (int b = 0; b < CL_GC_BINS; ++b) {
        if (!g->positions[b]) continue;
        bool ok = fprintf(f, "%s\t%d\t%llu\t", contig, b, (unsigned long long)g->positions[b]) >= 0;
        ok = ok && put(f, "%.4f", s.mean_raw[b]) && fputc('\t', f) != EOF && put(f, "%.4f", s.mean_qc[b]) && fputc('\t', f) != EOF;
        ok = ok && put(f, "%.6f", s.norm_raw[b]) && fputc('\t', f) != EOF && put(f, "%.6f", s.norm_qc[b]) && fputc('\t', f) != EOF;
        ok = ok && put(f, "%.6f", s.zero_frac[b]) && fputc('\n', f) != EOF;
        if (!ok) return CL_ERR_INVALID;
    }
    return CL_OK;
}

extern "C" int dut_gc_summary_write_header(FILE *f)
{
    if (!f) return CL_ERR_INVALID;
    return fputs("#contig\twindow\tmax_invalid\tpositions\tskipped\tmean_raw\tmean_qc\tat_dropout_raw\tgc_dropout_raw\tat_dropout_qc\tgc_dropout_qc\n", f) >= 0
               ? CL_OK : CL_ERR_INVALID;
}

extern "C" int dut_gc_summary_write(FILE *f, const char *contig, const cl_gc_bias *g)
{
    dut_gc_stats s;
    if (!f || !contig || dut_gc_bias_stats(g, &s) != CL_OK) return CL_ERR_INVALID;
    bool ok = fprintf(f, "%s\t%u\t%u\t%llu\t%llu\t", contig, g->window, g->max_invalid, (unsigned long long)s.positions, (unsigned long long)g->n_skipped) >= 0;
    ok = ok && put(f, "%.4f", s.total_mean_raw) && fputc('\t', f) != EOF && put(f, "%.4f", s.total_mean_qc);
    for (const double d : {s.at_dropout_raw, s.gc_dropout_raw, s.at_dropout_qc, s.gc_dropout_qc}) ok = ok && fputc('\t', f) != EOF && put(f, "%.6f", d);
    ok = ok && fputc('\n', f) != EOF;
    return ok ? CL_OK : CL_ERR_INVALID;
}
