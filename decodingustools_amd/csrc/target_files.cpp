// target_files.cpp -- the host side of the per-target summaries (include/dut_coverage.h): the reader of a BED of regions,
// the threshold list of `--target-thresholds`, and the table of cl_contig_targets' records, with the columns of
// cl_contig_target_order's behind them when asked.  Plain C++, no device.
#include "../../include/dut_coverage.h"

#include <cerrno>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

struct dut_targets {
    struct Contig {
        std::string name;
        std::vector<uint32_t> starts, ends, lines;
        std::vector<std::string> names;
        std::vector<const char *> name_ptrs;
    };
    std::vector<Contig> contigs;
};

namespace {

void set_err(char *err, size_t n, const std::string &m) { if (err && n) snprintf(err, n, "%s", m.c_str()); }

// a whole number of decimal digits only, at most 2^32 - 1
bool parse_u32(const char *b, const char *e, uint32_t *out)
{
    if (b == e) return false;
    uint64_t v = 0;
    for (const char *p = b; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10 + (uint64_t)(*p - '0');
        if (v > 0xFFFFFFFFull) return false;
    }
    *out = (uint32_t)v;
    return true;
}

bool starts_with(const char *b, const char *e, const char *word)
{
    const size_t n = strlen(word);
    return (size_t)(e - b) >= n && memcmp(b, word, n) == 0;
}

} // namespace

extern "C" dut_targets *dut_targets_parse(const char *text, size_t len, char *err, size_t err_len)
{
    try {
        std::unique_ptr<dut_targets> t(new dut_targets);
        std::map<std::string, size_t> index;
        const char *p = text, *end = text ? text + len : nullptr;
        uint32_t line = 0;
        while (p && p < end) {
            const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
            const char *b = p, *e = nl ? nl : end;
            p = nl ? nl + 1 : end;
            ++line;
            if (e > b && e[-1] == '\r') --e;
            const char *q = b;
            while (q < e && (*q == ' ' || *q == '\t')) ++q;
            if (q == e || *b == '#' || starts_with(b, e, "track") || starts_with(b, e, "browser")) continue;
            // the columns: tab or blank separated
            const char *col[4][2];
            int nc = 0;
            q = b;
            while (q < e && nc < 4) {
                while (q < e && (*q == ' ' || *q == '\t')) ++q;
                if (q == e) break;
                col[nc][0] = q;
                while (q < e && *q != ' ' && *q != '\t') ++q;
                col[nc][1] = q;
                ++nc;
            }
            const std::string where = "line " + std::to_string(line) + ": ";
            if (nc < 3) { set_err(err, err_len, where + "fewer than 3 columns (contig, start, end)"); return nullptr; }
            uint32_t s = 0, en = 0;
            if (!parse_u32(col[1][0], col[1][1], &s)) { set_err(err, err_len, where + "malformed start '" + std::string(col[1][0], col[1][1]) + "'"); return nullptr; }
            if (!parse_u32(col[2][0], col[2][1], &en)) { set_err(err, err_len, where + "malformed end '" + std::string(col[2][0], col[2][1]) + "'"); return nullptr; }
            if (s > en) { set_err(err, err_len, where + "start " + std::to_string(s) + " > end " + std::to_string(en)); return nullptr; }
            const std::string contig(col[0][0], col[0][1]);
            auto it = index.find(contig);
            if (it == index.end()) {
                it = index.emplace(contig, t->contigs.size()).first;
                t->contigs.emplace_back();
                t->contigs.back().name = contig;
            }
            dut_targets::Contig &c = t->contigs[it->second];
            c.starts.push_back(s); c.ends.push_back(en); c.lines.push_back(line);
            c.names.push_back(nc >= 4 ? std::string(col[3][0], col[3][1]) : std::string("."));
        }
        for (dut_targets::Contig &c : t->contigs)
            for (const std::string &n : c.names) c.name_ptrs.push_back(n.c_str());
        return t.release();
    } catch (...) { set_err(err, err_len, "out of memory"); return nullptr; }
}

extern "C" dut_targets *dut_targets_read(const char *path, char *err, size_t err_len)
{
    try {
        FILE *f = path ? fopen(path, "rb") : nullptr;
        if (!f) { set_err(err, err_len, std::string("cannot read ") + (path ? path : "(null)")); return nullptr; }
        std::string text;
        char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) { set_err(err, err_len, std::string("cannot read ") + path); return nullptr; }
        char e[400] = {0};
        dut_targets *t = dut_targets_parse(text.data(), text.size(), e, sizeof(e));
        if (!t) set_err(err, err_len, std::string(path) + ": " + e);
        return t;
    } catch (...) { set_err(err, err_len, "out of memory"); return nullptr; }
}

extern "C" void dut_targets_free(dut_targets *t) { delete t; }
extern "C" size_t dut_targets_n_contigs(const dut_targets *t) { return t ? t->contigs.size() : 0; }

extern "C" const char *dut_targets_contig(const dut_targets *t, size_t c, size_t *n_targets)
{
    if (!t || c >= t->contigs.size()) return nullptr;
    if (n_targets) *n_targets = t->contigs[c].starts.size();
    return t->contigs[c].name.c_str();
}

extern "C" int dut_targets_get(const dut_targets *t, size_t c, const uint32_t **starts, const uint32_t **ends,
                               const char *const **names, const uint32_t **lines)
{
    if (!t || c >= t->contigs.size()) return CL_ERR_INVALID;
    const dut_targets::Contig &k = t->contigs[c];
    if (starts) *starts = k.starts.data();
    if (ends) *ends = k.ends.data();
    if (names) *names = k.name_ptrs.data();
    if (lines) *lines = k.lines.data();
    return CL_OK;
}

extern "C" int dut_thresholds_parse(const char *spec, uint32_t *thresholds, uint32_t *n_thresholds, char *err, size_t err_len)
{
    if (!thresholds || !n_thresholds) return CL_ERR_INVALID;
    *n_thresholds = 0;
    if (!spec || !*spec) spec = "1,10,20,30";
    const char *p = spec;
    for (;;) {
        const char *e = strchr(p, ',');
        if (!e) e = p + strlen(p);
        uint32_t v = 0;
        if (!parse_u32(p, e, &v)) { set_err(err, err_len, "target thresholds: '" + std::string(p, e) + "' is not a whole number below 2^32"); return CL_ERR_INVALID; }
        if (*n_thresholds == CL_TARGET_MAX_THRESHOLDS) { set_err(err, err_len, "target thresholds: more than 8"); return CL_ERR_INVALID; }
        if (*n_thresholds == 0 && v == 0) { set_err(err, err_len, "target thresholds: the first is 0"); return CL_ERR_INVALID; }
        if (*n_thresholds && v <= thresholds[*n_thresholds - 1]) { set_err(err, err_len, "target thresholds: not strictly ascending"); return CL_ERR_INVALID; }
        thresholds[(*n_thresholds)++] = v;
        if (!*e) break;
        p = e + 1;
    }
    return CL_OK;
}

extern "C" int dut_targets_write_header(FILE *f, const uint32_t *thresholds, uint32_t n_thresholds)
{
    return dut_targets_write_header_ex(f, thresholds, n_thresholds, 0);
}

extern "C" int dut_targets_write_header_ex(FILE *f, const uint32_t *thresholds, uint32_t n_thresholds, int order_columns)
{
    if (!f || n_thresholds > CL_TARGET_MAX_THRESHOLDS || (n_thresholds && !thresholds)) return CL_ERR_INVALID;
    bool ok = fputs("#contig\tstart\tend\tname\tlength\tmean_raw\tmean_qc\tcallable\tcallable_frac\tref_n\tno_coverage\tlow_coverage\t"
                    "excessive_coverage\tpoor_mapping_quality", f) >= 0;
    for (uint32_t k = 0; ok && k < n_thresholds; ++k) ok = fprintf(f, "\traw_ge_%" PRIu32, thresholds[k]) > 0;
    for (uint32_t k = 0; ok && k < n_thresholds; ++k) ok = fprintf(f, "\tqc_ge_%" PRIu32, thresholds[k]) > 0;
    if (order_columns) ok = ok && fputs("\traw_min\traw_q1\traw_median\traw_q3\traw_max\tqc_min\tqc_q1\tqc_median\tqc_q3\tqc_max", f) >= 0;
    ok = ok && fputc('\n', f) != EOF;
    return ok ? CL_OK : CL_ERR_INVALID;
}

namespace {

// the columns behind the name: the same for a target and for the total; with order_columns the ten order statistics
// behind them (ord: a target of some length's raw[5], qc[5]; NULL: `NA`, quantiles do not add)
bool write_figures(FILE *f, uint64_t len, uint64_t sum_raw, uint64_t sum_qc, const uint64_t state[6], const uint64_t *ge_raw,
                   const uint64_t *ge_qc, uint32_t K, bool order_columns, const uint32_t *ord)
{
    bool ok = fprintf(f, "\t%" PRIu64, len) > 0;
    if (len) ok = ok && fprintf(f, "\t%.4f\t%.4f", (double)sum_raw / (double)len, (double)sum_qc / (double)len) > 0;
    else ok = ok && fputs("\tNA\tNA", f) >= 0;
    ok = ok && fprintf(f, "\t%" PRIu64, state[CL_CALLABLE]) > 0;
    if (len) ok = ok && fprintf(f, "\t%.6f", (double)state[CL_CALLABLE] / (double)len) > 0;
    else ok = ok && fputs("\tNA", f) >= 0;
    ok = ok && fprintf(f, "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64, state[CL_REF_N], state[CL_NO_COVERAGE],
                       state[CL_LOW_COVERAGE], state[CL_EXCESSIVE_COVERAGE], state[CL_POOR_MAPPING_QUALITY]) > 0;
    for (uint32_t k = 0; ok && k < K; ++k) ok = fprintf(f, "\t%" PRIu64, ge_raw[k]) > 0;
    for (uint32_t k = 0; ok && k < K; ++k) ok = fprintf(f, "\t%" PRIu64, ge_qc[k]) > 0;
    for (int k = 0; ok && order_columns && k < 10; ++k) ok = ord ? fprintf(f, "\t%" PRIu32, ord[k]) > 0 : fputs("\tNA", f) >= 0;
    return ok && fputc('\n', f) != EOF;
}

} // namespace

extern "C" int dut_targets_write(FILE *f, const char *contig, const cl_target_stats *stats, const char *const *names, size_t n,
                                 uint32_t n_thresholds, dut_target_total *total)
{
    return dut_targets_write_ex(f, contig, stats, nullptr, names, n, n_thresholds, total);
}

extern "C" int dut_targets_write_ex(FILE *f, const char *contig, const cl_target_stats *stats, const cl_target_order *order,
                                    const char *const *names, size_t n, uint32_t n_thresholds, dut_target_total *total)
{
    if (!f || !contig || (n && !stats) || n_thresholds > CL_TARGET_MAX_THRESHOLDS) return CL_ERR_INVALID;
    for (size_t i = 0; i < n; ++i) {
        const cl_target_stats &s = stats[i];
        uint64_t st[6], gr[CL_TARGET_MAX_THRESHOLDS], gq[CL_TARGET_MAX_THRESHOLDS];
        for (int j = 0; j < 6; ++j) st[j] = s.state[j];
        for (uint32_t k = 0; k < CL_TARGET_MAX_THRESHOLDS; ++k) { gr[k] = s.ge_raw[k]; gq[k] = s.ge_qc[k]; }
        if (fprintf(f, "%s\t%" PRIu32 "\t%" PRIu32 "\t%s", contig, s.start, s.end, names && names[i] ? names[i] : ".") <= 0) return CL_ERR_INVALID;
        uint32_t ord[10];
        if (order) {
            // (both records are of the same target)
            if (order[i].start != s.start || order[i].end != s.end) return CL_ERR_INVALID;
            for (int k = 0; k < 5; ++k) { ord[k] = order[i].raw[k]; ord[5 + k] = order[i].qc[k]; }
        }
        if (!write_figures(f, s.len, s.sum_raw, s.sum_qc, st, gr, gq, n_thresholds, order != nullptr, order && s.len ? ord : nullptr)) return CL_ERR_INVALID;
        if (total) {
            total->n_targets += 1; total->len += s.len; total->sum_raw += s.sum_raw; total->sum_qc += s.sum_qc;
            for (int j = 0; j < 6; ++j) total->state[j] += st[j];
            for (uint32_t k = 0; k < CL_TARGET_MAX_THRESHOLDS; ++k) { total->ge_raw[k] += gr[k]; total->ge_qc[k] += gq[k]; }
        }
    }
    return CL_OK;
}

extern "C" int dut_targets_write_total(FILE *f, const dut_target_total *t, uint32_t n_thresholds)
{
    return dut_targets_write_total_ex(f, t, n_thresholds, 0);
}

extern "C" int dut_targets_write_total_ex(FILE *f, const dut_target_total *t, uint32_t n_thresholds, int order_columns)
{
    if (!f || !t || n_thresholds > CL_TARGET_MAX_THRESHOLDS) return CL_ERR_INVALID;
    if (fputs("total\t.\t.\t.", f) < 0) return CL_ERR_INVALID;
    return write_figures(f, t->len, t->sum_raw, t->sum_qc, t->state, t->ge_raw, t->ge_qc, n_thresholds, order_columns != 0, nullptr) ? CL_OK : CL_ERR_INVALID;
}
