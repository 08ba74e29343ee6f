// variants.cpp -- implementation of include/dut_variants.h: the per-position classification in plain C++ (the f64 rule
// the device's integer test is held against), the annotation of candidates against a haplogroup tree, the TSV of
// `find-variants`; the second-allele rule of `find-minor-alleles` in plain C++, its fraction parser and its TSV.  Host-only
// except dut_find_variants_files(_ex) and dut_find_minor_files, which run the device engine's cl_site_scan(_ex) and
// cl_site_scan_minor.  The same for `find-deletions`: the deletion rule, the merge of candidate positions into events,
// the TSV, and dut_find_deletions_files over cl_site_scan_dels.  And for `find-insertions`: the insertion rule, the
// grouping of observations into alleles, the TSV, and dut_find_insertions_files over cl_site_scan_ins.  And for `consensus`:
// the composed rule, the assembly of the bytes of cl_site_scan_consensus and the insertions into a sequence and a change
// list, the FASTA and the change list's file, and dut_find_consensus_files over both scans on one resident tile.  And for
// `find-strs`: the host route of cl_site_str_lengths over str_walk.h (dut_str_measure), the rule that turns a length
// histogram into an allele, the unit notation, the loci file's parser, the TSV, and dut_find_strs_files.  And for
// `error-profile`: the host route of cl_site_error_profile over ep_walk.h (dut_error_profile_measure), the TSV, and
// dut_error_profile_files.  And for `phase-sites`: the host route of cl_site_link_counts over link_walk.h
// (dut_link_measure), the integer rule that names a pair cis or trans, the sites file's parser, the TSV, and
// dut_find_links_files.
#include "../../include/dut_variants.h"
#include "../../include/dut_report.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>
#include "host_parallel.h"
#include "str_walk.h"
#include "ep_walk.h"
#include "link_walk.h"

namespace {

void set_err(char *err, size_t n, const std::string &m)
{
    if (err && n) snprintf(err, n, "%s", m.c_str());
}

const char CODE[] = "=ACMGRSVTWYHKDBN";                    // rust-htslib seq().as_bytes()

// ref[p] upper-cased if that is one of ACGT, else 0 ("other")
char ref_base(uint8_t b)
{
    const char u = (char)(b & ~32u);
    return (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? u : 0;
}

int classify_call(char called, uint8_t ref_byte)
{
    const char rb = ref_base(ref_byte);
    if (!(called == 'A' || called == 'C' || called == 'G' || called == 'T') || !rb) return DUT_SCAN_UNCOMPARABLE;
    return called == rb ? DUT_SCAN_MATCH : DUT_SCAN_VARIANT;
}

char *dup(const std::string &s)
{
    char *p = (char *)malloc(s.size() + 1);
    if (p) memcpy(p, s.c_str(), s.size() + 1);
    return p;
}

template <class Cand>
int annotate(const dut_tree *t, const char *build_id, const char *chromosome, const Cand *candidates, size_t n, dut_variant_note **notes)
{
    if (!t || !build_id || !chromosome || (n && !candidates) || !notes) return CL_ERR_INVALID;
    dut_tree_locus *lp = nullptr; size_t nl = 0;
    const int rc = dut_tree_collect_loci(t, build_id, chromosome, &lp, &nl);
    if (rc != CL_OK) return rc;
    std::unique_ptr<dut_tree_locus, decltype(&free)> loci(lp, free);
    dut_variant_note *o = (dut_variant_note *)calloc(std::max<size_t>(n, 1), sizeof(dut_variant_note));
    if (!o) return CL_ERR_NOMEM;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t pos = candidates[i].pos;
        const dut_tree_locus *b = std::lower_bound(lp, lp + nl, pos, [](const dut_tree_locus &l, uint32_t p) { return l.position < p; });
        if (b == lp + nl || b->position != pos) continue;                     // novel
        std::string names, alleles;
        for (; b != lp + nl && b->position == pos; ++b) {
            if (!names.empty()) { names += ","; alleles += ","; }
            names += b->name;
            const char alt = (char)candidates[i].alt;
            alleles += (b->derived[0] && b->derived[0] == alt) ? "derived" : (b->ancestral[0] && b->ancestral[0] == alt) ? "ancestral" : "other";
        }
        o[i].known = 1; o[i].names = dup(names); o[i].alleles = dup(alleles);
        if (!o[i].names || !o[i].alleles) { dut_variants_free_notes(o, n); return CL_ERR_NOMEM; }
    }
    *notes = o;
    return CL_OK;
}

int write_file(const char *path, const std::string &s, char *err, size_t err_len)
{
    FILE *f = fopen(path, "wb");
    if (!f) { set_err(err, err_len, std::string("cannot create ") + path); return CL_ERR_INVALID; }
    const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
    if (fclose(f) != 0 || !ok) { set_err(err, err_len, std::string("cannot write ") + path); return CL_ERR_INVALID; }
    return CL_OK;
}

// A rule of a count and parts per 10 000 (the second allele, the deletion, the insertion): its names in messages and TSV lines and the
// largest per-10k value
struct Rule { const char *count, *per_10k, *fraction; uint32_t max_per_10k; };
const Rule MINOR_RULE = {"min_minor_count", "min_minor_per_10k", "min_minor_fraction", 5000};
const Rule DEL_RULE = {"min_del_count", "min_del_per_10k", "min_del_fraction", 10000};
const Rule INS_RULE = {"min_ins_count", "min_ins_per_10k", "min_ins_fraction", 10000};

// what a file-level scan is asked with: the flag and base-quality filter, and a rule's own values -- dut_minor_options,
// dut_del_options and dut_ins_options member by member
struct FilterOptions { int has_min_base_quality; uint8_t min_base_quality; uint16_t exclude_flags; };
struct ScanOptions { uint32_t min_depth; uint8_t min_quality; FilterOptions flt; uint32_t per_10k, count, per_strand; };
ScanOptions scan_options(const dut_minor_options &o)
{
    return {o.min_depth, o.min_quality, {o.has_min_base_quality, o.min_base_quality, o.exclude_flags}, o.min_minor_per_10k, o.min_minor_count, o.min_minor_per_strand};
}
ScanOptions scan_options(const dut_del_options &o)
{
    return {o.min_depth, o.min_quality, {o.has_min_base_quality, o.min_base_quality, o.exclude_flags}, o.min_del_per_10k, o.min_del_count, o.min_del_per_strand};
}
ScanOptions scan_options(const dut_ins_options &o)
{
    return {o.min_depth, o.min_quality, {o.has_min_base_quality, o.min_base_quality, o.exclude_flags}, o.min_ins_per_10k, o.min_ins_count, o.min_ins_per_strand};
}

// the range checks of a rule, written once
bool rule_ok(const Rule &r, uint32_t min_depth, uint32_t count, uint32_t per_10k, char *err = nullptr, size_t err_len = 0)
{
    char b[96] = {0};
    if (min_depth == 0) snprintf(b, sizeof(b), "min_depth must be at least 1");
    else if (count == 0) snprintf(b, sizeof(b), "%s must be at least 1", r.count);
    else if (per_10k < 1 || per_10k > r.max_per_10k) snprintf(b, sizeof(b), "%s must lie in 1..%u", r.per_10k, r.max_per_10k);
    else return true;
    set_err(err, err_len, b);
    return false;
}

// the comment lines every scan's TSV opens with, down to ##positions; the two filter lines and the two lines of a rule
// where the mode prints them
void tsv_preamble(std::string &s, const char *contig, uint32_t start, uint32_t end, const ScanOptions &o, bool filter_lines, const Rule *rule)
{
    char b[512], q[8] = ".";
    snprintf(b, sizeof(b), "##contig=%s\n##range=%u-%u\n##min_depth=%u\n##min_quality=%u\n", contig, start, end, o.min_depth, (unsigned)o.min_quality);
    s += b;
    if (o.flt.has_min_base_quality) snprintf(q, sizeof(q), "%u", (unsigned)o.flt.min_base_quality);
    snprintf(b, sizeof(b), "##min_base_quality=%s\n##exclude_flags=0x%04x\n", q, (unsigned)o.flt.exclude_flags);
    if (filter_lines) s += b;
    if (rule) { snprintf(b, sizeof(b), "##%s=%.4f\n##%s=%u\n", rule->fraction, (double)o.per_10k / 10000.0, rule->count, o.count); s += b; }
    snprintf(b, sizeof(b), "##positions=%u\n", end - start);
    s += b;
}

// opt: the extended TSV of dut_variants_write_ex (Res = cl_scan_result_ex); nullptr: the one of dut_variants_write
template <class Res>
int write_tsv(const char *path, const char *contig, const Res *res, uint32_t min_depth, uint8_t min_quality,
              const dut_variants_options *opt, const dut_variant_note *notes, char *err, size_t err_len)
{
    if (!path || !contig || !res || (res->n_variant && !res->candidates)) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    std::string s;
    char b[512];
    ScanOptions o = {min_depth, min_quality, {}, 0, 0, 0};
    if (opt) o.flt = {opt->has_min_base_quality, opt->min_base_quality, opt->exclude_flags};
    tsv_preamble(s, contig, res->start, res->end, o, opt != nullptr, nullptr);
    snprintf(b, sizeof(b), "##low_depth=%llu\n##mixed=%llu\n##uncomparable=%llu\n##match=%llu\n##variant=%llu\n",
             (unsigned long long)res->n_low_depth, (unsigned long long)res->n_mixed, (unsigned long long)res->n_uncomparable,
             (unsigned long long)res->n_match, (unsigned long long)res->n_variant);
    s += b;
    s += "#contig\tpos\tref\talt\tdepth\tA\tC\tG\tT\tfreq\tstatus\tnames\talleles";
    s += opt ? "\talt_fwd\talt_rev\tref_fwd\tref_rev\tfilter\n" : "\n";
    for (uint64_t i = 0; i < res->n_variant; ++i) {
        const auto &c = res->candidates[i];
        const uint32_t ac = c.alt == 'A' ? c.a : c.alt == 'C' ? c.c : c.alt == 'G' ? c.g : c.t;
        const double freq = c.depth ? (double)ac / (double)c.depth : 0.0;
        snprintf(b, sizeof(b), "\t%u\t%c\t%c\t%u\t%u\t%u\t%u\t%u\t%.4f\t", c.pos, (char)c.ref, (char)c.alt, c.depth, c.a, c.c, c.g, c.t, freq);
        s += contig; s += b;
        if (!notes) s += ".\t.\t.";
        else if (!notes[i].known) s += "novel\t.\t.";
        else { s += "known\t"; s += notes[i].names ? notes[i].names : "."; s += "\t"; s += notes[i].alleles ? notes[i].alleles : "."; }
        if constexpr (std::is_same<Res, cl_scan_result_ex>::value) {
            const bool strand = std::min(c.alt_fwd, c.alt_rev) < opt->min_alt_per_strand;
            snprintf(b, sizeof(b), "\t%u\t%u\t%u\t%u\t%s", c.alt_fwd, c.alt_rev, c.ref_fwd, c.ref_rev, strand ? "strand" : "PASS");
            s += b;
        }
        s += "\n";
    }
    return write_file(path, s, err, err_len);
}

// What the file-level scans share: the opened files, the contig's records and reference bases, the context with the tile
// resident.  scan_files_open: everything that needs no device and no record; scan_files_upload: the HIP runtime + context
// beside `side` (the caller's own slow start, such as a tree's JSON) and the contig's records, then cl_site_upload.
struct ScanFiles {
    std::unique_ptr<dut_fasta, decltype(&dut_fasta_close)> fa{nullptr, dut_fasta_close};
    std::unique_ptr<dut_bam, decltype(&dut_bam_close)> bam{nullptr, dut_bam_close};
    std::unique_ptr<cl_ctx, decltype(&cl_destroy)> ctx{nullptr, cl_destroy};
    int tid = -1;
    uint32_t contig_len = 0;
    dut_records rec{};
    const uint64_t *seq_off = nullptr; const uint8_t *seq4 = nullptr;
    const uint8_t *bases = nullptr; uint64_t blen = 0;
    void engine_err(char *err, size_t err_len, const char *what) const { const char *m = cl_last_error(ctx.get()); set_err(err, err_len, (m && *m) ? m : what); }
};

int scan_files_open(ScanFiles &F, const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t &start,
                           uint32_t &end, char *err, size_t err_len)
{
    if (has_region && start >= end) { set_err(err, err_len, "the region is empty"); return CL_ERR_INVALID; }
    char e[512] = {0};
    F.fa.reset(dut_fasta_open(fasta_path, e, sizeof(e)));
    if (!F.fa) { set_err(err, err_len, e); return CL_ERR_INVALID; }
    F.bam.reset(dut_bam_open(bam_path, e, sizeof(e)));
    if (!F.bam) { set_err(err, err_len, e); return CL_ERR_INVALID; }
    if (!dut_bam_has_index(F.bam.get())) { set_err(err, err_len, std::string("no .bai or .csi index beside ") + bam_path); return CL_ERR_INVALID; }
    for (int t = 0; t < dut_bam_n_ref(F.bam.get()); ++t) if (strcmp(dut_bam_ref_name(F.bam.get(), t), contig) == 0) { F.tid = t; break; }
    if (F.tid < 0) { set_err(err, err_len, std::string("contig ") + contig + " is not in the BAM header"); return CL_ERR_INVALID; }
    F.contig_len = dut_bam_ref_len(F.bam.get(), F.tid);
    if (!has_region) { start = 0; end = F.contig_len; }
    if (end > F.contig_len) { set_err(err, err_len, "the region ends beyond contig " + std::string(contig) + " (" + std::to_string(F.contig_len) + " bases)"); return CL_ERR_INVALID; }
    return CL_OK;
}

// side(): runs beside the context's creation; side_ok(): its verdict (it sets the message itself), asked after the FASTA's
template <class Side, class SideOk>
int scan_files_upload(ScanFiles &F, const char *contig, int device_id, Side &&side, SideOk &&side_ok, char *err, size_t err_len)
{
    int crc = CL_OK;
    cl_options opt = {4, 500, 10, 20, 10, 1, 0.1};
    dut::Thread tt = dut::spawn_or_run([&]() { side(); });
    dut::Thread ct = dut::spawn_or_run([&]() { cl_ctx *c = nullptr; crc = cl_create(&opt, device_id, nullptr, &c); F.ctx.reset(c); });
    const int brc = dut_bam_read_contig(F.bam.get(), F.tid, &F.rec, &F.seq_off, &F.seq4);
    const int frc = dut_fasta_fetch(F.fa.get(), contig, &F.bases, &F.blen);
    if (tt.joinable()) tt.join();
    if (ct.joinable()) ct.join();
    if (frc != CL_OK) { set_err(err, err_len, dut_fasta_error(F.fa.get())); return frc; }
    if (!side_ok()) return CL_ERR_INVALID;
    if (brc != CL_OK) { set_err(err, err_len, dut_bam_error(F.bam.get())); return brc; }
    if (crc != CL_OK) { set_err(err, err_len, "no usable HIP device (the engine has no CPU fallback)"); return crc; }
    cl_site_tile tile;
    tile.n_reads = F.rec.n; tile.pos = F.rec.pos; tile.mapq = F.rec.mapq; tile.cigar_off = F.rec.cigar_off; tile.cigar = F.rec.cigar;
    tile.seq_off = F.seq_off; tile.seq4 = F.seq4;
    const int rc = cl_site_upload(F.ctx.get(), F.contig_len, F.blen, &tile);
    if (rc != CL_OK) F.engine_err(err, err_len, "site upload failed");
    return rc;
}

// The tile of the opened files resident for a scan: scan_files_upload, then, for a filtered scan (flt), the attachment --
// the records' flags and, per base, qual >= min_base_quality (none: every base passes) -- and the engine's filter in f
template <class Side, class SideOk>
int scan_files_resident(ScanFiles &F, const char *contig, int device_id, const FilterOptions *flt, cl_scan_filter &f, Side &&side, SideOk &&side_ok,
                        char *err, size_t err_len)
{
    int rc = scan_files_upload(F, contig, device_id, side, side_ok, err, err_len);
    if (rc != CL_OK || !flt) return rc;
    cl_site_quals q;
    q.n_reads = F.rec.n; q.flag = F.rec.flag; q.qual_off = F.rec.qual_off; q.qual = F.rec.qual; q.seq_off = F.seq_off;
    rc = cl_site_attach_quals(F.ctx.get(), &q, flt->has_min_base_quality ? flt->min_base_quality : 0);
    if (rc != CL_OK) F.engine_err(err, err_len, "site attachment failed");
    f = {flt->exclude_flags, (uint8_t)(flt->has_min_base_quality ? 1 : 0), 0};
    return rc;
}

// The file-level scan of a rule: its options checked, then always the filtered form -- its strand planes give the
// per-strand counts; with no mask and no threshold it counts what the unfiltered form does -- by the engine's scan of the
// rule, and its TSV by write
template <class Options, class Params, class Result>
int rule_files_run(const Rule &rule, const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start, uint32_t end,
                   const Options *o, const char *output_path, int device_id,
                   cl_status (*scan)(cl_ctx *, uint8_t, const cl_scan_filter *, const Params *, const uint8_t *, uint64_t, uint32_t, uint32_t, Result *),
                   int (*write)(const char *, const char *, const Result *, const Options *, char *, size_t), char *err, size_t err_len)
{
    if (!bam_path || !fasta_path || !contig || !output_path || !o) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    const ScanOptions r = scan_options(*o);
    if (!rule_ok(rule, r.min_depth, r.count, r.per_10k, err, err_len)) return CL_ERR_INVALID;
    ScanFiles F;
    cl_scan_filter f;
    int rc = scan_files_open(F, bam_path, fasta_path, contig, has_region, start, end, err, err_len);
    if (rc != CL_OK) return rc;
    if ((rc = scan_files_resident(F, contig, device_id, &r.flt, f, []() {}, []() { return true; }, err, err_len)) != CL_OK) return rc;
    const Params prm = {r.min_depth, r.count, r.per_10k};
    Result res;
    rc = scan(F.ctx.get(), r.min_quality, &f, &prm, F.bases, F.blen, start, end, &res);
    if (rc != CL_OK) { F.engine_err(err, err_len, "site scan failed"); return rc; }
    return write(output_path, contig, &res, o, err, err_len);
}

// ---- consensus ----
const char *const CONS_KIND[] = {"snv", "del", "ins", "ins_skipped"};
const char *const CONS_NOTE[] = {".", "anchor_deleted", "too_long", "no_allele"};

void cons_text(char *dst, size_t cap, const std::string &s) { snprintf(dst, cap, "%s", s.c_str()); }

int cons_assemble(const uint8_t *cons, uint32_t start, uint32_t end, const uint8_t *ref, uint64_t n_ref, const cl_ins_result *ins,
                  const dut_ins_allele *alleles, size_t n_alleles, const cl_ins_params *ip, int fill_ref, std::string &seq,
                  std::vector<dut_cons_change> &ch, uint64_t (&n)[3])
{
    const uint64_t len = (uint64_t)end - start;
    auto ref_at = [&](uint64_t i) -> char { return i < n_ref ? (char)ref[i] : 'N'; };       // as sent, case preserved
    auto ref_upper = [&](uint64_t i) -> char { return (char)(ref_at(i) & ~32); };
    const uint64_t n_ins = ins ? ins->n_inserted : 0;
    uint64_t ic = 0; size_t ia = 0;                                          // the next candidate and its first allele
    seq.reserve(len + 64);
    for (uint64_t i = 0; i < len; ++i) {
        const uint8_t b = cons[i];
        const uint32_t pos = start + (uint32_t)i + 1u;
        if (b == '-') {
            if (i == 0 || cons[i - 1] != '-') {
                uint64_t j = i;
                while (j + 1 < len && cons[j + 1] == '-') ++j;
                dut_cons_change c{};
                c.pos = pos; c.end = start + (uint32_t)j + 1u; c.kind = DUT_CONS_DEL;
                std::string r = ".";
                if (j - i + 1 <= 64) { r.clear(); for (uint64_t k = i; k <= j; ++k) r += ref_upper(k); }
                cons_text(c.ref, sizeof(c.ref), r); cons_text(c.cons, sizeof(c.cons), "-");
                ch.push_back(c); n[0] += 1;
            }
        } else if (b == 'N') seq += 'N';
        else if (b == 'n') { const char r = ref_base((uint8_t)ref_at(i)); seq += (fill_ref && r) ? (char)(r | 32) : 'N'; }
        else if (b == 'A' || b == 'C' || b == 'G' || b == 'T') {
            seq += (char)b;
            if (ref_base((uint8_t)ref_at(i)) != (char)b) {
                dut_cons_change c{};
                c.pos = c.end = pos; c.kind = DUT_CONS_SNV;
                cons_text(c.ref, sizeof(c.ref), std::string(1, ref_upper(i))); cons_text(c.cons, sizeof(c.cons), std::string(1, (char)b));
                ch.push_back(c);
            }
        } else return CL_ERR_INVALID;
        // a called insertion behind this position
        if (ic < n_ins && ins->candidates[ic].pos < pos) return CL_ERR_INVALID;      // not ascending, or below the range
        if (ic < n_ins && ins->candidates[ic].pos == pos) {
            const cl_ins_candidate &cd = ins->candidates[ic++];
            while (ia < n_alleles && alleles[ia].pos < pos) ++ia;
            if (ia >= n_alleles || alleles[ia].pos != pos) return CL_ERR_INVALID;    // a candidate has observations
            const dut_ins_allele &top = alleles[ia];
            std::string text;
            for (uint32_t j = 0; j < std::min<uint32_t>(top.len, 32u); ++j) {
                const char k = CODE[(top.key[j / 16] >> (60 - 4 * (j % 16))) & 15u];
                text += (k == 'A' || k == 'C' || k == 'G' || k == 'T') ? k : 'N';
            }
            dut_cons_change c{};
            c.pos = c.end = pos; c.count = top.count; c.depth = cd.depth;
            c.note = b == '-' ? DUT_CONS_NOTE_ANCHOR_DELETED : top.len > 32 ? DUT_CONS_NOTE_TOO_LONG
                   : !(top.count >= ip->min_ins_count && 10000ull * top.count >= (uint64_t)ip->min_ins_per_10k * cd.depth) ? DUT_CONS_NOTE_NO_ALLELE
                   : DUT_CONS_NOTE_NONE;
            c.kind = c.note ? DUT_CONS_INS_SKIPPED : DUT_CONS_INS;
            cons_text(c.ref, sizeof(c.ref), std::string(1, ref_upper(i))); cons_text(c.cons, sizeof(c.cons), text);
            if (!c.note) seq += text;
            ch.push_back(c); n[c.note ? 2 : 1] += 1;
        }
    }
    return ic == n_ins ? CL_OK : CL_ERR_INVALID;                             // a candidate beyond the range
}

bool cons_options_ok(const dut_cons_options &o, char *err, size_t err_len)
{
    if (!rule_ok(DEL_RULE, o.min_depth, o.min_del_count, o.min_del_per_10k, err, err_len)) return false;
    if (!rule_ok(INS_RULE, o.min_depth, o.min_ins_count, o.min_ins_per_10k, err, err_len)) return false;
    if (o.line_width == 0) { set_err(err, err_len, "line_width must be at least 1"); return false; }
    return true;
}

// no exception leaves the library through the C ABI
template <class F> int no_throw(char *err, size_t err_len, F &&f)
{
    try { return f(); }
    catch (const std::bad_alloc &) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_NOMEM; }
    catch (...) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_INVALID; }
}

} // namespace

extern "C" {

int dut_scan_classify(const uint32_t hist16[16], uint8_t ref_byte, uint32_t min_depth, char *called)
{
    if (called) *called = 0;
    if (!hist16) return CL_ERR_INVALID;
    uint64_t total = 0; uint32_t best = 0; int bc = 0;
    for (int c = 0; c < 16; ++c) { total += hist16[c]; if (hist16[c] > best) { best = hist16[c]; bc = c; } }
    if (total < min_depth) return DUT_SCAN_LOW_DEPTH;
    if (total == 0) return DUT_SCAN_LOW_DEPTH;                                // (min_depth 0 is refused everywhere; no bases, no call)
    const double freq = (double)best / (double)total;                         // caller.rs:139-141
    if (!(freq >= 0.7)) return DUT_SCAN_MIXED;
    if (called) *called = CODE[bc];
    return classify_call(CODE[bc], ref_byte);
}

int dut_scan_classify_counts(const uint32_t counts5[5], uint8_t ref_byte, uint32_t min_depth, char *called)
{
    if (called) *called = 0;
    if (!counts5) return CL_ERR_INVALID;
    const uint64_t total = counts5[4];
    uint64_t named = 0; uint32_t best = 0; int bi = 0;
    for (int i = 0; i < 4; ++i) { named += counts5[i]; if (counts5[i] > best) { best = counts5[i]; bi = i; } }
    if (named > total) return CL_ERR_INVALID;
    if (total < min_depth || total == 0) return DUT_SCAN_LOW_DEPTH;
    if ((double)best / (double)total >= 0.7) {
        if (called) *called = "ACGT"[bi];
        return classify_call("ACGT"[bi], ref_byte);
    }
    if ((double)(total - named) / (double)total >= 0.7) return DUT_SCAN_UNDETERMINED;
    return DUT_SCAN_MIXED;
}

// decimal text to parts per 10 000, exactly; the value in [1, max_per_10k], `range` naming that interval in the message
static int fraction_parse(const char *text, uint32_t *per_10k, uint32_t max_per_10k, const char *range, char *err, size_t err_len, uint32_t min_per_10k = 1)
{
    if (per_10k) *per_10k = 0;
    if (!text || !per_10k) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    // digits [ '.' digits ] or '.' digits, at most four decimals; the value in parts per 10 000, exactly
    const char *p = text;
    uint64_t whole = 0; int n_whole = 0, n_frac = 0; uint32_t frac = 0;
    for (; *p >= '0' && *p <= '9'; ++p, ++n_whole) whole = std::min<uint64_t>(whole * 10 + (uint64_t)(*p - '0'), 1000000);
    if (*p == '.') for (++p; *p >= '0' && *p <= '9'; ++p, ++n_frac) if (n_frac < 4) frac = frac * 10 + (uint32_t)(*p - '0');
    if (*p || n_whole + n_frac == 0) { set_err(err, err_len, "not a decimal fraction"); return CL_ERR_INVALID; }
    if (n_frac > 4) { set_err(err, err_len, "at most four decimals"); return CL_ERR_INVALID; }
    for (int k = n_frac; k < 4; ++k) frac *= 10;
    const uint64_t v = whole * 10000 + frac;
    if (v < min_per_10k || v > max_per_10k) { set_err(err, err_len, std::string("the fraction must lie in ") + range); return CL_ERR_INVALID; }
    *per_10k = (uint32_t)v;
    return CL_OK;
}

int dut_minor_fraction_parse(const char *text, uint32_t *per_10k, char *err, size_t err_len)
{
    return fraction_parse(text, per_10k, 5000, "(0, 0.5]", err, err_len);
}

int dut_del_fraction_parse(const char *text, uint32_t *per_10k, char *err, size_t err_len)
{
    return fraction_parse(text, per_10k, 10000, "(0, 1]", err, err_len);
}

int dut_del_classify_counts(uint32_t del, uint32_t depth, const cl_del_params *params)
{
    if (!params || !rule_ok(DEL_RULE, params->min_depth, params->min_del_count, params->min_del_per_10k)) return CL_ERR_INVALID;
    const uint64_t span = (uint64_t)del + depth;
    if (span < params->min_depth) return DUT_DEL_LOW_DEPTH;
    return (del >= params->min_del_count && 10000ull * del >= (uint64_t)params->min_del_per_10k * span) ? DUT_DEL_DELETED : DUT_DEL_KEPT;
}

// maximal runs of consecutive positions; per run the position of the smallest del (the first among equals)
static int del_events(const cl_del_candidate *cand, size_t n, std::vector<dut_del_event> &ev)
{
    for (size_t i = 0; i < n; ++i) {
        const cl_del_candidate &c = cand[i];
        if (i && c.pos <= cand[i - 1].pos) return CL_ERR_INVALID;
        if (i == 0 || c.pos != cand[i - 1].pos + 1) {
            dut_del_event e{};
            e.start = e.end = e.q = c.pos; e.length = 1;
            e.del = e.max_del = c.del; e.del_fwd = c.del_fwd; e.del_rev = c.del_rev; e.span = (uint64_t)c.del + c.depth;
            ev.push_back(e);
            continue;
        }
        dut_del_event &e = ev.back();
        e.end = c.pos; e.length += 1;
        if (c.del < e.del) { e.q = c.pos; e.del = c.del; e.del_fwd = c.del_fwd; e.del_rev = c.del_rev; e.span = (uint64_t)c.del + c.depth; }
        e.max_del = std::max(e.max_del, c.del);
    }
    return CL_OK;
}

int dut_del_events(const cl_del_candidate *candidates, size_t n, dut_del_event **events, size_t *n_events)
{
    if (events) *events = nullptr;
    if (n_events) *n_events = 0;
    if (!events || !n_events || (n && !candidates)) return CL_ERR_INVALID;
    try {
        std::vector<dut_del_event> ev;
        if (del_events(candidates, n, ev) != CL_OK) return CL_ERR_INVALID;
        if (ev.empty()) return CL_OK;
        dut_del_event *out = static_cast<dut_del_event *>(malloc(ev.size() * sizeof(dut_del_event)));
        if (!out) return CL_ERR_NOMEM;
        memcpy(out, ev.data(), ev.size() * sizeof(dut_del_event));
        *events = out; *n_events = ev.size();
        return CL_OK;
    }
    catch (...) { return CL_ERR_NOMEM; }
}

void dut_del_events_free(dut_del_event *events) { free(events); }

static int del_write(const char *path, const char *contig, const cl_del_result *res, const dut_del_options *opt, char *err, size_t err_len)
{
    if (!path || !contig || !res || !opt || (res->n_deleted && !res->candidates)) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    std::vector<dut_del_event> ev;
    if (del_events(res->candidates, (size_t)res->n_deleted, ev) != CL_OK) { set_err(err, err_len, "candidate positions must ascend"); return CL_ERR_INVALID; }
    std::string s;
    char b[512];
    tsv_preamble(s, contig, res->start, res->end, scan_options(*opt), true, &DEL_RULE);
    snprintf(b, sizeof(b), "##low_depth=%llu\n##kept=%llu\n##deleted=%llu\n##events=%llu\n", (unsigned long long)res->n_low_depth,
             (unsigned long long)res->n_kept, (unsigned long long)res->n_deleted, (unsigned long long)ev.size());
    s += b;
    s += "#contig\tstart\tend\tlength\tref\tdel\tspan\tfreq\tmax_del\tdel_fwd\tdel_rev\tfilter\n";
    size_t at = 0;                                                           // the event's first candidate
    for (const dut_del_event &e : ev) {
        std::string ref = ".";
        if (e.length <= 64) { ref.clear(); for (uint32_t k = 0; k < e.length; ++k) ref += (char)res->candidates[at + k].ref; }
        at += e.length;
        const double freq = e.span ? (double)e.del / (double)e.span : 0.0;
        const bool strand = std::min(e.del_fwd, e.del_rev) < opt->min_del_per_strand;
        snprintf(b, sizeof(b), "\t%u\t%u\t%u\t%s\t%u\t%llu\t%.4f\t%u\t%u\t%u\t%s\n", e.start, e.end, e.length, ref.c_str(), e.del,
                 (unsigned long long)e.span, freq, e.max_del, e.del_fwd, e.del_rev, strand ? "strand" : "PASS");
        s += contig; s += b;
    }
    return write_file(path, s, err, err_len);
}

int dut_del_write(const char *path, const char *contig, const cl_del_result *res, const dut_del_options *opt, char *err, size_t err_len)
{
    try { return del_write(path, contig, res, opt, err, err_len); }
    catch (...) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_NOMEM; }
}

int dut_ins_classify_counts(uint32_t ins, uint32_t depth, const cl_ins_params *params)
{
    if (!params || !rule_ok(INS_RULE, params->min_depth, params->min_ins_count, params->min_ins_per_10k)) return CL_ERR_INVALID;
    if (depth < params->min_depth) return DUT_INS_LOW_DEPTH;
    return (ins >= params->min_ins_count && 10000ull * ins >= (uint64_t)params->min_ins_per_10k * depth) ? DUT_INS_INSERTED : DUT_INS_KEPT;
}

// observations of equal (pos, len, key) counted; per position the top allele in front, the others by (len, key)
static void ins_alleles(const cl_ins_obs *obs, size_t n, std::vector<dut_ins_allele> &al)
{
    std::vector<const cl_ins_obs *> o(n);
    for (size_t i = 0; i < n; ++i) o[i] = obs + i;
    auto same = [](const cl_ins_obs &a, const cl_ins_obs &b) { return a.pos == b.pos && a.len == b.len && a.key[0] == b.key[0] && a.key[1] == b.key[1]; };
    std::sort(o.begin(), o.end(), [](const cl_ins_obs *a, const cl_ins_obs *b) {
        if (a->pos != b->pos) return a->pos < b->pos;
        if (a->len != b->len) return a->len < b->len;
        if (a->key[0] != b->key[0]) return a->key[0] < b->key[0];
        return a->key[1] < b->key[1];
    });
    size_t first = 0;                                                        // the first allele of the position at hand
    for (size_t i = 0; i < n; ++i) {
        if (i == 0 || !same(*o[i], *o[i - 1])) {
            if (i && o[i]->pos != o[i - 1]->pos) first = al.size();
            dut_ins_allele a{};
            a.pos = o[i]->pos; a.len = o[i]->len; a.key[0] = o[i]->key[0]; a.key[1] = o[i]->key[1];
            al.push_back(a);
        }
        dut_ins_allele &a = al.back();
        a.count += 1; (o[i]->strand ? a.rev : a.fwd) += 1;
        // the position's last observation: its largest allele (the first in (len, key) order among equals) moves to the front
        if (i + 1 == n || o[i + 1]->pos != o[i]->pos) {
            size_t top = first;
            for (size_t k = first + 1; k < al.size(); ++k) if (al[k].count > al[top].count) top = k;
            std::rotate(al.begin() + first, al.begin() + top, al.begin() + top + 1);
        }
    }
}

int dut_ins_alleles(const cl_ins_obs *obs, size_t n_obs, dut_ins_allele **alleles, size_t *n_alleles)
{
    if (alleles) *alleles = nullptr;
    if (n_alleles) *n_alleles = 0;
    if (!alleles || !n_alleles || (n_obs && !obs)) return CL_ERR_INVALID;
    try {
        std::vector<dut_ins_allele> al;
        ins_alleles(obs, n_obs, al);
        if (al.empty()) return CL_OK;
        dut_ins_allele *out = static_cast<dut_ins_allele *>(malloc(al.size() * sizeof(dut_ins_allele)));
        if (!out) return CL_ERR_NOMEM;
        memcpy(out, al.data(), al.size() * sizeof(dut_ins_allele));
        *alleles = out; *n_alleles = al.size();
        return CL_OK;
    }
    catch (...) { return CL_ERR_NOMEM; }
}

void dut_ins_alleles_free(dut_ins_allele *alleles) { free(alleles); }

static int ins_write(const char *path, const char *contig, const cl_ins_result *res, const dut_ins_options *opt, char *err, size_t err_len)
{
    if (!path || !contig || !res || !opt || (res->n_inserted && !res->candidates) || (res->n_obs && !res->obs)) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    std::vector<dut_ins_allele> al;
    ins_alleles(res->obs, (size_t)res->n_obs, al);
    std::string s;
    char b[512];
    tsv_preamble(s, contig, res->start, res->end, scan_options(*opt), true, &INS_RULE);
    snprintf(b, sizeof(b), "##low_depth=%llu\n##kept=%llu\n##inserted=%llu\n", (unsigned long long)res->n_low_depth,
             (unsigned long long)res->n_kept, (unsigned long long)res->n_inserted);
    s += b;
    s += "#contig\tpos\tref\tins\tdepth\tfreq\talleles\tlength\tseq\tallele_count\tallele_fwd\tallele_rev\tins_fwd\tins_rev\tfilter\n";
    size_t at = 0;                                                           // the candidate's first allele
    for (uint64_t i = 0; i < res->n_inserted; ++i) {
        const cl_ins_candidate &c = res->candidates[i];
        if (i && c.pos <= res->candidates[i - 1].pos) { set_err(err, err_len, "candidate positions must ascend"); return CL_ERR_INVALID; }
        size_t n_al = 0; uint64_t n_obs = 0;
        while (at + n_al < al.size() && al[at + n_al].pos == c.pos) { n_obs += al[at + n_al].count; ++n_al; }
        if (n_obs != c.ins || n_al == 0) { set_err(err, err_len, "a candidate's observations must be as many as its ins"); return CL_ERR_INVALID; }
        const dut_ins_allele &top = al[at];
        at += n_al;
        std::string seq;
        for (uint32_t j = 0; j < std::min<uint32_t>(top.len, 32u); ++j) seq += CODE[(top.key[j / 16] >> (60 - 4 * (j % 16))) & 15u];
        if (top.len > 32) seq += "...";
        const double freq = c.depth ? (double)c.ins / (double)c.depth : 0.0;
        const bool strand = std::min(c.ins_fwd, c.ins_rev) < opt->min_ins_per_strand;
        snprintf(b, sizeof(b), "\t%u\t%c\t%u\t%u\t%.4f\t%llu\t%u\t%s\t%u\t%u\t%u\t%u\t%u\t%s\n", c.pos, (char)c.ref, c.ins, c.depth, freq,
                 (unsigned long long)n_al, top.len, seq.c_str(), top.count, top.fwd, top.rev, c.ins_fwd, c.ins_rev, strand ? "strand" : "PASS");
        s += contig; s += b;
    }
    if (at != al.size()) { set_err(err, err_len, "observations at a position that is no candidate"); return CL_ERR_INVALID; }
    return write_file(path, s, err, err_len);
}

int dut_ins_write(const char *path, const char *contig, const cl_ins_result *res, const dut_ins_options *opt, char *err, size_t err_len)
{
    try { return ins_write(path, contig, res, opt, err, err_len); }
    catch (...) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_NOMEM; }
}

int dut_cons_classify_counts(uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint64_t depth, uint32_t del, const cl_cons_params *params,
                             uint8_t ref_byte, char *byte)
{
    if (byte) *byte = 0;
    if (!params || !rule_ok(DEL_RULE, params->min_depth, params->min_del_count, params->min_del_per_10k)) return CL_ERR_INVALID;
    if ((uint64_t)a + c + g + t > depth || depth > 0xFFFFFFFFull) return CL_ERR_INVALID;
    const uint32_t cnt[4] = {a, c, g, t};
    int mi = 0;
    for (int b = 1; b < 4; ++b) if (cnt[b] > cnt[mi]) mi = b;                  // the first among equals
    const uint64_t span = depth + del, m = cnt[mi];
    auto leave = [&](int cls, char b) { if (byte) *byte = b; return cls; };
    if (span < params->min_depth) return leave(DUT_CONS_LOW_DEPTH, 'n');
    if (del >= params->min_del_count && 10000ull * del >= (uint64_t)params->min_del_per_10k * span) return leave(DUT_CONS_DELETED, '-');
    if (depth < params->min_depth) return leave(DUT_CONS_LOW_DEPTH, 'n');
    if (10ull * m >= 7ull * depth) return leave("ACGT"[mi] == ref_base(ref_byte) ? DUT_CONS_REF : DUT_CONS_ALT, "ACGT"[mi]);
    return leave(DUT_CONS_NO_CALL, 'N');
}

int dut_cons_assemble(const uint8_t *cons, uint32_t start, uint32_t end, const uint8_t *ref, uint64_t n_ref, const cl_ins_result *ins,
                      const dut_ins_allele *alleles, size_t n_alleles, const cl_ins_params *ins_params, int fill_ref, dut_cons_assembly *out)
{
    if (out) memset(out, 0, sizeof(*out));
    if (!out || start > end || (end > start && !cons) || (n_ref && !ref)) return CL_ERR_INVALID;
    if (ins && ins->n_inserted && (!ins->candidates || !alleles || !ins_params ||
                                   !rule_ok(INS_RULE, ins_params->min_depth, ins_params->min_ins_count, ins_params->min_ins_per_10k))) return CL_ERR_INVALID;
    try {
        std::string seq;
        std::vector<dut_cons_change> ch;
        uint64_t n[3] = {0, 0, 0};
        const int rc = cons_assemble(cons, start, end, ref, n_ref, ins, alleles, n_alleles, ins_params, fill_ref, seq, ch, n);
        if (rc != CL_OK) return rc;
        out->seq = static_cast<char *>(malloc(seq.size() + 1));
        out->changes = static_cast<dut_cons_change *>(malloc(std::max<size_t>(ch.size(), 1) * sizeof(dut_cons_change)));
        if (!out->seq || !out->changes) { dut_cons_assembly_free(out); return CL_ERR_NOMEM; }
        memcpy(out->seq, seq.c_str(), seq.size() + 1);
        if (!ch.empty()) memcpy(out->changes, ch.data(), ch.size() * sizeof(dut_cons_change));
        out->seq_len = seq.size(); out->n_changes = ch.size();
        out->n_deletions = n[0]; out->n_insertions = n[1]; out->n_insertions_skipped = n[2];
        return CL_OK;
    }
    catch (...) { dut_cons_assembly_free(out); return CL_ERR_NOMEM; }
}

void dut_cons_assembly_free(dut_cons_assembly *a)
{
    if (!a) return;
    free(a->seq); free(a->changes);
    memset(a, 0, sizeof(*a));
}

int dut_cons_write_fasta(const char *path, const char *contig, int whole_contig, uint32_t start, uint32_t end, const char *seq, uint64_t seq_len,
                         uint32_t line_width, char *err, size_t err_len)
{
    if (!path || !contig || (seq_len && !seq)) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    if (line_width == 0) { set_err(err, err_len, "line_width must be at least 1"); return CL_ERR_INVALID; }
    return no_throw(err, err_len, [&]() -> int {
        std::string s = std::string(">") + contig;
        if (!whole_contig) s += ":" + std::to_string((uint64_t)start + 1) + "-" + std::to_string(end);
        s += "\n";
        s.reserve(s.size() + seq_len + seq_len / line_width + 2);
        for (uint64_t at = 0; at < seq_len; at += line_width) { s.append(seq + at, (size_t)std::min<uint64_t>(line_width, seq_len - at)); s += "\n"; }
        return write_file(path, s, err, err_len);
    });
}

int dut_cons_write_changes(const char *path, const char *contig, const cl_cons_result *res, const dut_cons_assembly *a, const dut_cons_options *opt,
                           char *err, size_t err_len)
{
    if (!path || !contig || !res || !a || !opt || (a->n_changes && !a->changes)) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    return no_throw(err, err_len, [&]() -> int {
        std::string s;
        char b[512];
        const ScanOptions o = {opt->min_depth, opt->min_quality, {opt->has_min_base_quality, opt->min_base_quality, opt->exclude_flags}, opt->min_del_per_10k,
                               opt->min_del_count, 0};
        tsv_preamble(s, contig, res->start, res->end, o, true, &DEL_RULE);
        // (tsv_preamble ends with ##positions: the insertion rule and the fill mode go in front of it)
        const size_t at = s.rfind("##positions=");
        snprintf(b, sizeof(b), "##%s=%.4f\n##%s=%u\n##fill=%s\n", INS_RULE.fraction, (double)opt->min_ins_per_10k / 10000.0, INS_RULE.count, opt->min_ins_count,
                 opt->fill_ref ? "ref" : "N");
        s.insert(at, b);
        snprintf(b, sizeof(b), "##low_depth=%llu\n##deleted=%llu\n##no_call=%llu\n##ref=%llu\n##alt=%llu\n##length=%llu\n##deletions=%llu\n##insertions=%llu\n"
                               "##insertions_skipped=%llu\n",
                 (unsigned long long)res->n_low_depth, (unsigned long long)res->n_deleted, (unsigned long long)res->n_no_call, (unsigned long long)res->n_ref,
                 (unsigned long long)res->n_alt, (unsigned long long)a->seq_len, (unsigned long long)a->n_deletions, (unsigned long long)a->n_insertions,
                 (unsigned long long)a->n_insertions_skipped);
        s += b;
        s += "#contig\tpos\tend\tkind\tref\tcons\tcount\tdepth\tnote\n";
        for (size_t i = 0; i < a->n_changes; ++i) {
            const dut_cons_change &c = a->changes[i];
            if (c.kind > DUT_CONS_INS_SKIPPED || c.note > DUT_CONS_NOTE_NO_ALLELE) { set_err(err, err_len, "unknown kind of change"); return CL_ERR_INVALID; }
            const bool is_ins = c.kind == DUT_CONS_INS || c.kind == DUT_CONS_INS_SKIPPED;
            snprintf(b, sizeof(b), "\t%u\t%u\t%s\t%.67s\t%.35s\t", c.pos, c.end, CONS_KIND[c.kind], c.ref, c.cons);
            s += contig; s += b;
            if (is_ins) { snprintf(b, sizeof(b), "%u\t%u\t", c.count, c.depth); s += b; } else s += ".\t.\t";
            s += CONS_NOTE[c.note]; s += "\n";
        }
        return write_file(path, s, err, err_len);
    });
}

int dut_find_consensus_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start, uint32_t end,
                             const dut_cons_options *opt, const char *output_path, const char *changes_path, int device_id, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&]() -> int {
        if (!bam_path || !fasta_path || !contig || !output_path || !opt) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        if (!cons_options_ok(*opt, err, err_len)) return CL_ERR_INVALID;
        ScanFiles F;
        cl_scan_filter f;
        int rc = scan_files_open(F, bam_path, fasta_path, contig, has_region, start, end, err, err_len);
        if (rc != CL_OK) return rc;
        const FilterOptions flt = {opt->has_min_base_quality, opt->min_base_quality, opt->exclude_flags};
        if ((rc = scan_files_resident(F, contig, device_id, &flt, f, []() {}, []() { return true; }, err, err_len)) != CL_OK) return rc;
        // both scans on the one resident tile: their results live in storage of their own
        const cl_cons_params cp = {opt->min_depth, opt->min_del_count, opt->min_del_per_10k};
        const cl_ins_params ip = {opt->min_depth, opt->min_ins_count, opt->min_ins_per_10k};
        cl_cons_result cres;
        cl_ins_result ires;
        if ((rc = cl_site_scan_consensus(F.ctx.get(), opt->min_quality, &f, &cp, F.bases, F.blen, start, end, &cres)) != CL_OK ||
            (rc = cl_site_scan_ins(F.ctx.get(), opt->min_quality, &f, &ip, F.bases, F.blen, start, end, &ires)) != CL_OK) {
            F.engine_err(err, err_len, "site scan failed");
            return rc;
        }
        dut_ins_allele *al = nullptr; size_t n_al = 0;
        if (ires.n_obs && (rc = dut_ins_alleles(ires.obs, (size_t)ires.n_obs, &al, &n_al)) != CL_OK) { set_err(err, err_len, "grouping the insertions failed"); return rc; }
        std::unique_ptr<dut_ins_allele, decltype(&dut_ins_alleles_free)> al_own(al, dut_ins_alleles_free);
        const uint64_t n_ref = std::min<uint64_t>(end, F.blen) > start ? std::min<uint64_t>(end, F.blen) - start : 0;
        dut_cons_assembly A;
        if ((rc = dut_cons_assemble(cres.cons, start, end, F.bases + std::min<uint64_t>(start, F.blen), n_ref, &ires, al, n_al, &ip, opt->fill_ref, &A)) != CL_OK) {
            set_err(err, err_len, "assembling the consensus failed");
            return rc;
        }
        rc = dut_cons_write_fasta(output_path, contig, start == 0 && end == F.contig_len, start, end, A.seq, A.seq_len, opt->line_width, err, err_len);
        if (rc == CL_OK && changes_path) rc = dut_cons_write_changes(changes_path, contig, &cres, &A, opt, err, err_len);
        dut_cons_assembly_free(&A);
        return rc;
    });
}

int dut_minor_classify_counts(uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint64_t depth, const cl_minor_params *params, char *major, char *minor)
{
    if (major) *major = 0;
    if (minor) *minor = 0;
    if (!params || !rule_ok(MINOR_RULE, params->min_depth, params->min_minor_count, params->min_minor_per_10k)) return CL_ERR_INVALID;
    if ((uint64_t)a + c + g + t > depth || depth > 0xFFFFFFFFull) return CL_ERR_INVALID;
    const uint32_t cnt[4] = {a, c, g, t};
    int mi = 0;
    for (int b = 1; b < 4; ++b) if (cnt[b] > cnt[mi]) mi = b;                  // the first among equals
    int ni = mi == 0 ? 1 : 0;
    for (int b = 1; b < 4; ++b) if (b != mi && cnt[b] > cnt[ni]) ni = b;
    if (major) *major = "ACGT"[mi];
    if (minor) *minor = "ACGT"[ni];
    if (depth < params->min_depth) return DUT_MINOR_LOW_DEPTH;
    const uint64_t c2 = cnt[ni];
    return (c2 >= params->min_minor_count && 10000ull * c2 >= (uint64_t)params->min_minor_per_10k * depth) ? DUT_MINOR_MINOR : DUT_MINOR_SINGLE;
}

int dut_minor_write(const char *path, const char *contig, const cl_minor_result *res, const dut_minor_options *opt, char *err, size_t err_len)
{
    if (!path || !contig || !res || !opt || (res->n_minor && !res->candidates)) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    std::string s;
    char b[512];
    tsv_preamble(s, contig, res->start, res->end, scan_options(*opt), true, &MINOR_RULE);
    snprintf(b, sizeof(b), "##low_depth=%llu\n##single=%llu\n##minor=%llu\n", (unsigned long long)res->n_low_depth,
             (unsigned long long)res->n_single, (unsigned long long)res->n_minor);
    s += b;
    s += "#contig\tpos\tref\tmajor\tminor\tdepth\tA\tC\tG\tT\tminor_freq\tmajor_fwd\tmajor_rev\tminor_fwd\tminor_rev\tfilter\n";
    for (uint64_t i = 0; i < res->n_minor; ++i) {
        const cl_minor_candidate &c = res->candidates[i];
        const uint32_t c2 = c.minor == 'A' ? c.a : c.minor == 'C' ? c.c : c.minor == 'G' ? c.g : c.t;
        const double freq = c.depth ? (double)c2 / (double)c.depth : 0.0;
        const bool strand = std::min(c.minor_fwd, c.minor_rev) < opt->min_minor_per_strand;
        snprintf(b, sizeof(b), "\t%u\t%c\t%c\t%c\t%u\t%u\t%u\t%u\t%u\t%.4f\t%u\t%u\t%u\t%u\t%s\n", c.pos, (char)c.ref, (char)c.major, (char)c.minor, c.depth,
                 c.a, c.c, c.g, c.t, freq, c.major_fwd, c.major_rev, c.minor_fwd, c.minor_rev, strand ? "strand" : "PASS");
        s += contig; s += b;
    }
    return write_file(path, s, err, err_len);
}

int dut_variants_annotate(const dut_tree *t, const char *build_id, const char *chromosome,
                          const cl_scan_candidate *candidates, size_t n, dut_variant_note **notes)
{
    return annotate(t, build_id, chromosome, candidates, n, notes);
}

int dut_variants_annotate_ex(const dut_tree *t, const char *build_id, const char *chromosome,
                             const cl_scan_candidate_ex *candidates, size_t n, dut_variant_note **notes)
{
    return annotate(t, build_id, chromosome, candidates, n, notes);
}

void dut_variants_free_notes(dut_variant_note *notes, size_t n)
{
    if (!notes) return;
    for (size_t i = 0; i < n; ++i) { free(notes[i].names); free(notes[i].alleles); }
    free(notes);
}

int dut_variants_write(const char *path, const char *contig, const cl_scan_result *res, uint32_t min_depth,
                       uint8_t min_quality, const dut_variant_note *notes, char *err, size_t err_len)
{
    return write_tsv(path, contig, res, min_depth, min_quality, nullptr, notes, err, err_len);
}

int dut_variants_write_ex(const char *path, const char *contig, const cl_scan_result_ex *res, uint32_t min_depth,
                          uint8_t min_quality, const dut_variants_options *opt, const dut_variant_note *notes,
                          char *err, size_t err_len)
{
    if (!opt) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    return write_tsv(path, contig, res, min_depth, min_quality, opt, notes, err, err_len);
}

int dut_find_variants_files_ex(const char *bam_path, const char *fasta_path, const char *contig, int has_region,
                               uint32_t start, uint32_t end, const char *tree_json_path, int provider, int tree_type,
                               const char *output_path, uint32_t min_depth, uint8_t min_quality,
                               const dut_variants_options *vopt, int device_id, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&]() -> int {
        if (!bam_path || !fasta_path || !contig || !output_path) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        if (min_depth == 0) { set_err(err, err_len, "min_depth must be at least 1"); return CL_ERR_INVALID; }
        ScanFiles F;
        int rc = scan_files_open(F, bam_path, fasta_path, contig, has_region, start, end, err, err_len);
        if (rc != CL_OK) return rc;
        // the build id the tree's coordinates are looked up by (mod.rs:51-54): the genome the header names, rCRS for mt
        std::string build;
        if (tree_json_path) {
            size_t tl = 0;
            const char *text = dut_bam_header_text(F.bam.get(), &tl);
            build = dut_reference_build(text, tl);
            if (build == "Unknown") { set_err(err, err_len, "Could not determine reference genome from BAM header"); return CL_ERR_INVALID; }
            if (tree_type == DUT_TREE_MTDNA) build = "rCRS";
        }
        // side by side, as dut_find_branch_files does: the tree JSON, the HIP runtime + context, the contig's records
        std::unique_ptr<dut_tree, decltype(&dut_tree_free)> tree(nullptr, dut_tree_free);
        char terr[512] = {0};
        const bool filtered = vopt && vopt->filtered;
        FilterOptions flt{};
        if (filtered) flt = {vopt->has_min_base_quality, vopt->min_base_quality, vopt->exclude_flags};
        cl_scan_filter f;
        rc = scan_files_resident(F, contig, device_id, filtered ? &flt : nullptr, f,
                                 [&]() { if (tree_json_path) tree.reset(dut_tree_load(tree_json_path, provider, tree_type, terr, sizeof(terr))); },
                                 [&]() { if (tree_json_path && !tree) { set_err(err, err_len, terr); return false; } return true; }, err, err_len);
        if (rc != CL_OK) return rc;
        // scan result -> annotation -> TSV, for either result type (wopt: the filter columns of the header, or none)
        auto finish = [&](int scan_rc, const auto &res, const dut_variants_options *wopt) {
            if (scan_rc != CL_OK) { F.engine_err(err, err_len, "site scan failed"); return scan_rc; }
            dut_variant_note *notes = nullptr;
            if (tree) {
                const int arc = annotate(tree.get(), build.c_str(), contig, res.candidates, (size_t)res.n_variant, &notes);
                if (arc != CL_OK) { set_err(err, err_len, "annotation failed"); return arc; }
            }
            const int wrc = write_tsv(output_path, contig, &res, min_depth, min_quality, wopt, notes, err, err_len);
            dut_variants_free_notes(notes, (size_t)res.n_variant);
            return wrc;
        };
        if (filtered) {
            cl_scan_result_ex res;
            return finish(cl_site_scan_ex(F.ctx.get(), min_quality, min_depth, &f, F.bases, F.blen, start, end, &res), res, vopt);
        }
        cl_scan_result res;
        return finish(cl_site_scan(F.ctx.get(), min_quality, min_depth, F.bases, F.blen, start, end, &res), res, nullptr);
    });
}

int dut_find_deletions_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start, uint32_t end,
                             const dut_del_options *opt, const char *output_path, int device_id, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&] { return rule_files_run(DEL_RULE, bam_path, fasta_path, contig, has_region, start, end, opt, output_path, device_id,
                                                              cl_site_scan_dels, dut_del_write, err, err_len); });
}

int dut_find_insertions_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start, uint32_t end,
                              const dut_ins_options *opt, const char *output_path, int device_id, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&] { return rule_files_run(INS_RULE, bam_path, fasta_path, contig, has_region, start, end, opt, output_path, device_id,
                                                              cl_site_scan_ins, dut_ins_write, err, err_len); });
}

int dut_find_minor_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start, uint32_t end,
                         const dut_minor_options *opt, const char *output_path, int device_id, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&] { return rule_files_run(MINOR_RULE, bam_path, fasta_path, contig, has_region, start, end, opt, output_path, device_id,
                                                              cl_site_scan_minor, dut_minor_write, err, err_len); });
}

int dut_find_variants_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region,
                            uint32_t start, uint32_t end, const char *tree_json_path, int provider, int tree_type,
                            const char *output_path, uint32_t min_depth, uint8_t min_quality, int device_id,
                            char *err, size_t err_len)
{
    return dut_find_variants_files_ex(bam_path, fasta_path, contig, has_region, start, end, tree_json_path, provider, tree_type,
                                      output_path, min_depth, min_quality, nullptr, device_id, err, err_len);
}

// ---- find-strs ----
static bool str_options_ok(const dut_str_options &o, char *err, size_t err_len)
{
    char b[96] = {0};
    if (o.min_depth == 0) snprintf(b, sizeof(b), "min_depth must be at least 1");
    else if (o.flank < 1 || o.flank > CL_STR_MAX_FLANK) snprintf(b, sizeof(b), "flank must lie in 1..%u", (unsigned)CL_STR_MAX_FLANK);
    else if (o.min_allele_per_10k < 1 || o.min_allele_per_10k > 10000) snprintf(b, sizeof(b), "min_allele_per_10k must lie in 1..10000");
    else return true;
    set_err(err, err_len, b);
    return false;
}

static const char *str_locus_fault(uint32_t start, uint32_t end, uint32_t contig_len)
{
    return start >= end ? "start >= end" : end > contig_len ? "it ends beyond the contig" : end - start > CL_STR_MAX_SPAN ? "it is longer than 1024 positions" : nullptr;
}

int dut_str_measure(const int32_t *pos, const uint16_t *flag, const uint8_t *mapq, const uint32_t *cigar_off, const uint32_t *cigar,
                    uint64_t n_reads, uint32_t contig_len, uint8_t min_quality, uint16_t exclude_flags, uint32_t flank,
                    const cl_str_locus *loci, size_t n_loci, uint32_t *hist, uint32_t *partial, uint32_t strands)
{
    return no_throw(nullptr, 0, [&]() -> int {
        if (strands < 1 || strands > 2 || flank < 1 || flank > CL_STR_MAX_FLANK) return CL_ERR_INVALID;
        if (n_reads && (!pos || !mapq || !cigar_off || (strands == 2 && !flag))) return CL_ERR_INVALID;
        if (n_loci && (!loci || !hist || !partial)) return CL_ERR_INVALID;
        if (n_reads > 0xFFFFFFF0ull) return CL_ERR_INVALID;
        for (size_t i = 0; i < n_loci; ++i) if (str_locus_fault(loci[i].start, loci[i].end, contig_len)) return CL_ERR_INVALID;
        for (uint64_t r = 0; r < n_reads; ++r) if (cigar_off[r + 1] < cigar_off[r]) return CL_ERR_INVALID;
        if (n_reads && cigar_off[n_reads] > cigar_off[0] && !cigar) return CL_ERR_INVALID;
        // the reads of a locus: per read its reference end (0: it never takes part), per window of kWin positions the range
        // of the reads that overlap it -- wider for an unsorted tile, exact all the same
        constexpr uint32_t kWin = CL_STR_MAX_SPAN;
        const size_t n_win = ((size_t)contig_len + kWin - 1) / kWin;
        std::vector<uint32_t> rend(n_reads, 0), wfirst(n_win + 1, 0xFFFFFFFFu), wlast(n_win + 1, 0);
        for (uint64_t r = 0; r < n_reads; ++r) {
            const uint32_t x = (uint32_t)pos[r];
            if (x >= contig_len) continue;
            uint64_t span = 0;
            for (uint32_t k = cigar_off[r]; k < cigar_off[r + 1]; ++k) { const uint32_t c = cigar[k]; span += ((0x18Du >> (c & 15u)) & 1u) ? (c >> 4) : 0u; }
            if (!span) continue;
            const uint64_t xe = (uint64_t)x + span;
            rend[r] = xe > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)xe;
            const uint32_t last_p = std::min(rend[r], contig_len) - 1u;
            for (uint32_t w = x / kWin; w <= last_p / kWin; ++w) { wfirst[w] = std::min(wfirst[w], (uint32_t)r); wlast[w] = std::max(wlast[w], (uint32_t)r + 1u); }
        }
        dut::parallel_for(n_loci, 16, [&](size_t i) {
            const uint32_t s = loci[i].start, e = loci[i].end;
            uint32_t *h = hist + i * strands * CL_STR_BINS;
            memset(h, 0, (size_t)strands * CL_STR_BINS * 4);
            uint32_t part = 0;
            const uint32_t w0 = s / kWin, w1 = (e - 1u) / kWin;
            const uint32_t r0 = std::min(wfirst[w0], wfirst[w1]), r1 = std::max(wlast[w0], wlast[w1]);
            for (uint32_t r = r0; r < r1; ++r) {
                if (mapq[r] < min_quality || rend[r] <= s || (uint32_t)pos[r] >= e) continue;
                uint32_t rev = 0;
                if (strands == 2) { if (flag[r] & exclude_flags) continue; rev = (flag[r] >> 4) & 1u; }
                const dut::StrMeasure m = dut::str_measure_read((uint32_t)pos[r], cigar + cigar_off[r], cigar_off[r + 1] - cigar_off[r], s, e, flank);
                if (m.spanning) h[rev * CL_STR_BINS + dut::str_bin(m.delta)] += 1u; else part += 1u;
            }
            partial[i] = part;
        });
        return CL_OK;
    });
}

int dut_str_call(const uint32_t *hist_fwd, const uint32_t *hist_rev, const dut_str_params *params, dut_str_allele_call *call)
{
    if (!hist_fwd || !params || !call) return CL_ERR_INVALID;
    if (params->min_depth == 0 || params->min_allele_per_10k < 1 || params->min_allele_per_10k > 10000) return CL_ERR_INVALID;
    auto at = [&](int b) -> uint64_t { return (uint64_t)hist_fwd[b] + (hist_rev ? hist_rev[b] : 0u); };
    uint64_t n = 0;
    for (int b = 0; b < CL_STR_BINS; ++b) n += at(b);
    int top = 0, second = -1;
    for (int b = 1; b < CL_STR_BINS - 1; ++b) if (at(b) > at(top)) top = b;                // the first among equals: the smallest delta
    for (int b = 0; b < CL_STR_BINS - 1; ++b) if (b != top && (second < 0 || at(b) > at(second))) second = b;
    memset(call, 0, sizeof(*call));
    call->n = n; call->other = at(CL_STR_BINS - 1);
    call->delta = top - 63; call->count = (uint32_t)at(top); call->fwd = hist_fwd[top]; call->rev = hist_rev ? hist_rev[top] : 0u;
    call->delta2 = second - 63; call->count2 = (uint32_t)at(second);
    call->status = n < params->min_depth ? DUT_STR_LOW_DEPTH
                 : 10000ull * at(top) >= (uint64_t)params->min_allele_per_10k * n ? DUT_STR_CALLED : DUT_STR_MIXED;
    return CL_OK;
}

int dut_str_units(uint32_t span, int32_t delta, uint32_t period, char *buf)
{
    if (buf) buf[0] = 0;
    const int64_t len = (int64_t)span + delta;
    if (!buf || period < 1 || period > 255 || len < 0) return CL_ERR_INVALID;
    if (len % period) snprintf(buf, DUT_STR_UNITS_LEN, "%lld.%lld", (long long)(len / period), (long long)(len % period));
    else snprintf(buf, DUT_STR_UNITS_LEN, "%lld", (long long)(len / period));
    return CL_OK;
}

// a decimal number below 2^32 and nothing else
static bool str_number(const std::string &t, uint32_t &v)
{
    if (t.empty() || t.size() > 10) return false;
    uint64_t x = 0;
    for (char ch : t) { if (ch < '0' || ch > '9') return false; x = x * 10 + (uint64_t)(ch - '0'); }
    if (x > 0xFFFFFFFFull) return false;
    v = (uint32_t)x;
    return true;
}

int dut_str_loci_parse(const char *path, const char *contig, dut_str_locus **loci, size_t *n_loci, size_t *n_skipped, char *err, size_t err_len)
{
    if (loci) *loci = nullptr;
    if (n_loci) *n_loci = 0;
    if (n_skipped) *n_skipped = 0;
    return no_throw(err, err_len, [&]() -> int {
        if (!path || !contig || !loci || !n_loci || !n_skipped) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        FILE *f = fopen(path, "rb");
        if (!f) { set_err(err, err_len, std::string("cannot read the loci file ") + path); return CL_ERR_INVALID; }
        std::string text;
        char buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) { set_err(err, err_len, std::string("cannot read the loci file ") + path); return CL_ERR_INVALID; }
        std::vector<dut_str_locus> out;
        size_t skipped = 0, line_no = 0;
        for (size_t at = 0; at < text.size();) {
            size_t nl = text.find('\n', at);
            if (nl == std::string::npos) nl = text.size();
            std::string line = text.substr(at, nl - at);
            at = nl + 1;
            ++line_no;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty() || line[0] == '#') continue;
            std::vector<std::string> col;
            for (size_t a = 0; col.size() < 5;) {
                const size_t t = line.find('\t', a);
                col.push_back(line.substr(a, t == std::string::npos ? std::string::npos : t - a));
                if (t == std::string::npos) break;
                a = t + 1;
            }
            auto malformed = [&](const char *why) {
                set_err(err, err_len, std::string(path) + ": line " + std::to_string(line_no) + ": " + why);
                return CL_ERR_INVALID;
            };
            if (col.size() < 5) return malformed("fewer than five tab-separated columns (contig start end period name)");
            dut_str_locus l;
            memset(&l, 0, sizeof(l));
            if (col[0].empty()) return malformed("an empty contig");
            if (!str_number(col[1], l.start)) return malformed("start is not a decimal number below 2^32");
            if (!str_number(col[2], l.end)) return malformed("end is not a decimal number below 2^32");
            if (!str_number(col[3], l.period)) return malformed("period is not a decimal number");
            if (l.start >= l.end) return malformed("start >= end");
            if (l.period < 1 || l.period > 255) return malformed("period must lie in 1..255");
            if (col[4].empty() || col[4].size() >= sizeof(l.name)) return malformed("the name must have 1..63 bytes");
            if (col[0] != contig) { ++skipped; continue; }
            memcpy(l.name, col[4].data(), col[4].size());
            out.push_back(l);
        }
        if (!out.empty()) {
            dut_str_locus *p = (dut_str_locus *)malloc(out.size() * sizeof(dut_str_locus));
            if (!p) { set_err(err, err_len, "out of memory"); return CL_ERR_NOMEM; }
            memcpy(p, out.data(), out.size() * sizeof(dut_str_locus));
            *loci = p;
        }
        *n_loci = out.size(); *n_skipped = skipped;
        return CL_OK;
    });
}

void dut_str_loci_free(dut_str_locus *loci) { free(loci); }

int dut_str_write(const char *path, const char *contig, const dut_str_locus *loci, size_t n_loci, size_t n_skipped, const uint32_t *hist,
                  const uint32_t *partial, uint32_t strands, const dut_str_options *opt, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&]() -> int {
        if (!path || !contig || !opt || (n_loci && (!loci || !hist || !partial))) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        if (strands < 1 || strands > 2) { set_err(err, err_len, "strands must be 1 or 2"); return CL_ERR_INVALID; }
        if (!str_options_ok(*opt, err, err_len)) return CL_ERR_INVALID;
        const dut_str_params prm = {opt->min_depth, opt->min_allele_per_10k};
        const char *const STATUS[] = {"low_depth", "mixed", "called"};
        uint64_t n_class[3] = {0, 0, 0};
        std::string body;
        char b[768];
        for (size_t i = 0; i < n_loci; ++i) {
            const dut_str_locus &l = loci[i];
            const uint32_t *hf = hist + i * strands * CL_STR_BINS, *hr = strands == 2 ? hf + CL_STR_BINS : nullptr;
            dut_str_allele_call c;
            if (dut_str_call(hf, hr, &prm, &c) != CL_OK) { set_err(err, err_len, "calling a locus failed"); return CL_ERR_INVALID; }
            n_class[c.status] += 1;
            const uint32_t span = l.end - l.start;
            // (a bin without a read may stand for a length below zero: it is never printed)
            const bool has1 = c.status != DUT_STR_LOW_DEPTH && c.count > 0, has2 = c.count2 > 0;
            char ru[DUT_STR_UNITS_LEN], a1[DUT_STR_UNITS_LEN], a2[DUT_STR_UNITS_LEN], d1[16], d2[16];
            if (l.start >= l.end || dut_str_units(span, 0, l.period, ru) != CL_OK || (has1 && dut_str_units(span, c.delta, l.period, a1) != CL_OK) ||
                (has2 && dut_str_units(span, c.delta2, l.period, a2) != CL_OK)) {
                set_err(err, err_len, "locus " + std::to_string(i) + ": start >= end, a period outside 1..255 or reads in a bin below the locus's own length");
                return CL_ERR_INVALID;
            }
            snprintf(d1, sizeof(d1), c.delta ? "%+d" : "%d", c.delta);
            snprintf(d2, sizeof(d2), c.delta2 ? "%+d" : "%d", c.delta2);
            snprintf(b, sizeof(b), "%s\t%u\t%u\t%s\t%u\t%s\t%llu\t%u\t%llu\t%s", contig, l.start, l.end, l.name, l.period, ru, (unsigned long long)c.n,
                     partial[i], (unsigned long long)c.other, STATUS[c.status]);
            body += b;
            if (!has1) body += "\t.\t.\t.\t.\t.\t.";
            else { snprintf(b, sizeof(b), "\t%s\t%s\t%u\t%.4f\t%u\t%u", a1, d1, c.count, (double)c.count / (double)c.n, c.fwd, c.rev); body += b; }
            if (!has2) body += "\t.\t.\t.\n";
            else { snprintf(b, sizeof(b), "\t%s\t%s\t%u\n", a2, d2, c.count2); body += b; }
        }
        std::string s;
        snprintf(b, sizeof(b), "##contig=%s\n##loci=%llu\n##loci_skipped=%llu\n##flank=%u\n##min_depth=%u\n##min_quality=%u\n##exclude_flags=0x%04x\n"
                               "##min_allele_fraction=%.4f\n##low_depth=%llu\n##mixed=%llu\n##called=%llu\n",
                 contig, (unsigned long long)n_loci, (unsigned long long)n_skipped, opt->flank, opt->min_depth, (unsigned)opt->min_quality,
                 (unsigned)opt->exclude_flags, (double)opt->min_allele_per_10k / 10000.0, (unsigned long long)n_class[0], (unsigned long long)n_class[1],
                 (unsigned long long)n_class[2]);
        s += b;
        s += "#contig\tstart\tend\tname\tperiod\tref_units\tspanning\tpartial\tother\tstatus\tallele\tdelta\tcount\tfreq\tfwd\trev\tallele2\tdelta2\tcount2\n";
        s += body;
        return write_file(path, s, err, err_len);
    });
}

int dut_find_strs_files(const char *bam_path, const char *fasta_path, const char *contig, const char *loci_path, const dut_str_options *opt,
                        const char *output_path, int device_id, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&]() -> int {
        if (!bam_path || !fasta_path || !contig || !loci_path || !output_path || !opt) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        if (!str_options_ok(*opt, err, err_len)) return CL_ERR_INVALID;
        dut_str_locus *lp = nullptr; size_t n = 0, skipped = 0;
        int rc = dut_str_loci_parse(loci_path, contig, &lp, &n, &skipped, err, err_len);
        if (rc != CL_OK) return rc;
        std::unique_ptr<dut_str_locus, decltype(&dut_str_loci_free)> own(lp, dut_str_loci_free);
        ScanFiles F;
        uint32_t start = 0, end = 0;
        if ((rc = scan_files_open(F, bam_path, fasta_path, contig, 0, start, end, err, err_len)) != CL_OK) return rc;
        for (size_t i = 0; i < n; ++i)
            if (const char *why = str_locus_fault(lp[i].start, lp[i].end, F.contig_len)) {
                set_err(err, err_len, std::string("locus ") + lp[i].name + " [" + std::to_string(lp[i].start) + ", " + std::to_string(lp[i].end) + ") of " +
                                          contig + " (" + std::to_string(F.contig_len) + " bases): " + why);
                return CL_ERR_INVALID;
            }
        const FilterOptions flt = {0, 0, opt->exclude_flags};
        cl_scan_filter f;
        if ((rc = scan_files_resident(F, contig, device_id, &flt, f, []() {}, []() { return true; }, err, err_len)) != CL_OK) return rc;
        std::vector<uint32_t> hist(n * 2 * CL_STR_BINS), partial(n);
        std::vector<cl_str_locus> chunk;
        for (size_t at = 0; at < n; at += CL_STR_MAX_LOCI) {
            const size_t m = std::min<size_t>(n - at, CL_STR_MAX_LOCI);
            chunk.resize(m);
            for (size_t i = 0; i < m; ++i) chunk[i] = {lp[at + i].start, lp[at + i].end};
            cl_str_result res;
            rc = cl_site_str_lengths(F.ctx.get(), opt->min_quality, &f, opt->flank, chunk.data(), m, &res);
            if (rc != CL_OK) { F.engine_err(err, err_len, "measuring the loci failed"); return rc; }
            memcpy(hist.data() + at * 2 * CL_STR_BINS, res.hist, m * 2 * CL_STR_BINS * 4);
            memcpy(partial.data() + at, res.partial, m * 4);
        }
        return dut_str_write(output_path, contig, lp, n, skipped, hist.data(), partial.data(), 2, opt, err, err_len);
    });
}

// ---- error-profile ----
namespace {

// the counts of one thread's reads, in the result's layout: from5 and from3 [cycle][16], ins5, ins3, del5, del3 [cycle],
// then total[16], n_uncomparable, n_reads, n_ins, n_del, ins_bases, del_bases
struct EpCounts {
    uint32_t C;
    std::vector<uint64_t> w;
    explicit EpCounts(uint32_t c) : C(c), w((size_t)36 * c + 22, 0) {}
    uint64_t *tail() { return w.data() + (size_t)36 * C; }
};

// the host's sink of ep_walk_read: one caller sees every base and event of read r
struct EpHostSink {
    const dut_ep_reads &R;
    const uint8_t *ref;
    EpCounts &n;
    uint64_t r;
    uint32_t L, rev;
    bool use_bq;
    uint8_t thr;
    bool passes(uint32_t q) const
    {
        if (!use_bq) return true;
        const uint64_t nq = R.qual_off[r + 1] - R.qual_off[r];
        return q >= nq || R.qual[R.qual_off[r] + q] >= thr;
    }
    void cycles(uint64_t *t5, uint64_t *t3, uint32_t width, uint32_t col, uint32_t q) const
    {
        const uint32_t d5 = dut::ep_d5(q, L, rev), d3 = dut::ep_d3(q, L, rev);
        if (d5 < n.C) t5[(size_t)d5 * width + col] += 1;
        if (d3 < n.C) t3[(size_t)d3 * width + col] += 1;
    }
    void base(uint32_t p, uint32_t q) const
    {
        if (!passes(q)) return;
        const uint64_t bi = R.seq_off[r] + q;
        const uint32_t byte = R.seq4[bi >> 1], code = (bi & 1u) ? (byte & 15u) : (byte >> 4);
        const uint32_t cell = dut::ep_cell(code, ref[p], rev);
        n.tail()[cell] += 1;                                                    // (cell 16: n_uncomparable)
        if (cell < 16u) cycles(n.w.data(), n.w.data() + (size_t)16 * n.C, 16, cell, q);
    }
    void event(uint32_t which, uint32_t q, uint32_t l) const
    {
        if (!passes(q)) return;
        n.tail()[18 + which] += 1; n.tail()[20 + which] += l;
        uint64_t *e = n.w.data() + (size_t)(32 + 2 * which) * n.C;
        cycles(e, e + n.C, 1, 0, q);
    }
    void ins(uint32_t, uint32_t q, uint32_t l) const { event(0, q, l); }
    void del(uint32_t, uint32_t q, uint32_t l) const { event(1, q, l); }
};

bool ep_options_ok(const dut_ep_options &o, char *err, size_t err_len)
{
    if (o.n_cycles >= 1 && o.n_cycles <= CL_EP_MAX_CYCLES) return true;
    set_err(err, err_len, "n_cycles must lie in 1..256");
    return false;
}

} // namespace

int dut_error_profile_measure(const dut_ep_reads *reads, uint32_t contig_len, const uint8_t *ref_bases, uint64_t ref_len, uint32_t start, uint32_t end,
                              const dut_ep_options *opt, uint64_t *tables, cl_ep_result *out)
{
    return no_throw(nullptr, 0, [&]() -> int {
        if (!reads || !opt || !tables || !out || !ep_options_ok(*opt, nullptr, 0)) return CL_ERR_INVALID;
        const dut_ep_reads &R = *reads;
        const bool filtered = opt->filtered != 0, use_bq = filtered && opt->has_min_base_quality;
        if (start > end || end > contig_len || (!ref_bases && ref_len)) return CL_ERR_INVALID;
        if (R.n_reads && (!R.pos || !R.mapq || !R.cigar_off || !R.seq_off || (filtered && !R.flag) || (use_bq && !R.qual_off))) return CL_ERR_INVALID;
        for (uint64_t r = 0; r < R.n_reads; ++r)
            if (R.cigar_off[r + 1] < R.cigar_off[r] || R.seq_off[r + 1] < R.seq_off[r] || (use_bq && R.qual_off[r + 1] < R.qual_off[r])) return CL_ERR_INVALID;
        if (R.n_reads && ((R.cigar_off[R.n_reads] > R.cigar_off[0] && !R.cigar) || (R.seq_off[R.n_reads] > R.seq_off[0] && !R.seq4) ||
                          (use_bq && R.qual_off[R.n_reads] > R.qual_off[0] && !R.qual))) return CL_ERR_INVALID;
        const uint32_t C = opt->n_cycles;
        const uint32_t hi = (uint32_t)std::min<uint64_t>(end, ref_len);
        EpCounts sum(C);
        std::mutex mu;
        const size_t grain = dut::grain_for((size_t)R.n_reads, 1u << 14), chunks = ((size_t)R.n_reads + grain - 1) / grain;
        dut::parallel_for(start < hi ? chunks : 0, 1, [&](size_t ch) {
            EpCounts mine(C);
            for (uint64_t r = ch * grain, r1 = std::min<uint64_t>(R.n_reads, r + grain); r < r1; ++r) {
                const uint32_t x = (uint32_t)R.pos[r];
                if (x >= contig_len || x >= hi || R.mapq[r] < opt->min_quality) continue;
                if (filtered && (R.flag[r] & opt->exclude_flags)) continue;
                const uint32_t *cg = R.cigar + R.cigar_off[r];
                const uint32_t n_ops = R.cigar_off[r + 1] - R.cigar_off[r];
                uint64_t span = 0;
                for (uint32_t k = 0; k < n_ops; ++k) span += ((0x18Du >> (cg[k] & 15u)) & 1u) ? (cg[k] >> 4) : 0u;
                if (!span || (uint64_t)x + span <= start) continue;
                mine.tail()[17] += 1;
                const uint64_t L = R.seq_off[r + 1] - R.seq_off[r];
                const EpHostSink sink{R, ref_bases, mine, r, (uint32_t)std::min<uint64_t>(L, 0xFFFFFFFFull), filtered ? (uint32_t)(R.flag[r] >> 4) & 1u : 0u,
                                      use_bq, opt->min_base_quality};
                dut::ep_walk_read(x, cg, n_ops, sink.L, start, hi, 0, 1, sink);
            }
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < sum.w.size(); ++i) sum.w[i] += mine.w[i];
        });
        memset(out, 0, sizeof(*out));
        out->start = start; out->end = end; out->n_cycles = C;
        memcpy(tables, sum.w.data(), (size_t)36 * C * 8);
        out->from5 = tables; out->from3 = tables + (size_t)16 * C;
        out->ins5 = tables + (size_t)32 * C; out->ins3 = out->ins5 + C; out->del5 = out->ins3 + C; out->del3 = out->del5 + C;
        const uint64_t *t = sum.tail();
        for (int k = 0; k < 16; ++k) { out->total[k] = t[k]; out->n_bases += t[k]; }
        out->n_uncomparable = t[16]; out->n_reads = t[17]; out->n_ins = t[18]; out->n_del = t[19]; out->ins_bases = t[20]; out->del_bases = t[21];
        return CL_OK;
    });
}

int dut_error_profile_write(const char *path, const char *contig, const cl_ep_result *res, const dut_ep_options *opt, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&]() -> int {
        if (!path || !contig || !res || !opt) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        if (!ep_options_ok(*opt, err, err_len)) return CL_ERR_INVALID;
        const uint32_t C = res->n_cycles;
        if (C != opt->n_cycles) { set_err(err, err_len, "the result's n_cycles differs from the options'"); return CL_ERR_INVALID; }
        if (!res->from5 || !res->from3 || !res->ins5 || !res->ins3 || !res->del5 || !res->del3) { set_err(err, err_len, "null table"); return CL_ERR_INVALID; }
        auto rate = [](const uint64_t *cells) -> std::string {
            uint64_t all = 0, diag = 0;
            for (int k = 0; k < 16; ++k) { all += cells[k]; if (k % 5 == 0) diag += cells[k]; }
            if (!all) return "NA";
            char b[32];
            snprintf(b, sizeof(b), "%.6f", (double)(all - diag) / (double)all);
            return b;
        };
        uint64_t diag = 0;
        for (int k = 0; k < 16; k += 5) diag += res->total[k];
        char b[512], q[8] = ".";
        if (opt->has_min_base_quality) snprintf(q, sizeof(q), "%u", (unsigned)opt->min_base_quality);
        std::string s;
        snprintf(b, sizeof(b), "##contig=%s\n##range=%u-%u\n##cycles=%u\n##min_quality=%u\n##min_base_quality=%s\n##exclude_flags=0x%04x\n", contig, res->start, res->end,
                 C, (unsigned)opt->min_quality, q, (unsigned)opt->exclude_flags);
        s += b;
        snprintf(b, sizeof(b), "##reads=%llu\n##bases=%llu\n##uncomparable=%llu\n##mismatches=%llu\n##mismatch_rate=%s\n##insertions=%llu\n##inserted_bases=%llu\n"
                               "##deletions=%llu\n##deleted_bases=%llu\n", (unsigned long long)res->n_reads, (unsigned long long)res->n_bases,
                 (unsigned long long)res->n_uncomparable, (unsigned long long)(res->n_bases - diag), rate(res->total).c_str(), (unsigned long long)res->n_ins,
                 (unsigned long long)res->ins_bases, (unsigned long long)res->n_del, (unsigned long long)res->del_bases);
        s += b;
        s += "#table\tcycle";
        for (int f = 0; f < 4; ++f) for (int t = 0; t < 4; ++t) { s += '\t'; s += "ACGT"[f]; s += '>'; s += "ACGT"[t]; }
        s += "\tins\tdel\tmismatch_rate\n";
        auto line = [&](const char *table, const std::string &cycle, const uint64_t *cells, uint64_t n_ins, uint64_t n_del) {
            s += table; s += '\t'; s += cycle;
            for (int k = 0; k < 16; ++k) { s += '\t'; s += std::to_string(cells[k]); }
            s += '\t' + std::to_string(n_ins) + '\t' + std::to_string(n_del) + '\t' + rate(cells) + '\n';
        };
        line("total", ".", res->total, res->n_ins, res->n_del);
        for (uint32_t d = 0; d < C; ++d) line("5p", std::to_string(d + 1), res->from5 + (size_t)16 * d, res->ins5[d], res->del5[d]);
        for (uint32_t d = 0; d < C; ++d) line("3p", std::to_string(d + 1), res->from3 + (size_t)16 * d, res->ins3[d], res->del3[d]);
        return write_file(path, s, err, err_len);
    });
}

int dut_error_profile_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start, uint32_t end,
                            const dut_ep_options *opt, const char *output_path, int device_id, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&]() -> int {
        if (!bam_path || !fasta_path || !contig || !output_path || !opt) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        if (!ep_options_ok(*opt, err, err_len)) return CL_ERR_INVALID;
        ScanFiles F;
        int rc = scan_files_open(F, bam_path, fasta_path, contig, has_region, start, end, err, err_len);
        if (rc != CL_OK) return rc;
        const FilterOptions flt = {opt->has_min_base_quality, opt->min_base_quality, opt->exclude_flags};
        cl_scan_filter f;
        if ((rc = scan_files_resident(F, contig, device_id, &flt, f, []() {}, []() { return true; }, err, err_len)) != CL_OK) return rc;
        cl_ep_result res;
        rc = cl_site_error_profile(F.ctx.get(), opt->min_quality, &f, opt->n_cycles, F.bases, F.blen, start, end, &res);
        if (rc != CL_OK) { F.engine_err(err, err_len, "the error profile failed"); return rc; }
        return dut_error_profile_write(output_path, contig, &res, opt, err, err_len);
    });
}

// ---- phase-sites ----
namespace {

static_assert(CL_LINK_CLASSES == CL_LINK_WALK_CLASSES && CL_LINK_MAX_PARTNERS == CL_LINK_WALK_MAX_PARTNERS, "link_walk.h packs the observations of cl_link_result");

// the host's source of link_observe_read: the stored bases and quality values of read r
struct LinkHostSource {
    const dut_ep_reads &R;
    uint64_t r;
    bool use_bq;
    uint8_t thr;
    uint32_t code(uint32_t q) const
    {
        const uint64_t bi = R.seq_off[r] + q;
        const uint32_t byte = R.seq4[bi >> 1];
        return (bi & 1u) ? (byte & 15u) : (byte >> 4);
    }
    bool passes(uint32_t q) const
    {
        if (!use_bq) return true;
        const uint64_t nq = R.qual_off[r + 1] - R.qual_off[r];
        return q >= nq || R.qual[R.qual_off[r] + q] >= thr;
    }
};

bool link_options_ok(const dut_link_options &o, char *err, size_t err_len)
{
    char b[96] = {0};
    if (o.min_depth == 0) snprintf(b, sizeof(b), "min_depth must be at least 1");
    else if (o.max_dist == 0) snprintf(b, sizeof(b), "max_dist must be at least 1");
    else if (o.max_partners < 1 || o.max_partners > CL_LINK_MAX_PARTNERS) snprintf(b, sizeof(b), "max_partners must lie in 1..%u", (unsigned)CL_LINK_MAX_PARTNERS);
    else if (o.min_link_count == 0) snprintf(b, sizeof(b), "min_link_count must be at least 1");
    else if (o.max_discord_per_10k > 4999) snprintf(b, sizeof(b), "max_discord_per_10k must lie in 0..4999");
    else return true;
    set_err(err, err_len, b);
    return false;
}

// strictly ascending?  the index of the first site that is not, 0 when all are
size_t link_unsorted_at(const uint32_t *sites, size_t n)
{
    for (size_t i = 1; i < n; ++i) if (sites[i] <= sites[i - 1]) return i;
    return 0;
}

const char *const LINK_ALLELE[] = {"A", "C", "G", "T", "del"};
const char *const LINK_STATUS[] = {"low_depth", "cis", "trans", "unresolved"};

} // namespace

int dut_link_discordance_parse(const char *text, uint32_t *per_10k, char *err, size_t err_len)
{
    return fraction_parse(text, per_10k, 4999, "[0, 0.4999]", err, err_len, 0);
}

int dut_link_pair_offsets(const uint32_t *sites, size_t n_sites, uint32_t max_dist, uint32_t max_partners, uint32_t *first, uint64_t *n_pairs)
{
    if (n_pairs) *n_pairs = 0;
    if ((n_sites && !sites) || !n_pairs || max_dist == 0 || max_partners < 1 || max_partners > CL_LINK_MAX_PARTNERS) return CL_ERR_INVALID;
    if (link_unsorted_at(sites, n_sites)) return CL_ERR_INVALID;
    uint64_t at = 0;
    for (size_t i = 0; i < n_sites; ++i) {
        if (first) first[i] = (uint32_t)std::min<uint64_t>(at, 0xFFFFFFFFull);
        at += dut::link_partner_count(sites, n_sites, i, max_dist, max_partners);
    }
    if (first) first[n_sites] = (uint32_t)std::min<uint64_t>(at, 0xFFFFFFFFull);
    *n_pairs = at;
    return CL_OK;
}

int dut_link_measure(const dut_ep_reads *reads, uint32_t contig_len, const dut_link_options *opt, const uint32_t *sites, size_t n_sites,
                     uint32_t *first, uint32_t *tables, uint32_t *site_counts)
{
    return no_throw(nullptr, 0, [&]() -> int {
        if (!reads || !opt || !first || (n_sites && (!sites || !site_counts))) return CL_ERR_INVALID;
        const dut_ep_reads &R = *reads;
        const bool filtered = opt->filtered != 0, use_bq = filtered && opt->has_min_base_quality;
        if (n_sites > CL_LINK_MAX_SITES) return CL_ERR_INVALID;
        uint64_t n_pairs = 0;
        if (dut_link_pair_offsets(sites, n_sites, opt->max_dist, opt->max_partners, first, &n_pairs) != CL_OK || n_pairs > CL_LINK_MAX_PAIRS) return CL_ERR_INVALID;
        if (n_pairs && !tables) return CL_ERR_INVALID;
        if (n_sites && sites[n_sites - 1] >= contig_len) return CL_ERR_INVALID;
        if (R.n_reads > 0xFFFFFFF0ull) return CL_ERR_INVALID;
        if (R.n_reads && (!R.pos || !R.mapq || !R.cigar_off || !R.seq_off || (filtered && !R.flag) || (use_bq && !R.qual_off))) return CL_ERR_INVALID;
        for (uint64_t r = 0; r < R.n_reads; ++r)
            if (R.cigar_off[r + 1] < R.cigar_off[r] || R.seq_off[r + 1] < R.seq_off[r] || (use_bq && R.qual_off[r + 1] < R.qual_off[r])) return CL_ERR_INVALID;
        if (R.n_reads && ((R.cigar_off[R.n_reads] > R.cigar_off[0] && !R.cigar) || (R.seq_off[R.n_reads] > R.seq_off[0] && !R.seq4) ||
                          (use_bq && R.qual_off[R.n_reads] > R.qual_off[0] && !R.qual))) return CL_ERR_INVALID;
        // the reads of an anchor: per read its reference end (0: it never takes part), per window of kWin positions the range
        // of the reads that overlap it -- wider for an unsorted tile, exact all the same
        constexpr uint32_t kWin = 1024;
        const size_t n_win = ((size_t)contig_len + kWin - 1) / kWin;
        std::vector<uint32_t> rend(R.n_reads, 0), wfirst(n_win + 1, 0xFFFFFFFFu), wlast(n_win + 1, 0);
        for (uint64_t r = 0; r < R.n_reads; ++r) {
            const uint32_t x = (uint32_t)R.pos[r];
            if (x >= contig_len) continue;
            uint64_t span = 0;
            for (uint32_t k = R.cigar_off[r]; k < R.cigar_off[r + 1]; ++k) { const uint32_t c = R.cigar[k]; span += ((0x18Du >> (c & 15u)) & 1u) ? (c >> 4) : 0u; }
            if (!span) continue;
            const uint64_t xe = (uint64_t)x + span;
            rend[r] = xe > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)xe;
            const uint32_t last_p = std::min(rend[r], contig_len) - 1u;
            for (uint32_t w = x / kWin; w <= last_p / kWin; ++w) { wfirst[w] = std::min(wfirst[w], (uint32_t)r); wlast[w] = std::max(wlast[w], (uint32_t)r + 1u); }
        }
        dut::parallel_for(n_sites, 16, [&](size_t i) {
            const uint32_t a = sites[i], n_part = first[i + 1] - first[i];
            uint32_t *cnt = site_counts + i * CL_LINK_CLASSES;
            uint32_t *tab = n_part ? tables + (size_t)first[i] * 36 : nullptr;
            memset(cnt, 0, CL_LINK_CLASSES * 4);
            if (n_part) memset(tab, 0, (size_t)n_part * 36 * 4);
            for (uint32_t r = wfirst[a / kWin]; r < wlast[a / kWin]; ++r) {
                if (R.mapq[r] < opt->min_quality || rend[r] <= a || (uint32_t)R.pos[r] > a) continue;
                if (filtered && (R.flag[r] & opt->exclude_flags)) continue;
                const uint64_t L = R.seq_off[r + 1] - R.seq_off[r];
                const LinkHostSource src{R, r, use_bq, opt->min_base_quality};
                const uint64_t obs = dut::link_observe_read((uint32_t)R.pos[r], R.cigar + R.cigar_off[r], R.cigar_off[r + 1] - R.cigar_off[r],
                                                            (uint32_t)std::min<uint64_t>(L, 0xFFFFFFFFull), sites + i, n_part + 1u, src);
                const uint32_t ca = dut::link_obs(obs, 0);
                if (ca == LINK_NONE) continue;
                cnt[ca] += 1u;
                for (uint32_t j = 1; j <= n_part; ++j) {
                    const uint32_t cb = dut::link_obs(obs, j);
                    if (cb != LINK_NONE) tab[(size_t)(j - 1u) * 36 + 6u * ca + cb] += 1u;
                }
            }
        });
        return CL_OK;
    });
}

// cis and trans exclude each other.  cis asks mm >= 1 and 10000 (Mm + mM) <= d m; trans asks Mm, mM >= 1 and 10000 mm <= d m,
// with m = Mm + mM + mm >= 1 in both.  If both held, their sum would give 10000 m <= 2 d m, that is d >= 5000: with
// d = max_discord_per_10k <= 4999 it cannot.
int dut_link_summarise(const uint32_t *site_counts_a, const uint32_t *site_counts_b, const uint32_t *table, const dut_link_params *params, dut_link_summary *out)
{
    if (!site_counts_a || !site_counts_b || !table || !params || !out) return CL_ERR_INVALID;
    if (params->min_depth == 0 || params->min_link_count == 0 || params->max_discord_per_10k > 4999) return CL_ERR_INVALID;
    auto two = [](const uint32_t *c, uint8_t &major, uint8_t &minor) {
        major = 0;
        for (uint8_t k = 1; k < 5; ++k) if (c[k] > c[major]) major = k;          // the first among equals
        minor = major == 0 ? 1 : 0;
        for (uint8_t k = 0; k < 5; ++k) if (k != major && c[k] > c[minor]) minor = k;
    };
    memset(out, 0, sizeof(*out));
    two(site_counts_a, out->major_a, out->minor_a);
    two(site_counts_b, out->major_b, out->minor_b);
    for (int k = 0; k < CL_LINK_CLASSES; ++k) { out->depth_a += site_counts_a[k]; out->depth_b += site_counts_b[k]; }
    for (int k = 0; k < 36; ++k) out->both += table[k];
    out->MM = table[6 * out->major_a + out->major_b]; out->Mm = table[6 * out->major_a + out->minor_b];
    out->mM = table[6 * out->minor_a + out->major_b]; out->mm = table[6 * out->minor_a + out->minor_b];
    const uint64_t n4 = out->MM + out->Mm + out->mM + out->mm, m = out->Mm + out->mM + out->mm;
    const uint64_t d = params->max_discord_per_10k, k = params->min_link_count;     // (counts below 2^32: every product fits 64 bits)
    out->other = out->both - n4;
    out->status = n4 < params->min_depth ? DUT_LINK_LOW_DEPTH
                : (out->mm >= k && 10000ull * (out->Mm + out->mM) <= d * m) ? DUT_LINK_CIS
                : (out->Mm >= k && out->mM >= k && 10000ull * out->mm <= d * m) ? DUT_LINK_TRANS : DUT_LINK_UNRESOLVED;
    return CL_OK;
}

int dut_link_sites_parse(const char *path, const char *contig, uint32_t **sites, size_t *n_sites, size_t *n_skipped, char *err, size_t err_len)
{
    if (sites) *sites = nullptr;
    if (n_sites) *n_sites = 0;
    if (n_skipped) *n_skipped = 0;
    return no_throw(err, err_len, [&]() -> int {
        if (!path || !contig || !sites || !n_sites || !n_skipped) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        FILE *f = fopen(path, "rb");
        if (!f) { set_err(err, err_len, std::string("cannot read the sites file ") + path); return CL_ERR_INVALID; }
        std::string text;
        char buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) { set_err(err, err_len, std::string("cannot read the sites file ") + path); return CL_ERR_INVALID; }
        std::vector<uint32_t> out;
        size_t skipped = 0, line_no = 0;
        for (size_t at = 0; at < text.size();) {
            size_t nl = text.find('\n', at);
            if (nl == std::string::npos) nl = text.size();
            std::string line = text.substr(at, nl - at);
            at = nl + 1;
            ++line_no;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty() || line[0] == '#') continue;
            auto malformed = [&](const char *why) {
                set_err(err, err_len, std::string(path) + ": line " + std::to_string(line_no) + ": " + why);
                return CL_ERR_INVALID;
            };
            const size_t t1 = line.find('\t');
            if (t1 == std::string::npos) return malformed("fewer than two tab-separated columns (contig position)");
            const size_t t2 = line.find('\t', t1 + 1);
            const std::string name = line.substr(0, t1), num = line.substr(t1 + 1, t2 == std::string::npos ? std::string::npos : t2 - t1 - 1);
            uint32_t pos1 = 0;
            if (name.empty()) return malformed("an empty contig");
            if (!str_number(num, pos1) || pos1 == 0) return malformed("the position is not a 1-based decimal number below 2^32");
            if (name != contig) { ++skipped; continue; }
            out.push_back(pos1 - 1u);
        }
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
        if (!out.empty()) {
            uint32_t *p = (uint32_t *)malloc(out.size() * sizeof(uint32_t));
            if (!p) { set_err(err, err_len, "out of memory"); return CL_ERR_NOMEM; }
            memcpy(p, out.data(), out.size() * sizeof(uint32_t));
            *sites = p;
        }
        *n_sites = out.size(); *n_skipped = skipped;
        return CL_OK;
    });
}

void dut_link_sites_free(uint32_t *sites) { free(sites); }

int dut_link_write(const char *path, const char *contig, const uint32_t *sites, size_t n_sites, size_t n_skipped, const uint32_t *first,
                   const uint32_t *tables, const uint32_t *site_counts, const dut_link_options *opt, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&]() -> int {
        if (!path || !contig || !opt || !first || (n_sites && (!sites || !site_counts))) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        if (!link_options_ok(*opt, err, err_len)) return CL_ERR_INVALID;
        uint64_t n_pairs = 0;
        std::vector<uint32_t> own(n_sites + 1);
        if (dut_link_pair_offsets(sites, n_sites, opt->max_dist, opt->max_partners, own.data(), &n_pairs) != CL_OK) {
            set_err(err, err_len, "the sites must be strictly ascending"); return CL_ERR_INVALID;
        }
        if (memcmp(own.data(), first, (n_sites + 1) * 4) != 0) { set_err(err, err_len, "first is not the pair set of these sites under max_dist and max_partners"); return CL_ERR_INVALID; }
        if (n_pairs && !tables) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        const dut_link_params prm = {opt->min_depth, opt->min_link_count, opt->max_discord_per_10k};
        uint64_t n_class[4] = {0, 0, 0, 0};
        std::string body;
        char b[768];
        for (size_t i = 0; i < n_sites; ++i)
            for (uint32_t p = first[i]; p < first[i + 1]; ++p) {
                const size_t j = i + 1 + (p - first[i]);
                dut_link_summary u;
                if (dut_link_summarise(site_counts + i * 6, site_counts + j * 6, tables + (size_t)p * 36, &prm, &u) != CL_OK) { set_err(err, err_len, "summarising a pair failed"); return CL_ERR_INVALID; }
                n_class[u.status] += 1;
                snprintf(b, sizeof(b), "%s\t%llu\t%llu\t%u\t%s\t%s\t%s\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%s\n", contig,
                         (unsigned long long)sites[i] + 1ull, (unsigned long long)sites[j] + 1ull, sites[j] - sites[i], LINK_ALLELE[u.major_a], LINK_ALLELE[u.minor_a],
                         LINK_ALLELE[u.major_b], LINK_ALLELE[u.minor_b], (unsigned long long)u.depth_a, (unsigned long long)u.depth_b, (unsigned long long)u.both,
                         (unsigned long long)u.MM, (unsigned long long)u.Mm, (unsigned long long)u.mM, (unsigned long long)u.mm, (unsigned long long)u.other,
                         LINK_STATUS[u.status]);
                body += b;
            }
        char q[8] = ".";
        if (opt->has_min_base_quality) snprintf(q, sizeof(q), "%u", (unsigned)opt->min_base_quality);
        std::string s;
        snprintf(b, sizeof(b), "##contig=%s\n##sites=%llu\n##sites_skipped=%llu\n##pairs=%llu\n##max_dist=%u\n##max_partners=%u\n##min_depth=%u\n##min_quality=%u\n"
                               "##min_base_quality=%s\n##exclude_flags=0x%04x\n##min_link_count=%u\n##max_discordance=%.4f\n"
                               "##low_depth=%llu\n##cis=%llu\n##trans=%llu\n##unresolved=%llu\n",
                 contig, (unsigned long long)n_sites, (unsigned long long)n_skipped, (unsigned long long)n_pairs, opt->max_dist, opt->max_partners, opt->min_depth,
                 (unsigned)opt->min_quality, q, (unsigned)opt->exclude_flags, opt->min_link_count, (double)opt->max_discord_per_10k / 10000.0,
                 (unsigned long long)n_class[0], (unsigned long long)n_class[1], (unsigned long long)n_class[2], (unsigned long long)n_class[3]);
        s += b;
        s += "#contig\tpos_a\tpos_b\tdist\tmajor_a\tminor_a\tmajor_b\tminor_b\tdepth_a\tdepth_b\tboth\tMM\tMm\tmM\tmm\tother\tstatus\n";
        s += body;
        return write_file(path, s, err, err_len);
    });
}

int dut_find_links_files(const char *bam_path, const char *fasta_path, const char *contig, const char *sites_path, const dut_link_options *opt,
                         const char *output_path, int device_id, char *err, size_t err_len)
{
    return no_throw(err, err_len, [&]() -> int {
        if (!bam_path || !fasta_path || !contig || !sites_path || !output_path || !opt) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
        if (!link_options_ok(*opt, err, err_len)) return CL_ERR_INVALID;
        uint32_t *sp = nullptr; size_t n = 0, skipped = 0;
        int rc = dut_link_sites_parse(sites_path, contig, &sp, &n, &skipped, err, err_len);
        if (rc != CL_OK) return rc;
        std::unique_ptr<uint32_t, decltype(&dut_link_sites_free)> own(sp, dut_link_sites_free);
        ScanFiles F;
        uint32_t start = 0, end = 0;
        if ((rc = scan_files_open(F, bam_path, fasta_path, contig, 0, start, end, err, err_len)) != CL_OK) return rc;
        if (n > CL_LINK_MAX_SITES) { set_err(err, err_len, std::to_string(n) + " sites, more than " + std::to_string(CL_LINK_MAX_SITES)); return CL_ERR_INVALID; }
        if (n && sp[n - 1] >= F.contig_len) {
            set_err(err, err_len, "site " + std::to_string((unsigned long long)sp[n - 1] + 1ull) + " lies beyond contig " + contig + " (" + std::to_string(F.contig_len) + " bases)");
            return CL_ERR_INVALID;
        }
        uint64_t n_pairs = 0;
        if ((rc = dut_link_pair_offsets(sp, n, opt->max_dist, opt->max_partners, nullptr, &n_pairs)) != CL_OK) { set_err(err, err_len, "the pair set could not be formed"); return rc; }
        if (n_pairs > CL_LINK_MAX_PAIRS) { set_err(err, err_len, std::to_string(n_pairs) + " pairs, more than " + std::to_string(CL_LINK_MAX_PAIRS) + ": lower --max-dist or --max-partners"); return CL_ERR_INVALID; }
        const FilterOptions flt = {opt->has_min_base_quality, opt->min_base_quality, opt->exclude_flags};
        cl_scan_filter f;
        if ((rc = scan_files_resident(F, contig, device_id, &flt, f, []() {}, []() { return true; }, err, err_len)) != CL_OK) return rc;
        cl_link_result res;
        rc = cl_site_link_counts(F.ctx.get(), opt->min_quality, &f, sp, n, opt->max_dist, opt->max_partners, &res);
        if (rc != CL_OK) { F.engine_err(err, err_len, "counting the linked sites failed"); return rc; }
        return dut_link_write(output_path, contig, sp, n, skipped, res.first, res.tables, res.site_counts, opt, err, err_len);
    });
}

} // extern "C"
