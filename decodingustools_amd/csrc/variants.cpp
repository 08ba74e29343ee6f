// variants.cpp -- implementation of include/dut_variants.h: the per-position classification in plain C++ (the f64 rule
// the device's integer test is held against), the annotation of candidates against a haplogroup tree, the TSV of
// `find-variants`.  Host-only except dut_find_variants_files(_ex), which runs the device engine's cl_site_scan(_ex).
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

// opt: the extended TSV of dut_variants_write_ex (Res = cl_scan_result_ex); nullptr: the one of dut_variants_write
template <class Res>
int write_tsv(const char *path, const char *contig, const Res *res, uint32_t min_depth, uint8_t min_quality,
              const dut_variants_options *opt, const dut_variant_note *notes, char *err, size_t err_len)
{
    if (!path || !contig || !res || (res->n_variant && !res->candidates)) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    std::string s;
    char b[512];
    snprintf(b, sizeof(b), "##contig=%s\n##range=%u-%u\n##min_depth=%u\n##min_quality=%u\n", contig, res->start, res->end,
             min_depth, (unsigned)min_quality);
    s += b;
    if (opt) {
        if (opt->has_min_base_quality) snprintf(b, sizeof(b), "##min_base_quality=%u\n##exclude_flags=0x%04x\n", (unsigned)opt->min_base_quality, (unsigned)opt->exclude_flags);
        else snprintf(b, sizeof(b), "##min_base_quality=.\n##exclude_flags=0x%04x\n", (unsigned)opt->exclude_flags);
        s += b;
    }
    snprintf(b, sizeof(b), "##positions=%u\n", res->end - res->start);
    s += b;
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
    FILE *f = fopen(path, "wb");
    if (!f) { set_err(err, err_len, std::string("cannot create ") + path); return CL_ERR_INVALID; }
    const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
    if (fclose(f) != 0 || !ok) { set_err(err, err_len, std::string("cannot write ") + path); return CL_ERR_INVALID; }
    return CL_OK;
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

static int dut_find_variants_files_impl(const char *bam_path, const char *fasta_path, const char *contig, int has_region,
                                        uint32_t start, uint32_t end, const char *tree_json_path, int provider, int tree_type,
                                        const char *output_path, uint32_t min_depth, uint8_t min_quality,
                                        const dut_variants_options *vopt, int device_id, char *err, size_t err_len)
{
    if (!bam_path || !fasta_path || !contig || !output_path) { set_err(err, err_len, "null argument"); return CL_ERR_INVALID; }
    if (min_depth == 0) { set_err(err, err_len, "min_depth must be at least 1"); return CL_ERR_INVALID; }
    if (has_region && start >= end) { set_err(err, err_len, "the region is empty"); return CL_ERR_INVALID; }
    char e[512] = {0};
    std::unique_ptr<dut_fasta, decltype(&dut_fasta_close)> fa(dut_fasta_open(fasta_path, e, sizeof(e)), dut_fasta_close);
    if (!fa) { set_err(err, err_len, e); return CL_ERR_INVALID; }
    std::unique_ptr<dut_bam, decltype(&dut_bam_close)> bam(dut_bam_open(bam_path, e, sizeof(e)), dut_bam_close);
    if (!bam) { set_err(err, err_len, e); return CL_ERR_INVALID; }
    if (!dut_bam_has_index(bam.get())) { set_err(err, err_len, std::string("no .bai or .csi index beside ") + bam_path); return CL_ERR_INVALID; }
    int tid = -1;
    for (int t = 0; t < dut_bam_n_ref(bam.get()); ++t) if (strcmp(dut_bam_ref_name(bam.get(), t), contig) == 0) { tid = t; break; }
    if (tid < 0) { set_err(err, err_len, std::string("contig ") + contig + " is not in the BAM header"); return CL_ERR_INVALID; }
    const uint32_t contig_len = dut_bam_ref_len(bam.get(), tid);
    if (!has_region) { start = 0; end = contig_len; }
    if (end > contig_len) { set_err(err, err_len, "the region ends beyond contig " + std::string(contig) + " (" + std::to_string(contig_len) + " bases)"); return CL_ERR_INVALID; }
    // the build id the tree's coordinates are looked up by (mod.rs:51-54): the genome the header names, rCRS for mt
    std::string build;
    if (tree_json_path) {
        size_t tl = 0;
        const char *text = dut_bam_header_text(bam.get(), &tl);
        build = dut_reference_build(text, tl);
        if (build == "Unknown") { set_err(err, err_len, "Could not determine reference genome from BAM header"); return CL_ERR_INVALID; }
        if (tree_type == DUT_TREE_MTDNA) build = "rCRS";
    }
    // side by side, as dut_find_branch_files does: the tree JSON, the HIP runtime + context, the contig's records
    std::unique_ptr<dut_tree, decltype(&dut_tree_free)> tree(nullptr, dut_tree_free);
    std::unique_ptr<cl_ctx, decltype(&cl_destroy)> ctx(nullptr, cl_destroy);
    char terr[512] = {0};
    int crc = CL_OK;
    cl_options opt = {4, 500, 10, 20, 10, 1, 0.1};
    dut::Thread tt = dut::spawn_or_run([&]() { if (tree_json_path) tree.reset(dut_tree_load(tree_json_path, provider, tree_type, terr, sizeof(terr))); });
    dut::Thread ct = dut::spawn_or_run([&]() { cl_ctx *c = nullptr; crc = cl_create(&opt, device_id, nullptr, &c); ctx.reset(c); });
    dut_records rec{}; const uint64_t *seq_off = nullptr; const uint8_t *seq4 = nullptr;
    const int brc = dut_bam_read_contig(bam.get(), tid, &rec, &seq_off, &seq4);
    const uint8_t *bases = nullptr; uint64_t blen = 0;
    const int frc = dut_fasta_fetch(fa.get(), contig, &bases, &blen);
    if (tt.joinable()) tt.join();
    if (ct.joinable()) ct.join();
    if (frc != CL_OK) { set_err(err, err_len, dut_fasta_error(fa.get())); return frc; }
    if (tree_json_path && !tree) { set_err(err, err_len, terr); return CL_ERR_INVALID; }
    if (brc != CL_OK) { set_err(err, err_len, dut_bam_error(bam.get())); return brc; }
    if (crc != CL_OK) { set_err(err, err_len, "no usable HIP device (the engine has no CPU fallback)"); return crc; }
    cl_site_tile tile;
    tile.n_reads = rec.n; tile.pos = rec.pos; tile.mapq = rec.mapq; tile.cigar_off = rec.cigar_off; tile.cigar = rec.cigar;
    tile.seq_off = seq_off; tile.seq4 = seq4;
    auto engine_err = [&](const char *what) { const char *m = cl_last_error(ctx.get()); set_err(err, err_len, (m && *m) ? m : what); };
    int rc = cl_site_upload(ctx.get(), contig_len, blen, &tile);
    if (rc != CL_OK) { engine_err("site upload failed"); return rc; }
    // scan result -> annotation -> TSV, for either result type (wopt: the filter columns of the header, or none)
    auto finish = [&](int scan_rc, const auto &res, const dut_variants_options *wopt) {
        if (scan_rc != CL_OK) { engine_err("site scan failed"); return scan_rc; }
        dut_variant_note *notes = nullptr;
        if (tree) {
            const int arc = annotate(tree.get(), build.c_str(), contig, res.candidates, (size_t)res.n_variant, &notes);
            if (arc != CL_OK) { set_err(err, err_len, "annotation failed"); return arc; }
        }
        const int wrc = write_tsv(output_path, contig, &res, min_depth, min_quality, wopt, notes, err, err_len);
        dut_variants_free_notes(notes, (size_t)res.n_variant);
        return wrc;
    };
    if (vopt && vopt->filtered) {
        cl_site_quals q;
        q.n_reads = rec.n; q.flag = rec.flag; q.qual_off = rec.qual_off; q.qual = rec.qual; q.seq_off = seq_off;
        rc = cl_site_attach_quals(ctx.get(), &q, vopt->has_min_base_quality ? vopt->min_base_quality : 0);
        if (rc != CL_OK) { engine_err("site attachment failed"); return rc; }
        const cl_scan_filter flt = {vopt->exclude_flags, (uint8_t)(vopt->has_min_base_quality ? 1 : 0), 0};
        cl_scan_result_ex res;
        return finish(cl_site_scan_ex(ctx.get(), min_quality, min_depth, &flt, bases, blen, start, end, &res), res, vopt);
    }
    cl_scan_result res;
    return finish(cl_site_scan(ctx.get(), min_quality, min_depth, bases, blen, start, end, &res), res, nullptr);
}

int dut_find_variants_files_ex(const char *bam_path, const char *fasta_path, const char *contig, int has_region,
                               uint32_t start, uint32_t end, const char *tree_json_path, int provider, int tree_type,
                               const char *output_path, uint32_t min_depth, uint8_t min_quality,
                               const dut_variants_options *opt, int device_id, char *err, size_t err_len)
{
    // no exception leaves the library through the C ABI
    try { return dut_find_variants_files_impl(bam_path, fasta_path, contig, has_region, start, end, tree_json_path, provider, tree_type,
                                               output_path, min_depth, min_quality, opt, device_id, err, err_len); }
    catch (const std::bad_alloc &) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_NOMEM; }
    catch (...) { set_err(err, err_len, "out of memory or internal error"); return CL_ERR_INVALID; }
}

int dut_find_variants_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region,
                            uint32_t start, uint32_t end, const char *tree_json_path, int provider, int tree_type,
                            const char *output_path, uint32_t min_depth, uint8_t min_quality, int device_id,
                            char *err, size_t err_len)
{
    return dut_find_variants_files_ex(bam_path, fasta_path, contig, has_region, start, end, tree_json_path, provider, tree_type,
                                      output_path, min_depth, min_quality, nullptr, device_id, err, err_len);
}

} // extern "C"
