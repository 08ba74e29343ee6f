/*
 * dut_variants.h -- the plumbing around the dense site scan (cl_site_scan) of `find-variants`: where does the sample
 * differ from the reference at all, and which of those differences does the haplogroup tree not know.
 *
 * The reference has no such subcommand.  The counting and the call are the ones of find-y-branch / find-mt-branch
 * (haplogroup::caller::process_region, src/haplogroup/caller.rs:62-152), taken at every position of a contig or a
 * region instead of at the tree's sites, so the two never disagree about a tree site.  find-variants itself calls SNVs
 * only; deletions are counted and called per position by find-deletions and insertions by find-insertions (both below);
 * the sample's sequence itself is written by `consensus` (at the end of this header).  With dut_variants_options the scan takes a flag mask and a base-quality threshold
 * (cl_site_scan_ex) and the TSV carries per-strand allele counts and a strand filter.
 */
#ifndef DUT_VARIANTS_H
#define DUT_VARIANTS_H

#include "dut_haplogroup.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The classes of cl_site_scan (include/callable_loci.h). */
enum { DUT_SCAN_LOW_DEPTH = 0, DUT_SCAN_MIXED = 1, DUT_SCAN_UNCOMPARABLE = 2, DUT_SCAN_MATCH = 3, DUT_SCAN_VARIANT = 4,
       DUT_SCAN_UNDETERMINED = 5 };

/* One position in plain C++, no device, with the f64 rule of caller.rs:132-149 as dut_call_sites takes it:
 * depth = sum of the 16 codes, called <=> depth >= min_depth && (largest as f64 / depth as f64) >= 0.7.
 * ref_byte: the FASTA byte, case preserved (anything but ACGTacgt is "other"; pass 'N' beyond the reference).
 * *called (may be NULL): the called base ("=ACMGRSVTWYHKDBN") or 0 when there is no call. */
int dut_scan_classify(const uint32_t hist16[16], uint8_t ref_byte, uint32_t min_depth, char *called);
/* The same from the five counters of cl_site_scan_counts (a, c, g, t, depth).  The codes that are not A/C/G/T are only
 * known by their sum: when that sum reaches 0.7 of the depth the position is uncomparable if one code holds it and
 * mixed if several share it, which five counters cannot tell -- DUT_SCAN_UNDETERMINED. */
int dut_scan_classify_counts(const uint32_t counts5[5], uint8_t ref_byte, uint32_t min_depth, char *called);

/* What the tree knows about a candidate.  known = 1 when the tree has a SNP locus with coordinates for build_id on
 * `chromosome` at the position (the "relevant" of dut_tree_collect_sites); then names = the loci's names, ascending,
 * comma separated, and alleles = per locus, in that order, whether alt is its derived allele, its ancestral allele or
 * neither: "derived" / "ancestral" / "other".  known = 0 (novel): both NULL. */
typedef struct dut_variant_note {
    int   known;
    char *names;
    char *alleles;
} dut_variant_note;
int dut_variants_annotate(const dut_tree *t, const char *build_id, const char *chromosome,
                          const cl_scan_candidate *candidates, size_t n, dut_variant_note **notes);
void dut_variants_free_notes(dut_variant_note *notes, size_t n);

/* The TSV: comment lines ##contig= ##range=start-end (0-based half open) ##min_depth= ##min_quality= ##positions=
 * ##low_depth= ##mixed= ##uncomparable= ##match= ##variant=, the header
 *   #contig pos ref alt depth A C G T freq status names alleles
 * and one line per candidate: pos 1-based, freq = alt count / depth in f64 as %.4f, status novel | known.
 * notes == NULL (no tree was given): status, names and alleles are all "."; a novel candidate has names and alleles ".". */
int dut_variants_write(const char *path, const char *contig, const cl_scan_result *res, uint32_t min_depth,
                       uint8_t min_quality, const dut_variant_note *notes, char *err, size_t err_len);

/* `find-variants` on files, one GPU: open the BAM (its index is required) and the FASTA, read the contig's records,
 * cl_site_upload, cl_site_scan over the region (has_region == 0: the whole contig), annotate against the tree
 * (tree_json_path may be NULL: no annotation), write the TSV.  Errors with a message: an unknown contig, a region
 * that is empty or ends beyond the contig, min_depth == 0, with a tree a BAM header that does not name its genome. */
int dut_find_variants_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region,
                            uint32_t start, uint32_t end, const char *tree_json_path, int provider, int tree_type,
                            const char *output_path, uint32_t min_depth, uint8_t min_quality, int device_id,
                            char *err, size_t err_len);

/* ---- the filtered, strand-aware form ------------------------------------------------------------------------ */
/* filtered == 0: the unfiltered scan and the TSV above, the other fields are ignored.  Otherwise the scan is
 * cl_site_scan_ex with exclude_flags and, when has_min_base_quality, the pass bits of min_base_quality; a candidate whose
 * alternative base has fewer than min_alt_per_strand observations on either strand is marked, not dropped. */
typedef struct dut_variants_options {
    int      filtered;
    int      has_min_base_quality;
    uint8_t  min_base_quality;
    uint16_t exclude_flags;
    uint32_t min_alt_per_strand;
} dut_variants_options;

/* dut_variants_annotate for the candidates of cl_site_scan_ex. */
int dut_variants_annotate_ex(const dut_tree *t, const char *build_id, const char *chromosome,
                             const cl_scan_candidate_ex *candidates, size_t n, dut_variant_note **notes);

/* The extended TSV (no device needed): the comment lines of dut_variants_write with ##min_base_quality= ("." when
 * !has_min_base_quality) and ##exclude_flags=0x%04x after ##min_quality=, the header
 *   #contig pos ref alt depth A C G T freq status names alleles alt_fwd alt_rev ref_fwd ref_rev filter
 * and per candidate filter = "strand" when min(alt_fwd, alt_rev) < min_alt_per_strand, else "PASS".  ##variant= is the
 * scan's count: marked candidates stay in the file. */
int dut_variants_write_ex(const char *path, const char *contig, const cl_scan_result_ex *res, uint32_t min_depth,
                          uint8_t min_quality, const dut_variants_options *opt, const dut_variant_note *notes,
                          char *err, size_t err_len);

/* dut_find_variants_files with options (NULL or filtered == 0: exactly that call).  With a filter: cl_site_upload,
 * cl_site_attach_quals with the records' flags and qualities, cl_site_scan_ex, dut_variants_write_ex. */
int dut_find_variants_files_ex(const char *bam_path, const char *fasta_path, const char *contig, int has_region,
                               uint32_t start, uint32_t end, const char *tree_json_path, int provider, int tree_type,
                               const char *output_path, uint32_t min_depth, uint8_t min_quality,
                               const dut_variants_options *opt, int device_id, char *err, size_t err_len);

/* ---- find-minor-alleles: a second allele beside the most frequent one (cl_site_scan_minor) ------------------------- */
/* The classes of cl_site_scan_minor. */
enum { DUT_MINOR_LOW_DEPTH = 0, DUT_MINOR_SINGLE = 1, DUT_MINOR_MINOR = 2 };

/* Decimal text to parts per 10 000, exactly: digits, optionally '.' and at most four decimals ("0.05" -> 500, "0.5" ->
 * 5000, ".0125" -> 125).  The value must lie in (0, 0.5]; no sign, no exponent, nothing after the number. */
int dut_minor_fraction_parse(const char *text, uint32_t *per_10k, char *err, size_t err_len);

/* The rule of cl_site_scan_minor for one position in plain C++, with the same integer comparison: the class, and in
 * *major / *minor (may be NULL) the two bases.  depth is the depth of the scan there (a + c + g + t and every other
 * code).  CL_ERR_INVALID: null or refused params (as cl_site_scan_minor refuses them), a + c + g + t > depth,
 * depth >= 2^32. */
int dut_minor_classify_counts(uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint64_t depth, const cl_minor_params *params,
                              char *major, char *minor);

/* What a find-minor-alleles run is asked: the scan's parameters and filter, and the strand mark of the TSV. */
typedef struct dut_minor_options {
    uint32_t min_depth;
    uint8_t  min_quality;
    int      has_min_base_quality;
    uint8_t  min_base_quality;
    uint16_t exclude_flags;
    uint32_t min_minor_per_10k;       /* 1..5000 */
    uint32_t min_minor_count;         /* >= 1 */
    uint32_t min_minor_per_strand;    /* K: filter = "strand" when min(minor_fwd, minor_rev) < K; 0: always PASS */
} dut_minor_options;

/* The TSV (no device needed): comment lines ##contig= ##range=start-end ##min_depth= ##min_quality= ##min_base_quality=
 * ("." when !has_min_base_quality) ##exclude_flags=0x%04x ##min_minor_fraction=%.4f ##min_minor_count= ##positions=
 * ##low_depth= ##single= ##minor=, the header
 *   #contig pos ref major minor depth A C G T minor_freq major_fwd major_rev minor_fwd minor_rev filter
 * and one line per candidate: minor_freq = c2 / depth as %.4f.  ##minor= is the scan's count: marked lines stay. */
int dut_minor_write(const char *path, const char *contig, const cl_minor_result *res, const dut_minor_options *opt,
                    char *err, size_t err_len);

/* `find-minor-alleles` on files, one GPU: reads as dut_find_variants_files_ex does, always attaches the records' flags
 * and pass bits and runs the filtered form of cl_site_scan_minor (with no mask and no threshold it counts what the
 * unfiltered form does), writes the TSV.  Errors with a message: those of dut_find_variants_files, refused options. */
int dut_find_minor_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start,
                         uint32_t end, const dut_minor_options *opt, const char *output_path, int device_id,
                         char *err, size_t err_len);

/* ---- find-deletions: per-position deletion counts and calls (cl_site_scan_dels) ------------------------------------ */
/* The classes of cl_site_scan_dels. */
enum { DUT_DEL_LOW_DEPTH = 0, DUT_DEL_KEPT = 1, DUT_DEL_DELETED = 2 };

/* Decimal text to parts per 10 000, exactly, as dut_minor_fraction_parse takes it ("0.7" -> 7000, "1" -> 10000,
 * ".0001" -> 1).  The value must lie in (0, 1]. */
int dut_del_fraction_parse(const char *text, uint32_t *per_10k, char *err, size_t err_len);

/* The rule of cl_site_scan_dels for one position in plain C++, with the same integer comparison: span = del + depth;
 * low_depth when span < min_depth; deleted when del >= min_del_count and 10000 * del >= min_del_per_10k * span (in 64
 * bits); kept otherwise.  CL_ERR_INVALID: null or refused params (as cl_site_scan_dels refuses them). */
int dut_del_classify_counts(uint32_t del, uint32_t depth, const cl_del_params *params);

/* One deletion event: a maximal run of consecutive candidate positions (runs end at the range's borders, where the
 * candidates do).  start .. end are 1-based, inclusive; length = end - start + 1.  q is the position of the run where
 * del is smallest, the first among equals: del, span = del + depth, del_fwd, del_rev are those of q.  max_del is the
 * largest del of the run. */
typedef struct dut_del_event {
    uint32_t start, end, length;
    uint32_t q;
    uint32_t del, del_fwd, del_rev, max_del;
    uint64_t span;
} dut_del_event;

/* Merges candidates (ascending position, as cl_site_scan_dels returns them) into events.  *events: malloc'ed, release
 * with dut_del_events_free (NULL when there is none).  CL_ERR_INVALID: null argument, positions not ascending. */
int dut_del_events(const cl_del_candidate *candidates, size_t n, dut_del_event **events, size_t *n_events);
void dut_del_events_free(dut_del_event *events);

/* What a find-deletions run is asked: the scan's parameters and filter, and the strand mark of the TSV. */
typedef struct dut_del_options {
    uint32_t min_depth;
    uint8_t  min_quality;
    int      has_min_base_quality;
    uint8_t  min_base_quality;
    uint16_t exclude_flags;
    uint32_t min_del_per_10k;         /* 1..10000 */
    uint32_t min_del_count;           /* >= 1 */
    uint32_t min_del_per_strand;      /* K: filter = "strand" when min(del_fwd, del_rev) < K; 0: always PASS */
} dut_del_options;

/* The TSV (no device needed): comment lines ##contig= ##range=start-end ##min_depth= ##min_quality= ##min_base_quality=
 * ("." when !has_min_base_quality) ##exclude_flags=0x%04x ##min_del_fraction=%.4f ##min_del_count= ##positions=
 * ##low_depth= ##kept= ##deleted= ##events=, the header
 *   #contig start end length ref del span freq max_del del_fwd del_rev filter
 * and one line per event of dut_del_events: ref = the deleted reference bases (the candidates' ref bytes) when
 * length <= 64, else "."; freq = del / span as %.4f.  ##deleted= is the scan's position count: marked lines stay. */
int dut_del_write(const char *path, const char *contig, const cl_del_result *res, const dut_del_options *opt,
                  char *err, size_t err_len);

/* `find-deletions` on files, one GPU: reads as dut_find_minor_files does, always attaches the records' flags and pass
 * bits and runs the filtered form of cl_site_scan_dels (with no mask and no threshold it counts what the unfiltered form
 * does), writes the TSV.  Errors with a message: those of dut_find_variants_files, refused options. */
int dut_find_deletions_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start,
                             uint32_t end, const dut_del_options *opt, const char *output_path, int device_id,
                             char *err, size_t err_len);

/* ---- find-insertions: per-position insertion counts, calls and alleles (cl_site_scan_ins) ------------------------- */
/* The classes of cl_site_scan_ins. */
enum { DUT_INS_LOW_DEPTH = 0, DUT_INS_KEPT = 1, DUT_INS_INSERTED = 2 };

/* The rule of cl_site_scan_ins for one position in plain C++, with the same integer comparison: low_depth when depth <
 * min_depth; inserted when ins >= min_ins_count and 10000 * ins >= min_ins_per_10k * depth (in 64 bits); kept otherwise.
 * CL_ERR_INVALID: null or refused params (as cl_site_scan_ins refuses them).  The fraction of the command line is parsed
 * by dut_del_fraction_parse: the same interval (0, 1]. */
int dut_ins_classify_counts(uint32_t ins, uint32_t depth, const cl_ins_params *params);

/* One allele of a position: the observations of cl_site_scan_ins there with equal (len, key).  Insertions longer than 32
 * bases that agree in length and in their first 32 bases are one allele: the key holds no more.  fwd + rev == count. */
typedef struct dut_ins_allele {
    uint32_t pos, len;                /* 1-based anchor; inserted bases */
    uint64_t key[2];                  /* as in cl_ins_obs */
    uint32_t count, fwd, rev, pad;
} dut_ins_allele;

/* Groups observations (in any order) into alleles: ascending position; within a position the top allele first -- the
 * most observations, then the smaller len, then the smaller key -- and the others behind it by (len, key).  *alleles:
 * malloc'ed, release with dut_ins_alleles_free (NULL when there is none).  CL_ERR_INVALID: null argument. */
int dut_ins_alleles(const cl_ins_obs *obs, size_t n_obs, dut_ins_allele **alleles, size_t *n_alleles);
void dut_ins_alleles_free(dut_ins_allele *alleles);

/* What a find-insertions run is asked: the scan's parameters and filter, and the strand mark of the TSV. */
typedef struct dut_ins_options {
    uint32_t min_depth;
    uint8_t  min_quality;
    int      has_min_base_quality;
    uint8_t  min_base_quality;
    uint16_t exclude_flags;
    uint32_t min_ins_per_10k;         /* 1..10000 */
    uint32_t min_ins_count;           /* >= 1 */
    uint32_t min_ins_per_strand;      /* K: filter = "strand" when min(ins_fwd, ins_rev) < K; 0: always PASS */
} dut_ins_options;

/* The TSV (no device needed): comment lines ##contig= ##range=start-end ##min_depth= ##min_quality= ##min_base_quality=
 * ("." when !has_min_base_quality) ##exclude_flags=0x%04x ##min_ins_fraction=%.4f ##min_ins_count= ##positions=
 * ##low_depth= ##kept= ##inserted=, the header
 *   #contig pos ref ins depth freq alleles length seq allele_count allele_fwd allele_rev ins_fwd ins_rev filter
 * and one line per candidate: pos = the 1-based anchor, the base before the insertion; freq = ins / depth as %.4f;
 * alleles = the number of alleles there; length, seq, allele_count, allele_fwd, allele_rev describe the top allele, seq
 * decoded with "=ACMGRSVTWYHKDBN" and, for length > 32, its first 32 bases followed by "...".  ##inserted= is the scan's
 * count: marked lines stay.  CL_ERR_INVALID: null argument, candidates that do not ascend, a candidate whose
 * observations are not ins many. */
int dut_ins_write(const char *path, const char *contig, const cl_ins_result *res, const dut_ins_options *opt,
                  char *err, size_t err_len);

/* `find-insertions` on files, one GPU: reads as dut_find_deletions_files does, always attaches the records' flags and
 * pass bits and runs the filtered form of cl_site_scan_ins, writes the TSV.  Errors with a message: those of
 * dut_find_variants_files, refused options. */
int dut_find_insertions_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start,
                              uint32_t end, const dut_ins_options *opt, const char *output_path, int device_id,
                              char *err, size_t err_len);

/* ---- consensus: the sample's sequence, one byte per position (cl_site_scan_consensus), with its insertions ---------- */
/* The classes of cl_site_scan_consensus. */
enum { DUT_CONS_LOW_DEPTH = 0, DUT_CONS_DELETED = 1, DUT_CONS_NO_CALL = 2, DUT_CONS_REF = 3, DUT_CONS_ALT = 4 };

/* The rule of cl_site_scan_consensus for one position in plain C++, with the same integer comparisons; depth is the scan's
 * depth there (a + c + g + t and every other code), del the deletion count, ref_byte the FASTA byte, case preserved (pass
 * 'N' beyond the reference).  Returns the class and, in *byte (may be NULL), n - A C G T or N.  CL_ERR_INVALID: null or
 * refused params (as cl_site_scan_consensus refuses them), a + c + g + t > depth, depth >= 2^32. */
int dut_cons_classify_counts(uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint64_t depth, uint32_t del, const cl_cons_params *params,
                             uint8_t ref_byte, char *byte);

/* One entry of the change list.  pos .. end are 1-based, inclusive.
 *   DUT_CONS_SNV           an alt position: ref = the upper-cased reference byte, cons = the called base
 *   DUT_CONS_DEL           a maximal run of '-' (runs end at the range's borders): ref = the deleted reference bases when
 *                          the run has at most 64 positions, else "."; cons = "-"
 *   DUT_CONS_INS           an insertion spliced behind its anchor pos: ref = the anchor's reference byte, cons = the
 *                          inserted bases (codes outside A/C/G/T written N), count = the allele's observations, depth =
 *                          the anchor's depth
 *   DUT_CONS_INS_SKIPPED   a called insertion that was not spliced, note saying why: the anchor's byte is '-'
 *                          (anchor_deleted), the top allele is longer than 32 bases (too_long), or the top allele itself
 *                          does not meet the insertion rule (no_allele); cons = the allele's first 32 bases */
enum { DUT_CONS_SNV = 0, DUT_CONS_DEL = 1, DUT_CONS_INS = 2, DUT_CONS_INS_SKIPPED = 3 };
enum { DUT_CONS_NOTE_NONE = 0, DUT_CONS_NOTE_ANCHOR_DELETED = 1, DUT_CONS_NOTE_TOO_LONG = 2, DUT_CONS_NOTE_NO_ALLELE = 3 };
typedef struct dut_cons_change {
    uint32_t pos, end;
    uint32_t kind, note;
    uint32_t count, depth;            /* insertions only, else 0 */
    char     ref[68], cons[36];       /* NUL terminated */
} dut_cons_change;

/* What dut_cons_assemble returns: the sequence (NUL terminated, seq_len bytes before it), the change list in ascending
 * position (at one position: the deletion or SNV, then the insertion), and how many deletion runs, spliced and skipped
 * insertions it holds.  Release with dut_cons_assembly_free. */
typedef struct dut_cons_assembly {
    char            *seq;
    uint64_t         seq_len;
    dut_cons_change *changes;
    size_t           n_changes;
    uint64_t         n_deletions, n_insertions, n_insertions_skipped;
} dut_cons_assembly;

/* The sequence of [start, end) from the bytes of cl_site_scan_consensus (cons[p - start]), no device needed.  ref: the
 * reference bytes of the range, ref[0] <-> start, n_ref of them (fewer than end - start when the reference ends inside the
 * range: the rest reads as N).  ins / alleles: the result of cl_site_scan_ins over the same range and gates and the
 * alleles of its observations by dut_ins_alleles (ins == NULL: no insertion is spliced); ins_params: the parameters of
 * that call.  The bytes in order: '-' emits nothing, 'N' emits N, 'n' emits N -- or, with fill_ref, the lower-cased
 * reference base when that is one of a c g t -- and a base emits itself.  Behind a position that ins lists, the top allele
 * there is spliced when the position's byte is not '-', the allele has at most 32 bases and allele_count >= min_ins_count
 * and 10000 * allele_count >= min_ins_per_10k * depth; otherwise the insertion is listed as skipped.  CL_ERR_INVALID: a
 * null argument, a byte outside "n-ACGTN", candidates that do not ascend or lie outside the range, a candidate without
 * an allele, refused ins_params. */
int dut_cons_assemble(const uint8_t *cons, uint32_t start, uint32_t end, const uint8_t *ref, uint64_t n_ref, const cl_ins_result *ins,
                      const dut_ins_allele *alleles, size_t n_alleles, const cl_ins_params *ins_params, int fill_ref,
                      dut_cons_assembly *out);
void dut_cons_assembly_free(dut_cons_assembly *a);

/* What a consensus run is asked. */
typedef struct dut_cons_options {
    uint32_t min_depth;
    uint8_t  min_quality;
    int      has_min_base_quality;
    uint8_t  min_base_quality;
    uint16_t exclude_flags;
    uint32_t min_del_per_10k, min_del_count;      /* 1..10000, >= 1 */
    uint32_t min_ins_per_10k, min_ins_count;      /* 1..10000, >= 1 */
    int      fill_ref;                            /* 0: low-depth positions are N; 1: the lower-cased reference base */
    uint32_t line_width;                          /* >= 1 */
} dut_cons_options;

/* The FASTA (no device needed): the header ">contig" when whole_contig, else ">contig:START-END" (1-based, inclusive:
 * start + 1 .. end), then the sequence in lines of line_width bytes.  An empty sequence writes the header alone. */
int dut_cons_write_fasta(const char *path, const char *contig, int whole_contig, uint32_t start, uint32_t end, const char *seq,
                         uint64_t seq_len, uint32_t line_width, char *err, size_t err_len);

/* The change list, tab separated (no device needed): comment lines ##contig= ##range=start-end (0-based half open)
 * ##min_depth= ##min_quality= ##min_base_quality= ("." when !has_min_base_quality) ##exclude_flags=0x%04x
 * ##min_del_fraction=%.4f ##min_del_count= ##min_ins_fraction=%.4f ##min_ins_count= ##fill=N|ref ##positions= ##low_depth=
 * ##deleted= ##no_call= ##ref= ##alt= ##length= (of the sequence) ##deletions= ##insertions= ##insertions_skipped=, the header
 *   #contig pos end kind ref cons count depth note
 * and one line per change: kind snv | del | ins | ins_skipped; count and depth "." unless an insertion; note "." or the
 * reason an insertion was skipped. */
int dut_cons_write_changes(const char *path, const char *contig, const cl_cons_result *res, const dut_cons_assembly *asm_,
                           const dut_cons_options *opt, char *err, size_t err_len);

/* `consensus` on files, one GPU: reads as dut_find_deletions_files does, always attaches the records' flags and pass bits
 * and runs the filtered forms of cl_site_scan_consensus and cl_site_scan_ins on one resident tile, assembles, writes the
 * FASTA to output_path and, when changes_path is not NULL, the change list.  Errors with a message: those of
 * dut_find_variants_files, refused options. */
int dut_find_consensus_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start,
                             uint32_t end, const dut_cons_options *opt, const char *output_path, const char *changes_path,
                             int device_id, char *err, size_t err_len);

/* ---- find-strs: allele lengths of short tandem repeats (cl_site_str_lengths) ------------------------------------------ */
/* cl_site_str_lengths from host arrays, no device needed: the same hist and partial (the rule is written once, in
 * csrc/str_walk.h, and both routes compile it) for the reads pos / flag / mapq / cigar_off (n_reads + 1) / cigar of a contig
 * of contig_len positions.  strands == 1: one histogram per locus, flag and exclude_flags take no part (flag may be NULL);
 * strands == 2: reads with (flag & exclude_flags) != 0 are left out, forward first, reverse iff flag & 0x10.
 * hist: n_loci * strands * CL_STR_BINS, partial: n_loci, the caller's arrays, in the caller's order of loci.  The loci are
 * spread over DUT_THREADS threads.  CL_ERR_INVALID: a null array, strands outside 1..2, flank outside
 * [1, CL_STR_MAX_FLANK], a locus with start >= end, end > contig_len or end - start > CL_STR_MAX_SPAN, offsets that
 * decrease.  What a caller without a device gets, and the yardstick of tools/str_scan_bench.py. */
int dut_str_measure(const int32_t *pos, const uint16_t *flag, const uint8_t *mapq, const uint32_t *cigar_off, const uint32_t *cigar,
                    uint64_t n_reads, uint32_t contig_len, uint8_t min_quality, uint16_t exclude_flags, uint32_t flank,
                    const cl_str_locus *loci, size_t n_loci, uint32_t *hist, uint32_t *partial, uint32_t strands);

/* The allele of one locus from its histogram(s) of CL_STR_BINS bins (hist_rev may be NULL: one strand).
 *   n           the sum of all 128 bins, strands summed (the spanning reads); other = bin 127
 *   low_depth   n < min_depth
 *   top         the fullest of bins 0..126, among equals the smallest delta; bin 127 ("other") never wins
 *   called      not low and 10000 * count >= min_allele_per_10k * n (taken in 64 bits);  mixed: everything else
 *   second      the fullest of the remaining bins 0..126 under the same tie rule; count2 may be 0
 * delta = bin - 63.  fwd / rev: the top allele by strand (fwd == count, rev == 0 without hist_rev).  top and second are
 * filled in for every status.  CL_ERR_INVALID: a null argument, min_depth == 0, min_allele_per_10k outside [1, 10000]. */
enum { DUT_STR_LOW_DEPTH = 0, DUT_STR_MIXED = 1, DUT_STR_CALLED = 2 };
typedef struct dut_str_params { uint32_t min_depth, min_allele_per_10k; } dut_str_params;
typedef struct dut_str_allele_call {
    int      status;
    int32_t  delta, delta2;
    uint32_t count, fwd, rev, count2;
    uint64_t n, other;
} dut_str_allele_call;
int dut_str_call(const uint32_t *hist_fwd, const uint32_t *hist_rev /* may be NULL */, const dut_str_params *params,
                 dut_str_allele_call *call);

/* The usual repeat-unit notation of a length: len = span + delta bases of a repeat with units of `period` bases is
 * len / period, then '.' and len % period when that is not 0 ("9.3": nine units and three bases).  buf: at least
 * DUT_STR_UNITS_LEN bytes.  CL_ERR_INVALID: null buf, period outside 1..255, span + delta < 0. */
#define DUT_STR_UNITS_LEN 24
int dut_str_units(uint32_t span, int32_t delta, uint32_t period, char *buf);

/* One line of a loci file. */
typedef struct dut_str_locus {
    uint32_t start, end;              /* 0-based, half open */
    uint32_t period;                  /* 1..255 */
    char     name[64];                /* NUL terminated */
} dut_str_locus;

/* The loci file: tab separated `contig start end period name`, 0-based half open; lines that start with '#' and empty
 * lines are skipped, columns behind the fifth are ignored, lines of other contigs are skipped and counted in *n_skipped.
 * *loci: the lines of `contig` in file order, malloc'ed, release with dut_str_loci_free (NULL when there is none).
 * CL_ERR_INVALID with a message: an unreadable file; a malformed line, named by its number -- fewer than five columns, a
 * start, end or period that is not a decimal number below 2^32, start >= end, a period outside 1..255, an empty name or
 * one of more than 63 bytes.  Whether a locus fits the contig is not the parser's question. */
int dut_str_loci_parse(const char *path, const char *contig, dut_str_locus **loci, size_t *n_loci, size_t *n_skipped,
                       char *err, size_t err_len);
void dut_str_loci_free(dut_str_locus *loci);

/* What a find-strs run is asked. */
typedef struct dut_str_options {
    uint32_t min_depth;               /* >= 1 */
    uint8_t  min_quality;
    uint16_t exclude_flags;
    uint32_t flank;                   /* 1..CL_STR_MAX_FLANK */
    uint32_t min_allele_per_10k;      /* 1..10000 */
} dut_str_options;

/* The TSV (no device needed) of n_loci loci with hist (n_loci * strands * CL_STR_BINS) and partial (n_loci) as
 * cl_site_str_lengths or dut_str_measure return them: comment lines ##contig= ##loci= ##loci_skipped= ##flank= ##min_depth=
 * ##min_quality= ##exclude_flags=0x%04x ##min_allele_fraction=%.4f ##low_depth= ##mixed= ##called=, the header
 *   #contig start end name period ref_units spanning partial other status allele delta count freq fwd rev allele2 delta2 count2
 * and one line per locus in the given order: ref_units = dut_str_units of the reference's own length; spanning = n of
 * dut_str_call; status low_depth | mixed | called; allele, allele2 = dut_str_units texts; delta with its sign (+2, -4, 0);
 * freq = count / spanning as %.4f; the top allele's columns (allele delta count freq fwd rev) are "." for low_depth (and
 * when no read fell into bins 0..126 at all), the second allele's when its count is 0.  CL_ERR_INVALID: a null argument, strands outside 1..2, refused options. */
int dut_str_write(const char *path, const char *contig, const dut_str_locus *loci, size_t n_loci, size_t n_skipped,
                  const uint32_t *hist, const uint32_t *partial, uint32_t strands, const dut_str_options *opt,
                  char *err, size_t err_len);

/* `find-strs` on files, one GPU: parses the loci file (before any device is opened), reads as dut_find_insertions_files
 * does, always attaches the records' flags and runs the filtered form of cl_site_str_lengths, in chunks of at most
 * CL_STR_MAX_LOCI loci, writes the TSV.  Errors with a message: those of dut_find_variants_files, refused options, an
 * unreadable or malformed loci file, a locus that ends beyond the contig or is longer than CL_STR_MAX_SPAN. */
int dut_find_strs_files(const char *bam_path, const char *fasta_path, const char *contig, const char *loci_path,
                        const dut_str_options *opt, const char *output_path, int device_id, char *err, size_t err_len);

/* ---- error-profile: substitutions and indels by read cycle (cl_site_error_profile) ------------------------------------- */
/* The reads of a contig as host arrays: pos / flag / mapq / cigar_off (n_reads + 1) / cigar as dut_str_measure takes them;
 * the stored bases as 4-bit codes, base i of the array in byte i / 2, high nibble first, read r holding bases
 * [seq_off[r], seq_off[r + 1]); the quality values numbered by qual_off, which need not agree with seq_off (a base without
 * a value passes a base-quality filter, as in cl_site_attach_quals).  flag may be NULL for an unfiltered call, qual_off and
 * qual when no base-quality threshold is given. */
typedef struct dut_ep_reads {
    uint64_t        n_reads;
    const int32_t  *pos;
    const uint16_t *flag;
    const uint8_t  *mapq;
    const uint32_t *cigar_off, *cigar;
    const uint64_t *seq_off;
    const uint8_t  *seq4;
    const uint64_t *qual_off;
    const uint8_t  *qual;
} dut_ep_reads;

/* What an error-profile run is asked.  filtered == 0: no flag is read, every read is forward, every base passes (the
 * unfiltered form of cl_site_error_profile; exclude_flags and the threshold take no part).  dut_error_profile_files always
 * runs the filtered form. */
typedef struct dut_ep_options {
    uint8_t  min_quality;
    int      filtered;
    uint16_t exclude_flags;
    int      has_min_base_quality;    /* 0: every base passes */
    uint8_t  min_base_quality;
    uint32_t n_cycles;                /* 1..CL_EP_MAX_CYCLES */
} dut_ep_options;

/* cl_site_error_profile from host arrays, no device needed: the same tables and scalars (the walk is written once, in
 * csrc/ep_walk.h, and both routes compile it) over [start, end) of a contig of contig_len positions with the reference
 * bytes ref_bases[0, ref_len).  tables: 36 * n_cycles words of the caller's, filled as from5 and from3 [cycle][16], then
 * ins5, ins3, del5, del3 [cycle]; out's pointers are set into it.  The reads are spread over DUT_THREADS threads.
 * CL_ERR_INVALID: a null argument or array, n_cycles outside [1, CL_EP_MAX_CYCLES], start > end, end > contig_len, offsets
 * that decrease.  What a caller without a device gets, and the yardstick of tools/error_profile_bench.py. */
int dut_error_profile_measure(const dut_ep_reads *reads, uint32_t contig_len, const uint8_t *ref_bases, uint64_t ref_len,
                              uint32_t start, uint32_t end, const dut_ep_options *opt, uint64_t *tables, cl_ep_result *out);

/* The TSV (no device needed) of a result: comment lines ##contig= ##range=start-end ##cycles= ##min_quality=
 * ##min_base_quality= ("." when not given) ##exclude_flags=0x%04x ##reads= ##bases= ##uncomparable= ##mismatches=
 * ##mismatch_rate= ##insertions= ##inserted_bases= ##deletions= ##deleted_bases=, the header
 *   #table cycle A>A A>C A>G A>T C>A ... T>T ins del mismatch_rate
 * one `total` line with cycle ".", then `5p` lines for cycles 1..C and `3p` lines for cycles 1..C (1-based in the file).
 * mismatch_rate = the off-diagonal sum over the 16-cell sum as %.6f, "NA" when that sum is 0.  CL_ERR_INVALID: a null
 * argument, a result whose n_cycles is outside [1, CL_EP_MAX_CYCLES] or differs from the options'. */
int dut_error_profile_write(const char *path, const char *contig, const cl_ep_result *res, const dut_ep_options *opt,
                            char *err, size_t err_len);

/* `error-profile` on files, one GPU: reads as dut_find_strs_files does, always attaches the records' flags and pass bits
 * and runs the filtered form of cl_site_error_profile over the contig or the region, writes the TSV.  Errors with a
 * message: those of dut_find_variants_files, n_cycles outside [1, CL_EP_MAX_CYCLES]. */
int dut_error_profile_files(const char *bam_path, const char *fasta_path, const char *contig, int has_region, uint32_t start,
                            uint32_t end, const dut_ep_options *opt, const char *output_path, int device_id, char *err,
                            size_t err_len);

/* ---- phase-sites: joint allele counts of site pairs per read (cl_site_link_counts) ------------------------------------- */
/* What a phase-sites run is asked.  filtered == 0: no flag is read and every base passes (the unfiltered form of
 * cl_site_link_counts; exclude_flags and the threshold take no part).  dut_find_links_files always runs the filtered form. */
typedef struct dut_link_options {
    uint32_t min_depth;               /* >= 1 */
    uint8_t  min_quality;
    int      filtered;
    uint16_t exclude_flags;
    int      has_min_base_quality;    /* 0: every base passes */
    uint8_t  min_base_quality;
    uint32_t max_dist;                /* >= 1 */
    uint32_t max_partners;            /* 1..CL_LINK_MAX_PARTNERS */
    uint32_t min_link_count;          /* >= 1 */
    uint32_t max_discord_per_10k;     /* 0..4999 */
} dut_link_options;

/* The pair set of cl_site_link_counts for strictly ascending sites: first[i] (n_sites + 1 words, may be NULL) is the CSR
 * offset of anchor i, *n_pairs the number of pairs -- not bounded by CL_LINK_MAX_PAIRS, so that a caller can see how far
 * above it a set lies (offsets above 2^32 - 1 are clamped).  The engine, the host route and this function count the
 * partners of an anchor by one function of csrc/link_walk.h.  CL_ERR_INVALID: null sites with n_sites > 0, null n_pairs,
 * sites not strictly ascending, max_dist == 0, max_partners outside [1, CL_LINK_MAX_PARTNERS]. */
int dut_link_pair_offsets(const uint32_t *sites, size_t n_sites, uint32_t max_dist, uint32_t max_partners, uint32_t *first,
                          uint64_t *n_pairs);

/* cl_site_link_counts from host arrays, no device needed: the same first, tables and site_counts (the walk is written
 * once, in csrc/link_walk.h, and both routes compile it) for the reads of a contig of contig_len positions.  Of opt it
 * reads min_quality, filtered, exclude_flags, has_min_base_quality, min_base_quality (taken over the reads' quality
 * values; a base without one passes), max_dist and max_partners.  first: n_sites + 1, tables: 36 per pair (ask
 * dut_link_pair_offsets for their number first), site_counts: 6 per site, the caller's arrays.  The anchors are spread
 * over DUT_THREADS threads.  CL_ERR_INVALID: a null argument or array, what dut_link_pair_offsets refuses, more than
 * CL_LINK_MAX_SITES sites or CL_LINK_MAX_PAIRS pairs, a site >= contig_len, offsets that decrease.  What a caller without
 * a device gets, and the yardstick of tools/link_bench.py. */
int dut_link_measure(const dut_ep_reads *reads, uint32_t contig_len, const dut_link_options *opt, const uint32_t *sites,
                     size_t n_sites, uint32_t *first, uint32_t *tables, uint32_t *site_counts);

/* One pair from its two sites' counts (6 each) and its table (36), in integers.
 *   major       per site the fullest of A C G T del, the first in that order among equals
 *   minor       the fullest of the other four under the same tie rule (its count may be 0)
 *   both        the sum of the 36 cells;  MM Mm mM mm: the cells of {major_a, minor_a} x {major_b, minor_b};
 *               other = both - n4 with n4 their sum;  m = Mm + mM + mm
 *   low_depth   n4 < min_depth
 *   cis         else mm >= min_link_count and 10000 * (Mm + mM) <= max_discord_per_10k * m
 *   trans       else Mm >= min_link_count and mM >= min_link_count and 10000 * mm <= max_discord_per_10k * m
 *   unresolved  everything else
 * All products are taken in 64 bits.  max_discord_per_10k <= 4999 makes cis and trans exclude each other, in whichever
 * order they are asked.  depth_a / depth_b: the sum of the site's six counts.  CL_ERR_INVALID: a null argument,
 * min_depth == 0, min_link_count == 0, max_discord_per_10k > 4999. */
enum { DUT_LINK_LOW_DEPTH = 0, DUT_LINK_CIS = 1, DUT_LINK_TRANS = 2, DUT_LINK_UNRESOLVED = 3 };
typedef struct dut_link_params { uint32_t min_depth, min_link_count, max_discord_per_10k; } dut_link_params;
typedef struct dut_link_summary {
    int      status;
    uint8_t  major_a, minor_a, major_b, minor_b;      /* 0..4: A C G T del */
    uint64_t depth_a, depth_b, both, MM, Mm, mM, mm, other;
} dut_link_summary;
int dut_link_summarise(const uint32_t *site_counts_a, const uint32_t *site_counts_b, const uint32_t *table,
                       const dut_link_params *params, dut_link_summary *out);

/* "0.05" -> 500 parts per 10 000, exactly: a decimal in [0, 0.4999] with at most four decimals (the parser of the other
 * fractions, with 0 allowed). */
int dut_link_discordance_parse(const char *text, uint32_t *per_10k, char *err, size_t err_len);

/* The sites file: tab separated, column 1 the contig, column 2 a 1-based position; further columns are ignored, lines that
 * start with '#' and empty lines are skipped -- the TSVs of find-variants, find-minor-alleles and find-deletions (its
 * start column) can be given as they are.  Lines of other contigs are skipped and counted in *n_skipped.  *sites: the
 * 0-based positions of `contig`, sorted, duplicates merged, malloc'ed, release with dut_link_sites_free (NULL when there
 * is none).  CL_ERR_INVALID with a message: an unreadable file; a malformed line, named by its number -- fewer than two
 * columns, an empty contig, a position that is not a decimal number in [1, 2^32).  Whether a site fits the contig is not
 * the parser's question. */
int dut_link_sites_parse(const char *path, const char *contig, uint32_t **sites, size_t *n_sites, size_t *n_skipped,
                         char *err, size_t err_len);
void dut_link_sites_free(uint32_t *sites);

/* The TSV (no device needed) of the pairs of n_sites strictly ascending 0-based sites with first, tables and site_counts as
 * cl_site_link_counts or dut_link_measure return them under opt's max_dist and max_partners: comment lines ##contig=
 * ##sites= ##sites_skipped= ##pairs= ##max_dist= ##max_partners= ##min_depth= ##min_quality= ##min_base_quality= ("." when
 * not given) ##exclude_flags=0x%04x ##min_link_count= ##max_discordance=%.4f ##low_depth= ##cis= ##trans= ##unresolved=,
 * the header
 *   #contig pos_a pos_b dist major_a minor_a major_b minor_b depth_a depth_b both MM Mm mM mm other status
 * and one line per pair in pair order, positions 1-based, alleles A C G T or del, the columns of dut_link_summarise.
 * CL_ERR_INVALID: a null argument, refused options, a first that is not the pair set of the sites. */
int dut_link_write(const char *path, const char *contig, const uint32_t *sites, size_t n_sites, size_t n_skipped,
                   const uint32_t *first, const uint32_t *tables, const uint32_t *site_counts, const dut_link_options *opt,
                   char *err, size_t err_len);

/* `phase-sites` on files, one GPU: parses the sites file (before any device is opened), reads as dut_find_strs_files does,
 * always attaches the records' flags and pass bits and runs the filtered form of cl_site_link_counts -- with no mask and
 * no threshold it counts what the unfiltered form does -- and writes the TSV.  Errors with a message: those of
 * dut_find_variants_files, refused options, an unreadable or malformed sites file, a site beyond the contig, a pair set
 * above CL_LINK_MAX_PAIRS. */
int dut_find_links_files(const char *bam_path, const char *fasta_path, const char *contig, const char *sites_path,
                         const dut_link_options *opt, const char *output_path, int device_id, char *err, size_t err_len);

#ifdef __cplusplus
}
#endif
#endif /* DUT_VARIANTS_H */
