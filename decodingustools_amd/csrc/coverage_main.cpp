// dut-coverage -- the `coverage`, `find-y-branch` and `find-mt-branch` subcommands of the reference CLI (and this
// project's own `fingerprint` front end, `find-variants`, `find-minor-alleles`, `find-deletions`, `find-insertions`, `consensus`, `find-strs`, `error-profile` and `phase-sites`);
// `coverage` is the default: (src/cli.rs:14-61, src/main.rs:36-70)
// on the MI355X engine.  Same flags and defaults; BED to -o, the CoverageOutput JSON to ./summary.json.
// -s/--summary: the HTML report (the reference's sections and numbers in this project's own markup); the
// per-contig coverage figures <contig>_coverage.svg go beside the BED file.
#include "../../include/dut_bam.h"
#include "../../include/dut_haplogroup.h"
#include "../../include/dut_fingerprint.h"
#include "../../include/dut_variants.h"

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <algorithm>
#include <string>
#include <cerrno>
#include <sys/types.h>
#include <sys/wait.h>
#include <unistd.h>
#include <vector>

static void usage()
{
    fprintf(stderr,
            "Usage: dut-coverage [coverage] <BAM_FILE> -r <REFERENCE_FILE> [-o callable_regions.bed] [-s summary.html]\n"
            "       [-L <CONTIG>]... [--min-depth 4] [--max-depth 500] [--min-mapping-quality 10]\n"
            "       [--min-base-quality 20] [--min-depth-for-low-mapq 10] [--max-low-mapq 1]\n"
            "       [--max-low-mapq-fraction 0.1] [--device 0 | --devices 0,1,...]\n"
            "       [--depth-dist FILE] [--depth-windows FILE --window S] [--depth-summary FILE] [--depth-cap 1000]\n"
            "         depth profile per contig and in total: histogram of raw / quality-filtered depth (depths above the cap in\n"
            "         one last bin, cap 1..4095), mean depth per window of S >= 16 positions, quartiles and share at >= Nx\n"
            "       [--depth-bed FILE [--depth-bed-kind raw|qc] [--quantize SPEC]]\n"
            "         per-base depth as a BED of runs of equal depth (contig, start, end, depth; no header); kind raw (default)\n"
            "         or qc (quality-filtered); SPEC such as 1:4:100 merges runs within the bands 0, 1-3, 4-99, 100+ (at most\n"
            "         64 edges; a leading 0: and a trailing : are accepted)\n"
            "       [--targets BED --target-out FILE [--target-thresholds 1,10,20,30] [--target-quantiles]]\n"
            "         per region of BED (0-based, half open; column 4 = name): length, mean raw / quality-filtered depth, callable\n"
            "         bases and the other states, positions at >= each threshold (at most 8); a `total` line last, in which\n"
            "         overlapping regions count twice; --target-quantiles adds minimum, quartiles and maximum of both depths\n"
            "       [--gc-bias FILE] [--gc-summary FILE] [--gc-window 100] [--gc-max-n 4]\n"
            "         depth by the GC content of the reference in a window of W positions (1..1024) centred on each position: per\n"
            "         contig and in total a line per GC percentage (positions, mean and normalised depth, share without reads) and\n"
            "         a summary line with the AT and GC dropout; positions with more than K invalid bases (N, IUPAC) in the\n"
            "         window are skipped (K < W)\n"
            "       dut-coverage fingerprint <INPUT> [-r REF] [--ksize 31] [--scaled 1000] [--max-frequency N] [-o FILE] [-R full|chrY|chrM] [--device 0]\n"
            "       dut-coverage fingerprint-compare A.fp B.fp [C.fp ...] [--list FILE] -o out.tsv [--matrix FILE] [--query Q.fp] [--min-jaccard X] [--device 0]\n"
            "       dut-coverage find-variants <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END] [--min-depth 10]\n"
            "       [--min-quality 20] [--tree FILE [--provider ftdna|decodingus] [--tree-type y|mt]] [--device 0]\n"
            "       dut-coverage find-minor-alleles <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END] [--min-depth 10]\n"
            "       [--min-quality 20] [--min-minor-fraction 0.05] [--min-minor-count 3] [--min-base-quality Q] [--exclude-flags MASK]\n"
            "       [--min-minor-per-strand K] [--device 0]\n"
            "       dut-coverage find-deletions <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END] [--min-depth 10]\n"
            "       [--min-quality 20] [--min-del-fraction 0.7] [--min-del-count 3] [--min-base-quality Q] [--exclude-flags MASK]\n"
            "       [--min-del-per-strand K] [--device 0]\n"
            "       dut-coverage find-insertions <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END] [--min-depth 10]\n"
            "       [--min-quality 20] [--min-ins-fraction 0.7] [--min-ins-count 3] [--min-base-quality Q] [--exclude-flags MASK]\n"
            "       [--min-ins-per-strand K] [--device 0]\n"
            "       dut-coverage consensus <BAM_FILE> -r <REFERENCE_FILE> -o <FASTA> -L <CONTIG> [--region START-END] [--min-depth 10]\n"
            "       [--min-quality 20] [--min-del-fraction 0.7] [--min-del-count 3] [--min-ins-fraction 0.7] [--min-ins-count 3]\n"
            "       [--min-base-quality Q] [--exclude-flags MASK] [--fill N|ref] [--line-width 60] [--changes FILE] [--device 0]\n"
            "       dut-coverage find-strs <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> --loci FILE [--flank 5] [--min-depth 10]\n"
            "       [--min-quality 20] [--min-allele-fraction 0.7] [--exclude-flags MASK] [--device 0]\n"
            "       dut-coverage error-profile <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END] [--cycles 50]\n"
            "       [--min-quality 20] [--min-base-quality Q] [--exclude-flags MASK] [--device 0]\n"
            "       dut-coverage phase-sites <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> --sites FILE [--max-dist 1000] [--max-partners 4]\n"
            "       [--min-depth 10] [--min-quality 20] [--min-link-count 3] [--max-discordance 0.05] [--min-base-quality Q]\n"
            "       [--exclude-flags MASK] [--device 0]\n");
}

// fingerprint (src/cli.rs:129-156, src/commands/fingerprint.rs:9-52): a k-mer MinHash sketch of every read of a
// BAM or FASTQ file.  Argument and file-format errors are reported before any device is opened.
static int fingerprint_main(int argc, char **argv)
{
    std::string input, ref, out, region = "full";
    dut_fp_options opt = {31, 1000, 0, 0};
    int device = 0;
    auto usage_fp = []() {
        fprintf(stderr,
                "Usage: dut-coverage fingerprint <INPUT> [-r REF] [--ksize 31] [--scaled 1000] [--max-frequency N] [-o FILE]\n"
                "       [-R full|chrY|chrM] [--device 0]\n"
                "  INPUT: .bam, .fastq, .fq or .gz (FASTQ, plain or gzip; 4-line records).  1 <= ksize <= 64.\n"
                "  -R only labels the output file (#region=...), as in the reference: every read of the file is used.\n");
    };
    auto number = [&](const char *flag, const char *v, unsigned long long &dst) -> bool {
        char *end = nullptr;
        errno = 0;
        if (!*v || *v == '-') { fprintf(stderr, "error: invalid value '%s' for '%s'\n", v, flag); return false; }
        dst = strtoull(v, &end, 10);
        if (errno || *end) { fprintf(stderr, "error: invalid value '%s' for '%s'\n", v, flag); return false; }
        return true;
    };
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i], val;
        const size_t eq = a.find('=');
        const bool has_eq = a.rfind("--", 0) == 0 && eq != std::string::npos;
        if (has_eq) { val = a.substr(eq + 1); a = a.substr(0, eq); }
        auto next = [&]() -> const char * {
            if (has_eq) return val.c_str();
            if (i + 1 >= argc) { usage_fp(); exit(2); }
            return argv[++i];
        };
        unsigned long long v = 0;
        if (a == "-r" || a == "--reference") ref = next();
        else if (a == "-o" || a == "--output") out = next();
        else if (a == "--ksize") {
            if (!number("--ksize", next(), v)) return 2;
            if (v < 1 || v > 64) { fprintf(stderr, "error: invalid value '%llu' for '--ksize': this build supports 1..64\n", v); return 2; }
            opt.ksize = (uint32_t)v;
        }
        else if (a == "--scaled") { if (!number("--scaled", next(), v)) return 2; opt.scaled = v; }
        else if (a == "--max-frequency") {
            if (!number("--max-frequency", next(), v) || v > 0xFFFFFFFFull) { if (v > 0xFFFFFFFFull) fprintf(stderr, "error: invalid value for '--max-frequency'\n"); return 2; }
            opt.max_frequency = (uint32_t)v; opt.has_max_frequency = 1;
        }
        else if (a == "-R" || a == "--region") {
            region = next();
            if (region != "full" && region != "chrY" && region != "chrM") {
                fprintf(stderr, "error: invalid value '%s' for '--region <REGION>'\n  [possible values: full, chrY, chrM]\n", region.c_str());
                return 2;
            }
        }
        else if (a == "--device") device = atoi(next());
        else if (a == "-h" || a == "--help") { usage_fp(); return 0; }
        else if (!a.empty() && a[0] != '-' && input.empty()) input = a;
        else { fprintf(stderr, "error: unexpected argument '%s'\n", argv[i]); usage_fp(); return 2; }
    }
    if (input.empty()) { usage_fp(); return 2; }
    char err[1024] = {0};
    if (dut_fp_input_kind(input.c_str(), err, sizeof(err)) < 0) { fprintf(stderr, "Error: %s\n", err); return 1; }
    if (access(input.c_str(), R_OK) != 0) { fprintf(stderr, "Error: cannot open %s: %s\n", input.c_str(), strerror(errno)); return 1; }
    char digest[65] = {0};
    uint64_t processed = 0;
    const int rc = dut_fp_files(input.c_str(), ref.empty() ? nullptr : ref.c_str(), out.empty() ? nullptr : out.c_str(), &opt,
                                region.c_str(), device, digest, &processed, err, sizeof(err));
    if (digest[0]) printf("Processed %llu sequences\n%s\n", (unsigned long long)processed, digest);
    if (rc != CL_OK) { fprintf(stderr, "Error: %s\n", err); fflush(nullptr); _exit(1); }
    fflush(nullptr);
    _exit(0);                              // outputs are closed; skip the HIP runtime's exit handlers (see main)
}

// fingerprint-compare: the hash files `fingerprint -o` wrote, against each other (or --query against each of them) on the
// device.  Argument errors are reported before any file is read or a device is opened.
static int fingerprint_compare_main(int argc, char **argv)
{
    std::vector<std::string> files;
    std::string out, matrix, query, list;
    dut_fpc_file_options opt = {nullptr, 0.0, 0};
    int device = 0;
    auto usage_fc = []() {
        fprintf(stderr,
                "Usage: dut-coverage fingerprint-compare A.fp B.fp [C.fp ...] [--list FILE] -o out.tsv [--matrix FILE]\n"
                "       [--query Q.fp] [--min-jaccard X] [--device 0]\n"
                "  The files are what `fingerprint -o` writes.  Without --query: all pairs i < j; with it: Q against each other file.\n"
                "  --list adds one path per line.  --matrix: the square Jaccard matrix (without --query only).\n"
                "  --min-jaccard leaves out the lines below X (0..1).\n");
    };
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i], val;
        const size_t eq = a.find('=');
        const bool has_eq = a.rfind("--", 0) == 0 && eq != std::string::npos;
        if (has_eq) { val = a.substr(eq + 1); a = a.substr(0, eq); }
        auto next = [&]() -> const char * {
            if (has_eq) return val.c_str();
            if (i + 1 >= argc) { usage_fc(); exit(2); }
            return argv[++i];
        };
        if (a == "-o" || a == "--output") out = next();
        else if (a == "--matrix") matrix = next();
        else if (a == "--query") query = next();
        else if (a == "--list") list = next();
        else if (a == "--min-jaccard") {
            const char *v = next();
            char *end = nullptr;
            errno = 0;
            const double x = strtod(v, &end);
            if (!*v || errno || *end || !(x >= 0.0 && x <= 1.0)) { fprintf(stderr, "error: invalid value '%s' for '--min-jaccard' (0..1)\n", v); return 2; }
            opt.min_jaccard = x; opt.has_min_jaccard = 1;
        }
        else if (a == "--device") device = atoi(next());
        else if (a == "-h" || a == "--help") { usage_fc(); return 0; }
        else if (!a.empty() && a[0] != '-') files.push_back(a);
        else { fprintf(stderr, "error: unexpected argument '%s'\n", argv[i]); usage_fc(); return 2; }
    }
    if (out.empty()) { fprintf(stderr, "error: fingerprint-compare needs '-o <FILE>'\n"); usage_fc(); return 2; }
    if (!query.empty() && !matrix.empty()) { fprintf(stderr, "error: '--matrix' is written without '--query' only\n"); return 2; }
    if (!list.empty()) {
        FILE *f = fopen(list.c_str(), "rb");
        if (!f) { fprintf(stderr, "Error: cannot open %s: %s\n", list.c_str(), strerror(errno)); return 1; }
        std::string line;
        for (int ch; (ch = fgetc(f)) != EOF || !line.empty();) {
            if (ch != '\n' && ch != EOF) { line += (char)ch; continue; }
            while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
            if (!line.empty()) files.push_back(line);
            line.clear();
            if (ch == EOF) break;
        }
        fclose(f);
    }
    if (files.size() + (query.empty() ? 0 : 1) < 2) { fprintf(stderr, "error: fingerprint-compare needs at least two sketches\n"); usage_fc(); return 2; }
    std::vector<const char *> paths;
    for (const std::string &p : files) paths.push_back(p.c_str());
    if (!query.empty()) opt.query = query.c_str();
    char err[1024] = {0};
    const int rc = dut_fingerprint_compare_files(paths.data(), paths.size(), &opt, out.c_str(), matrix.empty() ? nullptr : matrix.c_str(),
                                                 device, err, sizeof(err));
    if (rc != CL_OK) { fprintf(stderr, "Error: %s\n", err); fflush(nullptr); _exit(1); }
    fflush(nullptr);
    _exit(0);                              // outputs are closed; skip the HIP runtime's exit handlers (see main)
}

// find-y-branch / find-mt-branch (src/cli.rs:62-105, src/commands/find_branch.rs).  The reference
// downloads the tree; here --tree names a local JSON file of the provider's shape.
static int find_branch_main(int argc, char **argv, int tree_type)
{
    std::string bam, ref, out, tree;
    uint32_t min_depth = 10; unsigned min_quality = 20;
    int provider = DUT_PROVIDER_FTDNA, show_snps = 0, device = 0;
    auto usage_fb = [&]() {
        fprintf(stderr, "Usage: dut-coverage %s <BAM_FILE> -r <REFERENCE_FILE> <OUTPUT_FILE> --tree <TREE_JSON>\n"
                        "       [--min-depth 10] [--min-quality 20] [--provider ftdna|decodingus] [--show-snps] [--device 0]\n",
                tree_type == DUT_TREE_YDNA ? "find-y-branch" : "find-mt-branch");
    };
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i], val;
        const size_t eq = a.find('=');
        const bool has_eq = a.rfind("--", 0) == 0 && eq != std::string::npos;
        if (has_eq) { val = a.substr(eq + 1); a = a.substr(0, eq); }
        auto next = [&]() -> const char * {
            if (has_eq) return val.c_str();
            if (i + 1 >= argc) { usage_fb(); exit(2); }
            return argv[++i];
        };
        if (a == "-r" || a == "--reference") ref = next();
        else if (a == "--tree") tree = next();
        else if (a == "--min-depth") min_depth = (uint32_t)strtoul(next(), nullptr, 10);
        else if (a == "--min-quality") min_quality = (unsigned)strtoul(next(), nullptr, 10);
        else if (a == "--provider") {
            const std::string p = next();
            if (p == "ftdna") provider = DUT_PROVIDER_FTDNA;
            else if (p == "decodingus") provider = DUT_PROVIDER_DECODINGUS;
            else { fprintf(stderr, "error: invalid value '%s' for '--provider'\n", p.c_str()); return 2; }
        }
        else if (a == "--show-snps") show_snps = 1;
        else if (a == "--device") device = atoi(next());
        else if (a == "-h" || a == "--help") { usage_fb(); return 0; }
        else if (!a.empty() && a[0] != '-' && bam.empty()) bam = a;
        else if (!a.empty() && a[0] != '-' && out.empty()) out = a;
        else { fprintf(stderr, "error: unexpected argument '%s'\n", argv[i]); usage_fb(); return 2; }
    }
    if (bam.empty() || ref.empty() || out.empty() || tree.empty()) { usage_fb(); return 2; }
    char err[1024] = {0};
    const int rc = dut_find_branch_files(bam.c_str(), ref.c_str(), tree.c_str(), out.c_str(), min_depth, (uint8_t)min_quality,
                                         tree_type, provider, show_snps, device, err, sizeof(err));
    if (rc != CL_OK) { fprintf(stderr, "Error: %s\n", err); return 1; }
    fflush(nullptr);
    _exit(0);                              // outputs are closed; skip the HIP runtime's exit handlers (see main)
}

// The values the scan subcommands share; each prints its message and returns false on a malformed one.
static bool cli_number(const char *flag, const std::string &v, unsigned long long &dst)
{
    char *e = nullptr;
    errno = 0;
    if (v.empty() || v[0] < '0' || v[0] > '9') { fprintf(stderr, "error: invalid value '%s' for '%s'\n", v.c_str(), flag); return false; }
    dst = strtoull(v.c_str(), &e, 10);
    if (errno || *e) { fprintf(stderr, "error: invalid value '%s' for '%s'\n", v.c_str(), flag); return false; }
    return true;
}

// --region START-END: 0-based, half open, not empty, below 2^32
static bool cli_region(const std::string &region, unsigned long long &start, unsigned long long &end)
{
    const size_t dash = region.find('-');
    if (dash == std::string::npos || !cli_number("--region", region.substr(0, dash), start) || !cli_number("--region", region.substr(dash + 1), end)) {
        if (dash == std::string::npos) fprintf(stderr, "error: invalid value '%s' for '--region': START-END\n", region.c_str());
        return false;
    }
    if (start >= end || end > 0xFFFFFFFFull) { fprintf(stderr, "error: invalid value '%s' for '--region': the range is empty or beyond 2^32\n", region.c_str()); return false; }
    return true;
}

static bool cli_min_depth(const std::string &v, unsigned long long &min_depth)
{
    if (!cli_number("--min-depth", v, min_depth)) return false;
    if (min_depth < 1 || min_depth > 0xFFFFFFFFull) { fprintf(stderr, "error: invalid value '%llu' for '--min-depth': at least 1\n", min_depth); return false; }
    return true;
}

static bool cli_min_quality(const std::string &v, unsigned long long &min_quality)
{
    if (!cli_number("--min-quality", v, min_quality)) return false;
    if (min_quality > 255) { fprintf(stderr, "error: invalid value '%llu' for '--min-quality': 0..255\n", min_quality); return false; }
    return true;
}

static bool cli_base_quality(const std::string &v, uint8_t &dst)
{
    unsigned long long q = 0;
    if (!cli_number("--min-base-quality", v, q)) return false;
    if (q > 255) { fprintf(stderr, "error: invalid value '%s' for '--min-base-quality': 0..255\n", v.c_str()); return false; }
    dst = (uint8_t)q;
    return true;
}

// --exclude-flags MASK: 0..65535, decimal or 0x hex
static bool cli_flag_mask(const std::string &v, uint16_t &dst)
{
    const bool hex = v.size() > 2 && v[0] == '0' && (v[1] == 'x' || v[1] == 'X');
    char *e = nullptr;
    errno = 0;
    const unsigned long long m = (hex ? isxdigit((unsigned char)v[2]) : (!v.empty() && isdigit((unsigned char)v[0]))) ? strtoull(v.c_str(), &e, hex ? 16 : 10) : 0;
    if (!e || errno || *e || m > 65535) { fprintf(stderr, "error: invalid value '%s' for '--exclude-flags': 0..65535, decimal or 0x hex\n", v.c_str()); return false; }
    dst = (uint16_t)m;
    return true;
}

static bool cli_count32(const char *flag, const std::string &v, uint32_t &dst)
{
    unsigned long long k = 0;
    if (!cli_number(flag, v, k)) return false;
    if (k > 0xFFFFFFFFull) { fprintf(stderr, "error: invalid value '%s' for '%s'\n", v.c_str(), flag); return false; }
    dst = (uint32_t)k;
    return true;
}

// What the scan subcommands (find-variants, find-minor-alleles, find-deletions, find-insertions, consensus, find-strs, error-profile, phase-sites) share on the command line: the BAM, -r, -o,
// -L, --region (0-based, half open), --min-depth, --min-quality, the two filter flags, --device, -h.
struct ScanCli {
    const char *name;
    void (*usage)();
    std::string bam, ref, out, contig;
    unsigned long long min_depth = 10, min_quality = 20, start = 0, end = 0;
    int device = 0;
    bool has_region = false, filter_flag = false;            // (a filter flag was given, whatever its value)
    uint8_t min_base_quality = 0;
    int has_min_base_quality = 0;
    uint16_t exclude_flags = 0;
    // the two filter fields into a command's options (dut_variants_options, dut_minor_options, dut_del_options, dut_ins_options)
    template <class Options> void filter_into(Options &o) const
    {
        o.has_min_base_quality = has_min_base_quality; o.min_base_quality = min_base_quality; o.exclude_flags = exclude_flags;
    }
};

// The argument loop of a scan subcommand.  own(a, next) takes the command's own flags: 1 taken, 0 not one of them, -1 a
// malformed value (its message printed).  Returns -1 to go on, else the exit status: argument errors leave with 2 before a
// device is opened.
template <class Own>
static int scan_cli_parse(int argc, char **argv, ScanCli &c, Own &&own)
{
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i], val;
        const size_t eq = a.find('=');
        const bool has_eq = a.rfind("--", 0) == 0 && eq != std::string::npos;
        if (has_eq) { val = a.substr(eq + 1); a = a.substr(0, eq); }
        auto next = [&]() -> const char * {
            if (has_eq) return val.c_str();
            if (i + 1 >= argc) { c.usage(); exit(2); }
            return argv[++i];
        };
        int mine = 0;
        if (a == "-r" || a == "--reference") c.ref = next();
        else if (a == "-o" || a == "--output") c.out = next();
        else if (a == "-L" || a == "--contig") c.contig = next();
        else if (a == "--region") { if (!cli_region(next(), c.start, c.end)) return 2; c.has_region = true; }
        else if (a == "--min-depth") { if (!cli_min_depth(next(), c.min_depth)) return 2; }
        else if (a == "--min-quality") { if (!cli_min_quality(next(), c.min_quality)) return 2; }
        else if (a == "--min-base-quality") { if (!cli_base_quality(next(), c.min_base_quality)) return 2; c.has_min_base_quality = 1; c.filter_flag = true; }
        else if (a == "--exclude-flags") { if (!cli_flag_mask(next(), c.exclude_flags)) return 2; c.filter_flag = true; }
        else if (a == "--device") c.device = atoi(next());
        else if (a == "-h" || a == "--help") { c.usage(); return 0; }
        else if ((mine = own(a, next)) != 0) { if (mine < 0) return 2; }
        else if (!a.empty() && a[0] != '-' && c.bam.empty()) c.bam = a;
        else { fprintf(stderr, "error: unexpected argument '%s'\n", argv[i]); c.usage(); return 2; }
    }
    if (c.bam.empty() || c.ref.empty() || c.out.empty()) { c.usage(); return 2; }
    if (c.contig.empty()) { fprintf(stderr, "error: %s needs '-L <CONTIG>'\n", c.name); c.usage(); return 2; }
    return -1;
}

// the three flags of a rule of a count and a fraction, --min-STEM-fraction, --min-STEM-count and --min-STEM-per-strand, for own()
template <class Next>
static int cli_rule_flags(const std::string &a, Next &&next, const std::string &stem, int (*parse)(const char *, uint32_t *, char *, size_t),
                          uint32_t &per_10k, uint32_t &count, uint32_t &per_strand)
{
    const std::string fraction = "--min-" + stem + "-fraction", cnt = "--min-" + stem + "-count", strand = "--min-" + stem + "-per-strand";
    if (a == fraction) {
        const std::string v = next();
        char why[128] = {0};
        if (parse(v.c_str(), &per_10k, why, sizeof(why)) == CL_OK) return 1;
        fprintf(stderr, "error: invalid value '%s' for '%s': %s\n", v.c_str(), fraction.c_str(), why);
        return -1;
    }
    if (a == cnt) {
        const std::string v = next();
        if (!cli_count32(cnt.c_str(), v, count)) return -1;
        if (count == 0) { fprintf(stderr, "error: invalid value '%s' for '%s': at least 1\n", v.c_str(), cnt.c_str()); return -1; }
        return 1;
    }
    if (a == strand) return cli_count32(strand.c_str(), next(), per_strand) ? 1 : -1;
    return 0;
}

// the end of a scan subcommand: outputs are closed; skip the HIP runtime's exit handlers (see main)
static int scan_cli_leave(int rc, const char *err)
{
    if (rc != CL_OK) fprintf(stderr, "Error: %s\n", err);
    fflush(nullptr);
    _exit(rc != CL_OK ? 1 : 0);
}

static void usage_fv()
{
    fprintf(stderr, "Usage: dut-coverage find-variants <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END]\n"
                    "       [--min-depth 10] [--min-quality 20] [--tree FILE [--provider ftdna|decodingus] [--tree-type y|mt]] [--device 0]\n"
                    "       [--min-base-quality Q] [--exclude-flags MASK] [--min-alt-per-strand K]\n"
                    "  --region: 0-based, half open, within the contig.  SNVs only.  Without the last three flags every fetched\n"
                    "  record counts (no flag or base-quality filter), as in find-y-branch.  With any of them: bases below Q\n"
                    "  (0..255) and reads with a flag bit of MASK (decimal or 0x hex, 0..65535) do not count, the TSV gains\n"
                    "  alt_fwd alt_rev ref_fwd ref_rev filter, and filter is 'strand' when min(alt_fwd, alt_rev) < K.\n");
}

// find-variants: every position of a contig (or of --region, 0-based half open) where the sample's called base differs
// from the reference, by the counting and the call of find-y-branch (defaults as there, src/cli.rs:62-105); with --tree,
// which of them the haplogroup tree knows.
static int find_variants_main(int argc, char **argv)
{
    ScanCli c = {"find-variants", usage_fv};
    std::string tree;
    int provider = DUT_PROVIDER_FTDNA, tree_type = DUT_TREE_YDNA;
    bool has_provider = false, has_tree_type = false;
    dut_variants_options vopt = {0, 0, 0, 0, 0};
    const int st = scan_cli_parse(argc, argv, c, [&](const std::string &a, auto &&next) {
        if (a == "--tree") tree = next();
        else if (a == "--min-alt-per-strand") { if (!cli_count32("--min-alt-per-strand", next(), vopt.min_alt_per_strand)) return -1; vopt.filtered = 1; }
        else if (a == "--provider") {
            const std::string p = next();
            if (p == "ftdna") provider = DUT_PROVIDER_FTDNA;
            else if (p == "decodingus") provider = DUT_PROVIDER_DECODINGUS;
            else { fprintf(stderr, "error: invalid value '%s' for '--provider'\n", p.c_str()); return -1; }
            has_provider = true;
        }
        else if (a == "--tree-type") {
            const std::string p = next();
            if (p == "y") tree_type = DUT_TREE_YDNA;
            else if (p == "mt") tree_type = DUT_TREE_MTDNA;
            else { fprintf(stderr, "error: invalid value '%s' for '--tree-type'\n", p.c_str()); return -1; }
            has_tree_type = true;
        }
        else return 0;
        return 1;
    });
    if (st >= 0) return st;
    if ((has_provider || has_tree_type) && tree.empty()) { fprintf(stderr, "error: '--provider' and '--tree-type' need '--tree <FILE>'\n"); return 2; }
    c.filter_into(vopt);
    if (c.filter_flag) vopt.filtered = 1;
    char err[1024] = {0};
    return scan_cli_leave(dut_find_variants_files_ex(c.bam.c_str(), c.ref.c_str(), c.contig.c_str(), c.has_region ? 1 : 0, (uint32_t)c.start, (uint32_t)c.end,
                                                     tree.empty() ? nullptr : tree.c_str(), provider, tree_type, c.out.c_str(), (uint32_t)c.min_depth,
                                                     (uint8_t)c.min_quality, &vopt, c.device, err, sizeof(err)), err);
}

static void usage_fm()
{
    fprintf(stderr, "Usage: dut-coverage find-minor-alleles <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END]\n"
                    "       [--min-depth 10] [--min-quality 20] [--min-minor-fraction 0.05] [--min-minor-count 3]\n"
                    "       [--min-base-quality Q] [--exclude-flags MASK] [--min-minor-per-strand K] [--device 0]\n"
                    "  A position is listed when it is at least --min-depth deep and the second most frequent of A C G T has at\n"
                    "  least --min-minor-count observations and --min-minor-fraction of the depth (a decimal in (0, 0.5], at most\n"
                    "  four decimals).  --region: 0-based, half open.  Q, MASK as in find-variants; filter is 'strand' when\n"
                    "  min(minor_fwd, minor_rev) < K.  SNVs only, one device.\n");
}

// find-minor-alleles: every position of a contig (or of --region) where a second base of A C G T stands beside the most
// frequent one -- at least --min-minor-count observations and --min-minor-fraction of the depth (cl_site_scan_minor).
// Counting as in find-variants with its filter flags.
static int find_minor_main(int argc, char **argv)
{
    ScanCli c = {"find-minor-alleles", usage_fm};
    dut_minor_options mopt = {10, 20, 0, 0, 0, 500, 3, 0};
    const int st = scan_cli_parse(argc, argv, c, [&](const std::string &a, auto &&next) {
        return cli_rule_flags(a, next, "minor", dut_minor_fraction_parse, mopt.min_minor_per_10k, mopt.min_minor_count, mopt.min_minor_per_strand);
    });
    if (st >= 0) return st;
    c.filter_into(mopt);
    mopt.min_depth = (uint32_t)c.min_depth; mopt.min_quality = (uint8_t)c.min_quality;
    char err[1024] = {0};
    return scan_cli_leave(dut_find_minor_files(c.bam.c_str(), c.ref.c_str(), c.contig.c_str(), c.has_region ? 1 : 0, (uint32_t)c.start, (uint32_t)c.end, &mopt,
                                               c.out.c_str(), c.device, err, sizeof(err)), err);
}

static void usage_fd()
{
    fprintf(stderr, "Usage: dut-coverage find-deletions <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END]\n"
                    "       [--min-depth 10] [--min-quality 20] [--min-del-fraction 0.7] [--min-del-count 3]\n"
                    "       [--min-base-quality Q] [--exclude-flags MASK] [--min-del-per-strand K] [--device 0]\n"
                    "  A position is listed when bases plus deletions there are at least --min-depth and the reads with a D\n"
                    "  operation over it are at least --min-del-count and --min-del-fraction of that sum (a decimal in (0, 1], at\n"
                    "  most four decimals).  One line per run of consecutive positions.  --region: 0-based, half open.  Q, MASK as\n"
                    "  in find-variants; filter is 'strand' when min(del_fwd, del_rev) < K.  Deletions only, one device.\n");
}

// find-deletions: every position of a contig (or of --region) that the reads delete -- at least --min-del-count reads with a
// D operation over it and --min-del-fraction of depth + deletions (cl_site_scan_dels) -- merged into events of consecutive
// positions.  Counting as in find-variants with its filter flags.
static int find_deletions_main(int argc, char **argv)
{
    ScanCli c = {"find-deletions", usage_fd};
    dut_del_options dopt = {10, 20, 0, 0, 0, 7000, 3, 0};
    const int st = scan_cli_parse(argc, argv, c, [&](const std::string &a, auto &&next) {
        return cli_rule_flags(a, next, "del", dut_del_fraction_parse, dopt.min_del_per_10k, dopt.min_del_count, dopt.min_del_per_strand);
    });
    if (st >= 0) return st;
    c.filter_into(dopt);
    dopt.min_depth = (uint32_t)c.min_depth; dopt.min_quality = (uint8_t)c.min_quality;
    char err[1024] = {0};
    return scan_cli_leave(dut_find_deletions_files(c.bam.c_str(), c.ref.c_str(), c.contig.c_str(), c.has_region ? 1 : 0, (uint32_t)c.start, (uint32_t)c.end, &dopt,
                                                   c.out.c_str(), c.device, err, sizeof(err)), err);
}

static void usage_fi()
{
    fprintf(stderr, "Usage: dut-coverage find-insertions <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END]\n"
                    "       [--min-depth 10] [--min-quality 20] [--min-ins-fraction 0.7] [--min-ins-count 3]\n"
                    "       [--min-base-quality Q] [--exclude-flags MASK] [--min-ins-per-strand K] [--device 0]\n"
                    "  A position is listed when it is at least --min-depth deep and the reads with an I operation directly behind\n"
                    "  their base there are at least --min-ins-count and --min-ins-fraction of the depth (a decimal in (0, 1], at\n"
                    "  most four decimals).  pos is the base before the insertion; the most frequent inserted sequence is shown\n"
                    "  (its first 32 bases).  --region: 0-based, half open.  Q, MASK as in find-variants; filter is 'strand' when\n"
                    "  min(ins_fwd, ins_rev) < K.  Insertions only, no left-alignment, one device.\n");
}

// find-insertions: every position of a contig (or of --region) behind whose base the reads insert something -- at least
// --min-ins-count reads with an I operation anchored there and --min-ins-fraction of the depth (cl_site_scan_ins) -- with the
// inserted alleles.  Counting as in find-variants with its filter flags.
static int find_insertions_main(int argc, char **argv)
{
    ScanCli c = {"find-insertions", usage_fi};
    dut_ins_options iopt = {10, 20, 0, 0, 0, 7000, 3, 0};
    const int st = scan_cli_parse(argc, argv, c, [&](const std::string &a, auto &&next) {
        return cli_rule_flags(a, next, "ins", dut_del_fraction_parse, iopt.min_ins_per_10k, iopt.min_ins_count, iopt.min_ins_per_strand);
    });
    if (st >= 0) return st;
    c.filter_into(iopt);
    iopt.min_depth = (uint32_t)c.min_depth; iopt.min_quality = (uint8_t)c.min_quality;
    char err[1024] = {0};
    return scan_cli_leave(dut_find_insertions_files(c.bam.c_str(), c.ref.c_str(), c.contig.c_str(), c.has_region ? 1 : 0, (uint32_t)c.start, (uint32_t)c.end, &iopt,
                                                    c.out.c_str(), c.device, err, sizeof(err)), err);
}

static void usage_cs()
{
    fprintf(stderr, "Usage: dut-coverage consensus <BAM_FILE> -r <REFERENCE_FILE> -o <FASTA> -L <CONTIG> [--region START-END]\n"
                    "       [--min-depth 10] [--min-quality 20] [--min-del-fraction 0.7] [--min-del-count 3]\n"
                    "       [--min-ins-fraction 0.7] [--min-ins-count 3] [--min-base-quality Q] [--exclude-flags MASK]\n"
                    "       [--fill N|ref] [--line-width 60] [--changes FILE] [--device 0]\n"
                    "  The sample's sequence over the contig or --region (0-based, half open): per position the called base (0.7 of\n"
                    "  the depth, as find-variants calls it), nothing where find-deletions would call a deletion, N where the column\n"
                    "  is mixed or too shallow (--fill ref: the lower-cased reference base where it is too shallow); behind a\n"
                    "  position where find-insertions calls an insertion, its most frequent allele of at most 32 bases.  --changes:\n"
                    "  a tab separated list of every difference from the reference.  No left-alignment, one device.\n");
}

// consensus: the called sequence of a contig or a region as FASTA (cl_site_scan_consensus for the bytes, cl_site_scan_ins for
// what is spliced in), and the list of its differences from the reference.  Counting as in find-variants with its filter flags.
static int consensus_main(int argc, char **argv)
{
    ScanCli c = {"consensus", usage_cs};
    dut_cons_options o = {10, 20, 0, 0, 0, 7000, 3, 7000, 3, 0, 60};
    std::string changes;
    const int st = scan_cli_parse(argc, argv, c, [&](const std::string &a, auto &&next) {
        auto fraction = [&](uint32_t &dst) {
            const std::string v = next();
            char why[128] = {0};
            if (dut_del_fraction_parse(v.c_str(), &dst, why, sizeof(why)) == CL_OK) return 1;
            fprintf(stderr, "error: invalid value '%s' for '%s': %s\n", v.c_str(), a.c_str(), why);
            return -1;
        };
        auto count = [&](uint32_t &dst) {
            const std::string v = next();
            if (!cli_count32(a.c_str(), v, dst)) return -1;
            if (dst == 0) { fprintf(stderr, "error: invalid value '%s' for '%s': at least 1\n", v.c_str(), a.c_str()); return -1; }
            return 1;
        };
        if (a == "--min-del-fraction") return fraction(o.min_del_per_10k);
        if (a == "--min-ins-fraction") return fraction(o.min_ins_per_10k);
        if (a == "--min-del-count") return count(o.min_del_count);
        if (a == "--min-ins-count") return count(o.min_ins_count);
        if (a == "--line-width") return count(o.line_width);
        if (a == "--changes") { changes = next(); return 1; }
        if (a == "--fill") {
            const std::string v = next();
            if (v == "N") o.fill_ref = 0;
            else if (v == "ref") o.fill_ref = 1;
            else { fprintf(stderr, "error: invalid value '%s' for '--fill'\n  [possible values: N, ref]\n", v.c_str()); return -1; }
            return 1;
        }
        return 0;
    });
    if (st >= 0) return st;
    c.filter_into(o);
    o.min_depth = (uint32_t)c.min_depth; o.min_quality = (uint8_t)c.min_quality;
    char err[1024] = {0};
    return scan_cli_leave(dut_find_consensus_files(c.bam.c_str(), c.ref.c_str(), c.contig.c_str(), c.has_region ? 1 : 0, (uint32_t)c.start, (uint32_t)c.end, &o,
                                                   c.out.c_str(), changes.empty() ? nullptr : changes.c_str(), c.device, err, sizeof(err)), err);
}

static void usage_fs()
{
    fprintf(stderr, "Usage: dut-coverage find-strs <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> --loci FILE [--flank 5]\n"
                    "       [--min-depth 10] [--min-quality 20] [--min-allele-fraction 0.7] [--exclude-flags MASK] [--device 0]\n"
                    "  The allele length of every short tandem repeat of FILE on the contig (tab separated: contig start end period\n"
                    "  name, 0-based half open, at most 1024 positions long): the bases each read holds between the two flanks of\n"
                    "  --flank matched bases (1..64), counted over the reads that span the locus, wherever their aligner put the\n"
                    "  gaps.  A locus is called when at least --min-depth reads span it and one length holds --min-allele-fraction\n"
                    "  of them (a decimal in (0, 1], at most four decimals).  MASK as in find-variants.  Lengths only, one device.\n");
}

// find-strs: per locus of a user-supplied catalogue the histogram of spanning reads' lengths (cl_site_str_lengths) and the
// allele it supports, in repeat units.  Argument errors leave with 2 before a device is opened.
static int find_strs_main(int argc, char **argv)
{
    ScanCli c = {"find-strs", usage_fs};
    dut_str_options o = {10, 20, 0, 5, 7000};
    std::string loci;
    const int st = scan_cli_parse(argc, argv, c, [&](const std::string &a, auto &&next) {
        if (a == "--loci") { loci = next(); return 1; }
        if (a == "--flank") {
            const std::string v = next();
            if (!cli_count32("--flank", v, o.flank)) return -1;
            if (o.flank < 1 || o.flank > CL_STR_MAX_FLANK) { fprintf(stderr, "error: invalid value '%s' for '--flank': 1..%u\n", v.c_str(), (unsigned)CL_STR_MAX_FLANK); return -1; }
            return 1;
        }
        if (a == "--min-allele-fraction") {
            const std::string v = next();
            char why[128] = {0};
            if (dut_del_fraction_parse(v.c_str(), &o.min_allele_per_10k, why, sizeof(why)) == CL_OK) return 1;
            fprintf(stderr, "error: invalid value '%s' for '--min-allele-fraction': %s\n", v.c_str(), why);
            return -1;
        }
        return 0;
    });
    if (st >= 0) return st;
    if (loci.empty()) { fprintf(stderr, "error: find-strs needs '--loci <FILE>'\n"); usage_fs(); return 2; }
    if (c.has_region || c.has_min_base_quality) { fprintf(stderr, "error: find-strs takes neither '--region' nor '--min-base-quality'\n"); usage_fs(); return 2; }
    o.min_depth = (uint32_t)c.min_depth; o.min_quality = (uint8_t)c.min_quality; o.exclude_flags = c.exclude_flags;
    char err[1024] = {0};
    return scan_cli_leave(dut_find_strs_files(c.bam.c_str(), c.ref.c_str(), c.contig.c_str(), loci.c_str(), &o, c.out.c_str(), c.device, err, sizeof(err)), err);
}

static void usage_ep()
{
    fprintf(stderr, "Usage: dut-coverage error-profile <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> [--region START-END] [--cycles 50]\n"
                    "       [--min-quality 20] [--min-base-quality Q] [--exclude-flags MASK] [--device 0]\n"
                    "  The sample's own error rates over the contig (or --region, 0-based half open): substitutions by reference\n"
                    "  base and read base in the orientation the molecule was sequenced in, the same by distance from the read's 5'\n"
                    "  and 3' end for the first --cycles positions (1..256), and insertion and deletion events by the same\n"
                    "  distances.  Q and MASK as in find-variants.  One contig, one device.\n");
}

// error-profile: the read-centric table of mismatches, insertions and deletions by cycle (cl_site_error_profile).  Argument
// errors leave with 2 before a device is opened.
static int error_profile_main(int argc, char **argv)
{
    ScanCli c = {"error-profile", usage_ep};
    dut_ep_options o = {20, 1, 0, 0, 0, 50};
    const int st = scan_cli_parse(argc, argv, c, [&](const std::string &a, auto &&next) {
        if (a != "--cycles") return 0;
        const std::string v = next();
        if (!cli_count32("--cycles", v, o.n_cycles)) return -1;
        if (o.n_cycles < 1 || o.n_cycles > CL_EP_MAX_CYCLES) { fprintf(stderr, "error: invalid value '%s' for '--cycles': 1..%u\n", v.c_str(), (unsigned)CL_EP_MAX_CYCLES); return -1; }
        return 1;
    });
    if (st >= 0) return st;
    o.min_quality = (uint8_t)c.min_quality;
    c.filter_into(o);
    char err[1024] = {0};
    return scan_cli_leave(dut_error_profile_files(c.bam.c_str(), c.ref.c_str(), c.contig.c_str(), c.has_region ? 1 : 0, (uint32_t)c.start, (uint32_t)c.end, &o,
                                                  c.out.c_str(), c.device, err, sizeof(err)), err);
}

static void usage_ps()
{
    fprintf(stderr, "Usage: dut-coverage phase-sites <BAM_FILE> -r <REFERENCE_FILE> -o <TSV> -L <CONTIG> --sites FILE [--max-dist 1000]\n"
                    "       [--max-partners 4] [--min-depth 10] [--min-quality 20] [--min-link-count 3] [--max-discordance 0.05]\n"
                    "       [--min-base-quality Q] [--exclude-flags MASK] [--device 0]\n"
                    "  Whether the second alleles of two nearby sites ride on the same reads.  FILE is tab separated, column 1 the\n"
                    "  contig, column 2 a 1-based position (the TSVs of find-variants, find-minor-alleles and find-deletions as they\n"
                    "  are).  Every site is paired with the next --max-partners sites (1..15) within --max-dist positions; per pair\n"
                    "  the reads that cover the first site are counted by what they show at both.  A pair is cis when at least\n"
                    "  --min-link-count reads carry both minor alleles and at most --max-discordance (a decimal in [0, 0.4999], at\n"
                    "  most four decimals) of the reads with a minor allele carry only one; trans when each minor allele has that\n"
                    "  many reads without the other and as few carry both.  Q and MASK as in find-variants.  Reads only, no mates.\n");
}

// phase-sites: the joint allele counts of site pairs per read (cl_site_link_counts) and the integer rule over them.  Argument
// errors leave with 2 before a device is opened.
static int phase_sites_main(int argc, char **argv)
{
    ScanCli c = {"phase-sites", usage_ps};
    dut_link_options o = {10, 20, 1, 0, 0, 0, 1000, 4, 3, 500};
    std::string sites;
    const int st = scan_cli_parse(argc, argv, c, [&](const std::string &a, auto &&next) {
        if (a == "--sites") { sites = next(); return 1; }
        if (a == "--max-dist" || a == "--max-partners" || a == "--min-link-count") {
            const std::string v = next();
            uint32_t &dst = a == "--max-dist" ? o.max_dist : a == "--max-partners" ? o.max_partners : o.min_link_count;
            if (!cli_count32(a.c_str(), v, dst)) return -1;
            const uint32_t most = a == "--max-partners" ? (uint32_t)CL_LINK_MAX_PARTNERS : 0xFFFFFFFFu;
            if (dst < 1 || dst > most) { fprintf(stderr, "error: invalid value '%s' for '%s': 1..%u\n", v.c_str(), a.c_str(), most); return -1; }
            return 1;
        }
        if (a == "--max-discordance") {
            const std::string v = next();
            char why[128] = {0};
            if (dut_link_discordance_parse(v.c_str(), &o.max_discord_per_10k, why, sizeof(why)) == CL_OK) return 1;
            fprintf(stderr, "error: invalid value '%s' for '--max-discordance': %s\n", v.c_str(), why);
            return -1;
        }
        return 0;
    });
    if (st >= 0) return st;
    if (sites.empty()) { fprintf(stderr, "error: phase-sites needs '--sites <FILE>'\n"); usage_ps(); return 2; }
    if (c.has_region) { fprintf(stderr, "error: phase-sites takes no '--region'\n"); usage_ps(); return 2; }
    o.min_depth = (uint32_t)c.min_depth; o.min_quality = (uint8_t)c.min_quality;
    c.filter_into(o);
    char err[1024] = {0};
    return scan_cli_leave(dut_find_links_files(c.bam.c_str(), c.ref.c_str(), c.contig.c_str(), sites.c_str(), &o, c.out.c_str(), c.device, err, sizeof(err)), err);
}

// DUT_TIMING=1: the wall clock (CLOCK_REALTIME, seconds) at the start of main and right before the process leaves, so
// that a harness that started the tool can tell what the loader took before main and what the exit took after it
static void stamp(const char *what)
{
    const char *e = getenv("DUT_TIMING");
    if (!e || *e != '1') return;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    fprintf(stderr, "[dut-timing] wall clock at %s: %.6f\n", what, (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec);
}

int main(int argc, char **argv)
{
    stamp("main");
    if (argc > 1 && !strcmp(argv[1], "find-y-branch")) return find_branch_main(argc, argv, DUT_TREE_YDNA);
    if (argc > 1 && !strcmp(argv[1], "find-mt-branch")) return find_branch_main(argc, argv, DUT_TREE_MTDNA);
    if (argc > 1 && !strcmp(argv[1], "fingerprint")) return fingerprint_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "fingerprint-compare")) return fingerprint_compare_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "find-variants")) return find_variants_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "find-minor-alleles")) return find_minor_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "find-deletions")) return find_deletions_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "find-insertions")) return find_insertions_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "consensus")) return consensus_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "find-strs")) return find_strs_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "error-profile")) return error_profile_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "phase-sites")) return phase_sites_main(argc, argv);
    cl_options opt = {4, 500, 10, 20, 10, 1, 0.1};      // src/cli.rs:34-60
    std::string bam, ref, out = "callable_regions.bed", summary = "summary.html";
    std::vector<const char *> contigs;
    std::vector<int> devices;
    std::string depth_dist, depth_windows, depth_summary;
    unsigned long long depth_cap = 1000, depth_window = 0;
    bool has_window = false;
    std::string depth_bed, depth_bed_kind, quantize;
    bool has_kind = false, has_quantize = false;
    std::string targets_bed, target_out, target_thr;
    bool has_target_thr = false, target_quantiles = false;
    std::string gc_bias, gc_summary;
    unsigned long long gc_window = 100, gc_max_n = 4;
    bool has_gc_window = false, has_gc_max_n = false;
    // a whole non-negative number, or exit 2 with a message (before any device is opened)
    auto number = [](const char *flag, const char *v) -> unsigned long long {
        char *end = nullptr;
        errno = 0;
        const unsigned long long x = (*v && *v != '-') ? strtoull(v, &end, 10) : 0ull;
        if (!*v || *v == '-' || errno || *end) { fprintf(stderr, "error: invalid value '%s' for '%s'\n", v, flag); exit(2); }
        return x;
    };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        std::string val;
        const size_t eq = a.find('=');
        const bool has_eq = a.rfind("--", 0) == 0 && eq != std::string::npos;
        if (has_eq) { val = a.substr(eq + 1); a = a.substr(0, eq); }
        auto next = [&]() -> const char * {
            if (has_eq) return val.c_str();
            if (i + 1 >= argc) { usage(); exit(2); }
            return argv[++i];
        };
        if (a == "coverage" && bam.empty()) continue;
        else if (a == "-r" || a == "--reference") ref = next();
        else if (a == "-o" || a == "--output") out = next();
        else if (a == "-s" || a == "--summary") summary = next();
        else if (a == "-L" || a == "--contig") contigs.push_back(strdup(next()));
        else if (a == "--min-depth") opt.min_depth = (uint32_t)strtoul(next(), nullptr, 10);
        else if (a == "--max-depth") opt.max_depth = (uint32_t)strtoul(next(), nullptr, 10);
        else if (a == "--min-mapping-quality") opt.min_mapping_quality = (uint8_t)strtoul(next(), nullptr, 10);
        else if (a == "--min-base-quality") opt.min_base_quality = (uint8_t)strtoul(next(), nullptr, 10);
        else if (a == "--min-depth-for-low-mapq") opt.min_depth_for_low_mapq = (uint32_t)strtoul(next(), nullptr, 10);
        else if (a == "--max-low-mapq") opt.max_low_mapq = (uint8_t)strtoul(next(), nullptr, 10);
        else if (a == "--max-low-mapq-fraction") opt.max_low_mapq_fraction = strtod(next(), nullptr);
        else if (a == "--depth-dist") depth_dist = next();
        else if (a == "--depth-windows") depth_windows = next();
        else if (a == "--depth-summary") depth_summary = next();
        else if (a == "--depth-cap") depth_cap = number("--depth-cap", next());
        else if (a == "--window") { depth_window = number("--window", next()); has_window = true; }
        else if (a == "--depth-bed") depth_bed = next();
        else if (a == "--depth-bed-kind") { depth_bed_kind = next(); has_kind = true; }
        else if (a == "--quantize") { quantize = next(); has_quantize = true; }
        else if (a == "--targets") targets_bed = next();
        else if (a == "--target-out") target_out = next();
        else if (a == "--target-thresholds") { target_thr = next(); has_target_thr = true; }
        else if (a == "--target-quantiles") target_quantiles = true;
        else if (a == "--gc-bias") gc_bias = next();
        else if (a == "--gc-summary") gc_summary = next();
        else if (a == "--gc-window") { gc_window = number("--gc-window", next()); has_gc_window = true; }
        else if (a == "--gc-max-n") { gc_max_n = number("--gc-max-n", next()); has_gc_max_n = true; }
        else if (a == "--device") devices.assign(1, atoi(next()));
        else if (a == "--devices") {
            // the contigs are dealt to these devices (HIP ordinals, comma separated; an ordinal may repeat)
            devices.clear();
            const std::string list = next();
            for (size_t b = 0; b <= list.size();) {
                const size_t e = std::min(list.find(',', b), list.size());
                if (e > b) devices.push_back(atoi(list.substr(b, e - b).c_str()));
                b = e + 1;
            }
            if (devices.empty()) { fprintf(stderr, "error: invalid value '%s' for '--devices'\n", list.c_str()); return 2; }
        }
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else if (!a.empty() && a[0] != '-' && bam.empty()) bam = a;
        else { fprintf(stderr, "error: unexpected argument '%s'\n", argv[i]); usage(); return 2; }
    }
    if (bam.empty() || ref.empty()) { usage(); return 2; }
    // the depth profile's arguments, checked before a device is opened
    if (depth_cap < 1 || depth_cap > CL_DEPTH_MAX_BINS - 1) { fprintf(stderr, "error: invalid value '%llu' for '--depth-cap': 1..%u\n", depth_cap, CL_DEPTH_MAX_BINS - 1); return 2; }
    if (has_window && (depth_window < CL_DEPTH_MIN_WINDOW || depth_window > 0xFFFFFFFFull)) { fprintf(stderr, "error: invalid value '%llu' for '--window': at least %u positions\n", depth_window, CL_DEPTH_MIN_WINDOW); return 2; }
    if (!depth_windows.empty() && !has_window) { fprintf(stderr, "error: '--depth-windows' needs '--window <S>' (S >= %u)\n", CL_DEPTH_MIN_WINDOW); return 2; }
    if (has_window && depth_windows.empty()) { fprintf(stderr, "error: '--window' needs '--depth-windows <FILE>'\n"); return 2; }
    dut_depth_options depth = {(uint32_t)depth_cap + 1u, (uint32_t)depth_window, depth_dist.empty() ? nullptr : depth_dist.c_str(),
                               depth_windows.empty() ? nullptr : depth_windows.c_str(), depth_summary.empty() ? nullptr : depth_summary.c_str()};
    // ... and the depth BED's
    if (has_kind && depth_bed.empty()) { fprintf(stderr, "error: '--depth-bed-kind' needs '--depth-bed <FILE>'\n"); return 2; }
    if (has_quantize && depth_bed.empty()) { fprintf(stderr, "error: '--quantize' needs '--depth-bed <FILE>'\n"); return 2; }
    if (has_kind && depth_bed_kind != "raw" && depth_bed_kind != "qc") {
        fprintf(stderr, "error: invalid value '%s' for '--depth-bed-kind'\n  [possible values: raw, qc]\n", depth_bed_kind.c_str());
        return 2;
    }
    uint32_t edges[CL_RUNS_MAX_EDGES] = {0}, n_edges = 0;
    if (has_quantize) {
        char why[256] = {0};
        if (dut_quantize_parse(quantize.c_str(), edges, &n_edges, why, sizeof(why)) != CL_OK) {
            fprintf(stderr, "error: invalid value '%s' for '--quantize': %s\n", quantize.c_str(), why);
            return 2;
        }
    }
    if (!target_out.empty() && targets_bed.empty()) { fprintf(stderr, "error: '--target-out' needs '--targets <BED>'\n"); return 2; }
    if (target_quantiles && targets_bed.empty()) { fprintf(stderr, "error: '--target-quantiles' needs '--targets <BED>'\n"); return 2; }
    if (has_target_thr && targets_bed.empty()) { fprintf(stderr, "error: '--target-thresholds' needs '--targets <BED>'\n"); return 2; }
    if (!targets_bed.empty() && target_out.empty()) { fprintf(stderr, "error: '--targets' needs '--target-out <FILE>'\n"); return 2; }
    uint32_t thresholds[CL_TARGET_MAX_THRESHOLDS] = {0}, n_thresholds = 0;
    if (!targets_bed.empty()) {
        char why[512] = {0};
        if (dut_thresholds_parse(has_target_thr ? target_thr.c_str() : nullptr, thresholds, &n_thresholds, why, sizeof(why)) != CL_OK) {
            fprintf(stderr, "error: invalid value '%s' for '--target-thresholds': %s\n", target_thr.c_str(), why);
            return 2;
        }
        // (read here once for its mistakes, before a device is opened; the library reads it again)
        dut_targets *tg = dut_targets_read(targets_bed.c_str(), why, sizeof(why));
        if (!tg) { fprintf(stderr, "error: invalid value for '--targets': %s\n", why); return 2; }
        dut_targets_free(tg);
    }
    const dut_target_options target_opt = {targets_bed.empty() ? nullptr : targets_bed.c_str(), target_out.empty() ? nullptr : target_out.c_str(),
                                           thresholds, n_thresholds};
    // ... and the GC bias's
    if ((has_gc_window || has_gc_max_n) && gc_bias.empty() && gc_summary.empty()) { fprintf(stderr, "error: '%s' needs '--gc-bias <FILE>' or '--gc-summary <FILE>'\n", has_gc_window ? "--gc-window" : "--gc-max-n"); return 2; }
    if (gc_window < 1 || gc_window > CL_GC_MAX_WINDOW) { fprintf(stderr, "error: invalid value '%llu' for '--gc-window': 1..%d\n", gc_window, CL_GC_MAX_WINDOW); return 2; }
    if (gc_max_n >= gc_window) { fprintf(stderr, "error: invalid value '%llu' for '--gc-max-n': below the window of %llu\n", gc_max_n, gc_window); return 2; }
    const dut_gc_options gc_opt = {gc_bias.empty() ? nullptr : gc_bias.c_str(), gc_summary.empty() ? nullptr : gc_summary.c_str(), (uint32_t)gc_window, (uint32_t)gc_max_n};
    const dut_depth_bed_options depth_bed_opt = {depth_bed.empty() ? nullptr : depth_bed.c_str(),
                                                 depth_bed_kind == "qc" ? (uint32_t)CL_DEPTH_QC : (uint32_t)CL_DEPTH_RAW, edges, n_edges};
    if (devices.empty()) devices.push_back(0);
    // The analysis runs in a child process and this one returns as soon as the child reports that every output file is
    // written and closed: what is left then -- the kernel taking a few gigabytes of decode buffers, the pinned staging
    // memory and the device context apart, 0.1 to 0.5 s depending on the box -- happens in the background, after the
    // command has returned (the child closes its output streams first, so a caller that reads them to their end does
    // not wait for it either).  Forked before anything touches the GPU.  DUT_CLI_FOREGROUND=1: one process, the caller
    // waits for the teardown too.
    int status_fd = -1;
    {
        const char *fg = getenv("DUT_CLI_FOREGROUND");
        int fds[2];
        if (!(fg && *fg == '1') && pipe(fds) == 0) {
            const pid_t pid = fork();
            if (pid > 0) {
                close(fds[1]);
                unsigned char code = 0;
                ssize_t g;
                do { g = read(fds[0], &code, 1); } while (g < 0 && errno == EINTR);
                if (g == 1) { stamp("return (the child goes on releasing)"); _exit(code); }
                int st = 0;                                   // the child ended without a word: its own status tells
                while (waitpid(pid, &st, 0) < 0 && errno == EINTR) {}
                _exit(WIFEXITED(st) ? WEXITSTATUS(st) : 1);
            }
            if (pid == 0) { close(fds[0]); status_fd = fds[1]; }
            else { close(fds[0]); close(fds[1]); }            // no fork: in the foreground
        }
    }
    auto leave = [&](int code) {
        fflush(nullptr);
        if (status_fd >= 0) {
            const unsigned char b = (unsigned char)code;
            if (write(status_fd, &b, 1) != 1) {}
            close(status_fd);
            close(1); close(2);                               // readers of the tool's output see its end now
        }
        _exit(code);
    };
    char err[1024] = {0};
    // this process ends with the analysis: what the library holds (device contexts, readers, decode buffers) is left to
    // the exit (DUT_CLI_TEARDOWN=1: given back piece by piece first, as a library caller's process would)
    const char *td = getenv("DUT_CLI_TEARDOWN");
    const unsigned flags = (td && *td == '1') ? 0u : DUT_FILES_LEAVE_TO_EXIT;
    const int rc = dut_coverage_files_ex5(bam.c_str(), ref.c_str(), out.c_str(), "summary.json", summary.c_str(), &opt,
                                          contigs.empty() ? nullptr : contigs.data(), contigs.size(), devices.data(), devices.size(),
                                          flags, &depth, &depth_bed_opt, &target_opt, target_quantiles ? DUT_TARGETS_ORDER : 0u, &gc_opt, err, sizeof(err));
    if (rc != CL_OK) { fprintf(stderr, "Error: Analysis error: %s\n", err); leave(1); }
    // every output file is written and closed: leave without the HIP runtime's exit handlers
    stamp("exit");
    leave(0);
    return 0;
}
