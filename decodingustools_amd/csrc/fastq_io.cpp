// fastq_io.cpp -- the FASTQ reader of the `fingerprint` path (include/dut_fingerprint.h; the reference's
// readers/fastq.rs on the bio crate): 4-line records, plain or gzip.  zlib's gzread reads a plain file as it
// is and goes on through the members of a multi-member gzip file (bgzipped FASTQ).
#include "../../include/dut_fingerprint.h"

#include <zlib.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct dut_fastq {
    gzFile gz = nullptr;
    std::string path;
    std::vector<char> buf;                  // bytes read and not yet consumed: [pos, end)
    size_t pos = 0, end = 0;
    bool eof = false, stopped = false;
    std::vector<uint64_t> off;
    std::vector<uint8_t> bases;
    std::string pend_seq;                   // a record read past the end of the previous batch
    bool has_pend = false;

    // the next line without its '\n' into [*s, *s + *n); false at the end of the file (no bytes left)
    bool line(const char **s, size_t *n)
    {
        for (size_t scan = pos;;) {
            const char *nl = scan < end ? (const char *)memchr(buf.data() + scan, '\n', end - scan) : nullptr;
            if (nl) {
                *s = buf.data() + pos; *n = (size_t)(nl - (buf.data() + pos));
                pos = (size_t)(nl - buf.data()) + 1;
                return true;
            }
            scan = end;
            if (eof) {
                if (pos == end) return false;
                *s = buf.data() + pos; *n = end - pos;       // last line without a newline
                pos = end;
                return true;
            }
            // keep [pos, end), read more behind it
            const size_t keep = end - pos;
            if (pos) { memmove(buf.data(), buf.data() + pos, keep); scan -= pos; pos = 0; end = keep; }
            if (buf.size() < end + (1u << 20)) buf.resize(std::max(buf.size() * 2, end + (size_t)(1u << 20)));
            const int g = gzread(gz, buf.data() + end, (unsigned)(buf.size() - end));
            if (g < 0) { eof = true; return false; }
            if (g == 0) eof = true;
            end += (size_t)g;
        }
    }
};

namespace {

void warn_stop(const dut_fastq *f, const char *why)
{
    fprintf(stderr, "warning: %s: %s; reading stops here\n", f->path.c_str(), why);
}

// one record's sequence (trailing whitespace trimmed) into seq; false at the end or where reading stops
bool next_record(dut_fastq *f, std::string &seq)
{
    if (f->stopped) return false;
    const char *s; size_t n;
    if (!f->line(&s, &n)) { f->stopped = true; return false; }
    // the id: the header after '@' up to the first whitespace
    if (n == 0 || (n == 1 && s[0] == '\r')) { f->stopped = true; return false; }      // blank line: no further record
    if (s[0] != '@') { warn_stop(f, "malformed FASTQ record (header without '@')"); f->stopped = true; return false; }
    size_t id_len = 0;
    while (1 + id_len < n && !isspace((unsigned char)s[1 + id_len])) ++id_len;
    if (id_len == 0) { warn_stop(f, "FASTQ record with an empty id"); f->stopped = true; return false; }
    if (!f->line(&s, &n)) { warn_stop(f, "incomplete FASTQ record"); f->stopped = true; return false; }
    while (n && isspace((unsigned char)s[n - 1])) --n;
    seq.assign(s, n);
    if (!f->line(&s, &n) || n == 0 || s[0] != '+') { warn_stop(f, "malformed FASTQ record (no '+' line)"); f->stopped = true; return false; }
    if (!f->line(&s, &n)) { warn_stop(f, "incomplete FASTQ record (no quality line)"); f->stopped = true; return false; }
    return true;
}

} // namespace

extern "C" {

dut_fastq *dut_fastq_open(const char *path, char *err, size_t err_len)
{
    if (!path) { if (err && err_len) snprintf(err, err_len, "null path"); return nullptr; }
    gzFile gz = gzopen(path, "rb");
    if (!gz) { if (err && err_len) snprintf(err, err_len, "cannot open %s", path); return nullptr; }
    gzbuffer(gz, 1u << 20);
    dut_fastq *f = new dut_fastq();
    f->gz = gz;
    f->path = path;
    return f;
}

int dut_fastq_next(dut_fastq *f, uint64_t max_bases, uint64_t *n_seq, const uint64_t **base_off, const uint8_t **bytes)
{
    if (!f || !n_seq || !base_off || !bytes) return CL_ERR_INVALID;
    try {
        f->off.clear(); f->bases.clear();
        std::string seq;
        for (;;) {
            if (f->has_pend) { seq.swap(f->pend_seq); f->has_pend = false; }
            else if (!next_record(f, seq)) break;
            if (!f->off.empty() && f->bases.size() + seq.size() > max_bases) { f->pend_seq.swap(seq); f->has_pend = true; break; }
            f->off.push_back(f->bases.size());
            f->bases.insert(f->bases.end(), seq.begin(), seq.end());
        }
        *n_seq = f->off.size();
        f->off.push_back(f->bases.size());
        if (f->bases.empty()) f->bases.push_back(0);       // a valid pointer for an empty batch
        *base_off = f->off.data(); *bytes = f->bases.data();
        return CL_OK;
    } catch (const std::bad_alloc &) { return CL_ERR_NOMEM; }
}

void dut_fastq_close(dut_fastq *f)
{
    if (!f) return;
    if (f->gz) gzclose(f->gz);
    delete f;
}

} // extern "C"
