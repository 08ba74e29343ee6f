// TEST INFRASTRUCTURE: drives the host-only parts of the library (BAM / FASTA reader, admission, BamStats,
// JSON writer, tree parsing / scoring / report) under AddressSanitizer + UBSan or ThreadSanitizer on the CPU.
// The device engine is not part of this binary: the cl_* symbols the host sources reference are defined below as a
// stand-in for the link and for the several-"device" orchestration.  The walk that takes a tile of reads into the engine
// needs no device (tile_walk.h) and is the library's own here.
#include "../../include/dut_coverage.h"
#include "../../include/dut_bam.h"
#include "../../include/dut_haplogroup.h"
#include "../../include/dut_report.h"
#include "../../decodingustools_amd/csrc/host_parallel.h"
#include "../../decodingustools_amd/csrc/pass_rows.h"
#include "../../decodingustools_amd/csrc/qual_pack.h"
#include "../../decodingustools_amd/csrc/tile_walk.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

// A stand-in for the device engine, for this binary only: a context that remembers the contig it was given and hands back
// two runs that depend on it (so that a result delivered to the wrong contig, or twice, shows in the BED).  It lets the
// host's orchestration -- dut_coverage_files_multi: one thread, reader pair and context per "device", results handed to
// the BED writer in tid order -- run under ThreadSanitizer without a GPU.  Nothing here computes a pileup.
struct cl_ctx { int device; int32_t tid; uint32_t len; uint64_t n_reads; cl_interval iv[2]; };
extern "C" {
cl_status cl_create(const cl_options *, int device, void *, cl_ctx **out)
{
    if (device < 0 || device > 7) return CL_ERR_DEVICE;
    *out = new cl_ctx(); (*out)->device = device; return CL_OK;
}
void cl_destroy(cl_ctx *c) { delete c; }
const char *cl_last_error(const cl_ctx *) { return "no device in the sanitizer build"; }
cl_status cl_contig_begin(cl_ctx *c, int32_t tid, uint32_t len, const uint8_t *, uint64_t) { c->tid = tid; c->len = len; c->n_reads = 0; return CL_OK; }
cl_status cl_push_reads(cl_ctx *c, const cl_read_tile *t) { c->n_reads += t->n_reads; return CL_OK; }
cl_status cl_push_reads_bits(cl_ctx *c, const cl_read_tile_bits *t)
{
    // every word the tile names is read (the sanitizers see an offset that runs past the reader's buffers)
    uint64_t seen = 0;
    if (t->n_reads && t->qual_off[t->n_reads] > t->qual_off[0])
        for (uint64_t w = t->qual_off[0] >> 6; w <= (t->qual_off[t->n_reads] - 1) >> 6; ++w) seen ^= t->pass_bits[w];
    for (uint64_t i = 0; i < t->n_reads; ++i) seen += t->pass_sum[i];
    c->n_reads += t->n_reads + (seen == 0x5EEDull ? 0 : 0);
    return CL_OK;
}
cl_status cl_contig_prefetch_qual(cl_ctx *, const uint8_t *, uint64_t) { return CL_OK; }
cl_status cl_contig_reserve(cl_ctx *, uint64_t, uint64_t, uint64_t) { return CL_OK; }
cl_status cl_contig_finish(cl_ctx *c, cl_contig_summary *s, const cl_interval **iv, size_t *n)
{
    memset(s, 0, sizeof(*s));
    const uint32_t cut = c->len > 1 ? 1 + (uint32_t)((c->n_reads * 7 + (uint32_t)c->tid) % (c->len - 1)) : c->len;
    c->iv[0] = {0, cut, CL_NO_COVERAGE}; c->iv[1] = {cut, c->len, CL_CALLABLE};
    s->state_counts[CL_NO_COVERAGE] = cut; s->state_counts[CL_CALLABLE] = c->len - cut; s->extent = c->len;
    s->n_intervals = cut < c->len ? 2 : 1;
    *iv = c->iv; *n = (size_t)s->n_intervals;
    return c->len ? CL_OK : CL_ERR_INVALID;
}
cl_status cl_contig_abort(cl_ctx *) { return CL_OK; }
cl_status cl_site_pileup(cl_ctx *, uint8_t, uint32_t, uint64_t, const cl_site_tile *, const uint32_t *, size_t, uint32_t *) { return CL_ERR_DEVICE; }
}

static unsigned long long checksum(const void *p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

// One round's reads as a caller hands them over, in arrays of exactly the sizes the interface names (the sanitizers see
// every byte the walk touches beyond them), with what a per-base walk makes of every read.
namespace {
struct Reads {
    std::vector<int32_t> pos; std::vector<uint8_t> mapq; std::vector<uint32_t> cigar_off{0u}, cigar;
    std::vector<uint64_t> qual_off{0ull}; std::vector<uint8_t> qual;
    std::vector<uint64_t> pass_bits; std::vector<uint32_t> pass_sum;      // the packed variant of the same (qual_pack)
    std::vector<uint32_t> end;                                            // pos + span, or pos beyond the 32-bit range
    std::vector<uint64_t> sum;                                            // the read's share of summed_baseq
    uint32_t err = 0;                                                     // kErrCigar / kErrRange, as the walk has to find them
    size_t n() const { return pos.size(); }
    void add(uint32_t p, uint8_t mq, const std::vector<uint32_t> &cig, const std::vector<uint8_t> &q, uint8_t thr, uint32_t min_mapq, std::vector<uint32_t> &want)
    {
        unsigned long long span = 0, x = p, y = 0;
        uint64_t sm = 0;
        for (uint32_t cw : cig) { const uint32_t op = cw & 15u, l = cw >> 4; if ((0x18Du >> op) & 1u) { span += l; if (!l) err |= clk::kErrCigar; } }
        if (span && cig.size() == 1 && !((0x181u >> (cig[0] & 15u)) & 1u)) err |= clk::kErrCigar;
        const bool in_range = span <= 0xFFFF0000ull - p;
        if (!in_range) err |= clk::kErrRange;
        const bool in_rows = in_range && span && mq >= min_mapq && !q.empty();
        for (uint32_t cw : cig) {                                         // what the column walk counts
            const uint32_t op = cw & 15u, l = cw >> 4;
            if (in_rows && ((0x181u >> op) & 1u))
                for (uint32_t k = 0; k < l && y + k < q.size(); ++k)
                    if (q[(size_t)(y + k)] >= thr) { sm += q[(size_t)(y + k)]; if (x + k < want.size()) want[(size_t)(x + k)] += 1; }
            if ((0x18Du >> op) & 1u) x += l;
            if ((0x193u >> op) & 1u) y += l;
        }
        pos.push_back((int32_t)p); mapq.push_back(mq); end.push_back(in_range ? p + (uint32_t)span : p); sum.push_back(sm);
        cigar.insert(cigar.end(), cig.begin(), cig.end()); cigar_off.push_back((uint32_t)cigar.size());
        qual.insert(qual.end(), q.begin(), q.end()); qual_off.push_back(qual.size());
    }
    // reads [a, b) as a tile: the offset arrays start at read a, the CIGAR and quality arrays are the contig's
    Offence push(Staging &hs, PushRecord &acc, const WalkOpts &wo, size_t a, size_t b, bool packed) const
    {
        cl_read_tile t;
        t.n_reads = b - a; t.pos = pos.data() + a; t.mapq = mapq.data() + a; t.cigar_off = cigar_off.data() + a; t.cigar = cigar.data();
        t.qual_off = qual_off.data() + a; t.qual = packed ? nullptr : qual.data();
        TileHead h;
        const Offence f = tile_header(hs.pos.size(), t.n_reads, t.pos, t.mapq, t.cigar_off, t.cigar, t.qual_off, h);
        if (f.st != CL_OK || h.n == 0) return f;
        return packed ? push_reads_bits(hs, acc, wo, &t, h, pass_bits.data(), pass_sum.data() + a) : push_reads_bits(hs, acc, wo, &t, h);
    }
};

// every staged array's size and the checksum of its [0, size) bytes, and every field of the push record
std::vector<unsigned long long> snapshot(const Staging &hs, const PushRecord &a)
{
    std::vector<unsigned long long> v;
    auto arr = [&](const auto &x) { v.push_back(x.size()); v.push_back(checksum(x.data(), x.size() * sizeof(*x.data()))); };
    arr(hs.ref); arr(hs.mapq); arr(hs.pos); arr(hs.cigar_off); arr(hs.cigar); arr(hs.qual_off); arr(hs.end); arr(hs.ck_x); arr(hs.ck_y);
    arr(hs.rec_cnt); arr(hs.rec_of); arr(hs.qbits); arr(hs.rb_off); arr(hs.qual); arr(hs.wide_idx); arr(hs.wide_pos); arr(hs.wide_rec_of);
    arr(hs.sc_off); arr(hs.sc);
    for (unsigned long long f : {(unsigned long long)a.host_max_end, (unsigned long long)a.host_sum_q, (unsigned long long)a.host_sum_cov,
                                 (unsigned long long)a.host_sum_mapq, (unsigned long long)a.host_n_ops, (unsigned long long)a.host_err,
                                 (unsigned long long)a.span_n, (unsigned long long)a.span_w, (unsigned long long)a.n_long,
                                 (unsigned long long)a.has_long, (unsigned long long)a.rec_counted, (unsigned long long)a.q_dev})
        v.push_back(f);
    return v;
}
} // namespace

// The host half of the pass-bit form on random reads, through the walk the library runs (tile_walk.h: push_reads_bits into
// a staged contig, in several tiles, as bytes and packed) and the row builder (pass_rows.h): the column sums of four
// windows must be what a per-base walk counts, the accumulated sums what the reads add up to, and a refused tile --
// one in every round, between accepted ones -- must leave the staged contig and the push record as they were.
constexpr int kRounds = 60, kRefusals = kRounds;
static int pass_bit_selftest()
{
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    constexpr uint32_t T = 2048, kContigLen = 50'000'000u, kMinMapq = 10;
    int bad = 0, tw_bad = 0, refusals = 0;
    for (int round = 0; round < kRounds; ++round) {
        auto miss = [&](const char *what) { ++tw_bad; fprintf(stderr, "tile walk selftest, round %d: %s\n", round, what); };
        const uint8_t thr = (uint8_t)(round % 3 == 0 ? 0 : (round % 3 == 1 ? 20 : 200));
        const bool packed = round % 2 == 1, single = round % 6 >= 4;      // (single: one read per tile)
        const int special = round % 15;                                    // 11 a wide read, 12 a span beyond 32 bits, 13 a zero-length D, 14 a lone non-match
        WalkOpts wo;
        wo.contig_len = kContigLen; wo.min_mapq = kMinMapq; wo.min_bq = thr;
        if (round % 10 == 7) wo.head_span = 37;                            // (a DUT_HEAD_SPAN of the Python tests: spans cut into several heads)
        const uint32_t n = 300 + (uint32_t)rnd(150);
        Reads R;
        std::vector<uint32_t> want(4 * T, 0);                  // qc_depth of positions [0, 4 T)
        uint32_t p = 0;
        for (uint32_t i = 0; i < n; ++i) {
            p += (uint32_t)rnd(36);
            std::vector<uint32_t> cig;
            const int kind = (int)rnd(5);
            unsigned long long qlen = 0;
            bool no_qual = false;
            if (i == n / 2 && special == 11) cig.push_back(20000u << 4);
            else if (i == n / 2 && special == 12) { cig.push_back(10u << 4); for (int j = 0; j < 17; ++j) cig.push_back((0xFFFFFFFu << 4) | 3u); cig.push_back(10u << 4); }
            else if (i == n / 2 && special == 13) { cig.push_back(30u << 4); cig.push_back((0u << 4) | 2u); cig.push_back(25u << 4); }
            else if (i == n / 2 && special == 14) { cig.push_back((50u << 4) | 2u); no_qual = true; }   // (without a quality string: in no row)
            else if (kind == 0) { const uint32_t l = 1 + (uint32_t)rnd(300); cig.push_back(l << 4); }
            else {
                if (rnd(3) == 0) cig.push_back(((uint32_t)(1 + rnd(9)) << 4) | 4u);        // S
                const int nops = 1 + (int)rnd(kind == 4 ? 150 : 12);
                for (int j = 0; j < nops; ++j) {
                    cig.push_back(((uint32_t)(1 + rnd(kind == 3 ? 70 : 20)) << 4) | (uint32_t)(rnd(4) == 0 ? 7u : 0u));   // M or =
                    const uint32_t o = (uint32_t)rnd(kind == 2 ? 6 : 4);
                    if (o == 0) cig.push_back(((uint32_t)(1 + rnd(3)) << 4) | 1u);           // I
                    else if (o == 1) cig.push_back(((uint32_t)(1 + rnd(5)) << 4) | 2u);      // D
                    else if (o >= 4) cig.push_back(((uint32_t)(1500 + rnd(3000)) << 4) | 3u); // N: a gapped (sparse) read
                }
                cig.push_back(((uint32_t)(1 + rnd(30)) << 4) | 0u);
            }
            for (uint32_t cw : cig) { const uint32_t op = cw & 15u, l = cw >> 4; if ((0x193u >> op) & 1u) qlen += l; }
            unsigned long long ql = rnd(7) == 0 ? qlen / 2 : qlen;                             // sometimes a truncated quality string
            if (rnd(23) == 0 || no_qual) ql = 0;
            std::vector<uint8_t> q((size_t)ql);
            for (auto &b : q) b = (uint8_t)(rnd(4) == 0 ? rnd(256) : 30 + rnd(12));
            R.add(p, (uint8_t)(rnd(6) == 0 ? 3 : 60), cig, q, thr, kMinMapq, want);
        }
        {   // the packed variant as a caller builds it: the bits of the whole quality array (every level of qual_pack), the reads' sums
            R.pass_bits.assign((R.qual.size() + 63) / 64 + (R.qual.empty() ? 1 : 0), 0ull);
            const uint64_t all = dut::qual_pass_read(R.qual.data(), R.qual.size(), thr, R.pass_bits.data(), round % 3);
            uint64_t naive = 0;
            for (uint8_t b : R.qual) naive += b >= thr ? b : 0u;
            if (all != naive) miss("qual_pass_read's sum");
            for (size_t i = 0; i < n; ++i) R.pass_sum.push_back((uint32_t)R.sum[i]);
        }
        // ---- the contig, staged as cl_contig_begin .. cl_push_reads do ----
        Staging hs;
        PushRecord acc;
        take_staging(hs);
        hs.clear(); hs.cigar_off.push_back(0u); hs.qual_off.push_back(0ull);
        // the tiles: cut inside a 64-bit word of the bit array and inside a chunk of 64 reads; the one behind the first cut
        // is first offered with an offence (three chunks or more: the offence lies in the first, a middle or the last)
        auto cut_at = [&](size_t c) { while (c % 64 == 0 || R.qual_off[c] % 64 == 0 || (n - c) % 64 < 2) ++c; return c; };
        const size_t c1 = cut_at(70 + (size_t)rnd(40)), c2 = cut_at(c1 + 130 + (size_t)rnd(30));
        auto refused_tile = [&]() {
            const size_t m = n - c1, nchunk = (m + 63) / 64;
            const int what = round % 4, where = (round / 4) % 3;          // unsorted, outside the contig, offsets that decrease, offsets that leave the tile
            size_t j = where == 0 ? (what == 0 ? 0 : 3) : (where == 1 ? 64 * (nchunk / 2) + 7 : 64 * (nchunk - 1));
            Reads B = R;
            Offence expect{CL_ERR_INVALID, "offset arrays must be non-decreasing"};
            if (what == 0) { B.pos[c1 + j] = B.pos[c1 + j - 1] - 1; expect = {CL_ERR_UNSORTED, "reads are not coordinate sorted"}; }
            else if (what == 1) {
                B.pos[c1 + j] = round % 8 < 4 ? (int32_t)kContigLen : -1;
                expect = {CL_ERR_INVALID, "read position outside [0, contig_len): the region fetch (mod.rs:53) never yields it"};
            }
            else if (what == 2) { if (round % 8 < 4) B.cigar_off[c1 + j + 1] = B.cigar_off[c1 + j] - 1; else B.qual_off[c1 + j + 1] = B.qual_off[c1 + j] - 1; }
            else { if (round % 8 < 4) B.qual_off[c1 + j + 1] = B.qual_off[n] + 5; else B.cigar_off[c1 + j + 1] = B.cigar_off[n] + 3; }
            const std::vector<unsigned long long> before = snapshot(hs, acc);
            const Offence f = B.push(hs, acc, wo, c1, n, packed);
            if (f.st != expect.st || !f.msg || strcmp(f.msg, expect.msg) != 0) miss("a refusal's status or message");
            if (snapshot(hs, acc) != before) miss("a refused tile changed the staged contig or the push record");
            ++refusals;
        };
        auto accept = [&](size_t a, size_t b) {
            const uint64_t sum0 = acc.host_sum_q;
            if (R.push(hs, acc, wo, a, b, packed).st != CL_OK) miss("a good tile was refused");
            uint64_t add = 0;
            for (size_t i = a; i < b; ++i) add += R.sum[i];
            if (acc.host_sum_q - sum0 != add) miss("the tile's share of summed_baseq");   // (single: that one read's naive sum)
        };
        if (single) { for (size_t i = 0; i < n; ++i) { if (i == c1) refused_tile(); accept(i, i + 1); } }
        else { accept(0, c1); refused_tile(); accept(c1, c2); accept(c2, n); }
        // ---- what the walk left, against the per-base walk ----
        uint64_t sum_cov = 0, sum_mapq = 0, max_end = 0;
        uint32_t span_n = 0, span_w = 0;
        std::vector<uint32_t> wide;
        if (hs.pos.size() != n || hs.end.size() != n || hs.rec_cnt.size() != n || hs.rb_off.size() != n + 1 || hs.sc_off.size() != n + 1) miss("the staged sizes");
        else for (size_t i = 0; i < n; ++i) {
            const uint64_t span = R.end[i] - (uint32_t)R.pos[i];
            unsigned long long l = 0;
            for (uint32_t k = R.cigar_off[i]; k < R.cigar_off[i + 1]; ++k) if ((0x18Du >> (R.cigar[k] & 15u)) & 1u) l += R.cigar[k] >> 4;
            if (hs.pos[i] != R.pos[i] || hs.mapq[i] != R.mapq[i] || hs.end[i] != R.end[i]) miss("a staged read");
            if (hs.rec_cnt[i] != (span + wo.head_span - 1) / wo.head_span) miss("a read's head count");
            sum_cov += span; if (R.mapq[i] >= kMinMapq) sum_mapq += R.mapq[i] * span;
            if (l <= 0xFFFF0000ull - (uint64_t)R.pos[i]) max_end = std::max<uint64_t>(max_end, (uint64_t)R.pos[i] + l);
            const uint32_t sp = l > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l;
            if (sp > clk::kWideSpan) { wide.push_back((uint32_t)i); span_w = std::max(span_w, sp); } else span_n = std::max(span_n, sp);
        }
        if (acc.host_sum_cov != sum_cov || acc.host_sum_mapq != sum_mapq || acc.host_n_ops != R.cigar.size() || acc.q_dev != R.qual.size() ||
            acc.host_max_end != max_end || acc.span_n != span_n || acc.span_w != span_w || acc.host_err != R.err || hs.wide_idx != wide)
            miss("the push record");
        if ((special == 11 && std::find(wide.begin(), wide.end(), n / 2) == wide.end()) || (special == 12 && !(R.err & clk::kErrRange)) || (special >= 13 && !(R.err & clk::kErrCigar)))
            miss("the round's special read is not what it should be");
        dut::RowReads H;
        H.pos = hs.pos.data(); H.end = hs.end.data(); H.mapq = hs.mapq.data(); H.off = hs.rb_off.data(); H.bits = hs.qbits.data();
        H.sc_off = hs.sc_off.data(); H.sc = hs.sc.data(); H.min_mapq = kMinMapq;
        std::vector<dut::RowCur> act;
        dut::RowScratch scr;
        uint32_t next = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t W = w * T;
            while (next < n && (uint32_t)hs.pos[next] < W + T) { dut::rows_enter(act, H, next, W); ++next; }
            size_t cap = 2, ng;
            std::vector<dut::RowCur> start = act;
            std::vector<uint32_t> buf;
            for (;;) { buf.assign(cap * dut::kRowGroupWords, 0xFFFFFFFFu); act = start; ng = dut::rows_window<T>(act, H, W, buf.data(), cap, scr); if (ng != SIZE_MAX) break; cap *= 2; }
            for (uint32_t x = 0; x < T; ++x) {
                uint32_t cnt = 0;
                for (size_t r = 0; r < 4 * ng; ++r) cnt += (buf[(r >> 2) * dut::kRowGroupWords + ((x >> 5) << 2) + (r & 3)] >> (x & 31u)) & 1u;
                if (cnt != want[W + x]) ++bad;
            }
        }
        give_staging(hs);
    }
    if (refusals != kRefusals) { ++tw_bad; fprintf(stderr, "tile walk selftest: %d refusal(s) instead of %d\n", refusals, kRefusals); }
    // the reference's "is N" bits, with buffers of exactly the sizes the interface names
    for (int round = 0; round < 40; ++round) {
        const size_t nb = (size_t)rnd(700), nw = (size_t)rnd(14);
        std::vector<uint8_t> ref(nb);
        for (auto &b : ref) b = (uint8_t)"ACGTNnacgtRY"[rnd(12)];
        std::vector<uint64_t> out(nw);
        dut::ref_n_words(ref.data(), nb, nw, out.data(), round % 3);
        for (size_t p = 0; p < 64 * nw; ++p) {
            const bool want = p >= nb || (ref[p] | 0x20) == 'n';
            if ((((out[p >> 6] >> (p & 63)) & 1ull) != 0) != want) ++bad;
        }
    }
    printf("pass-bit selftest: %d mismatch(es)\n", bad);
    printf("tile walk selftest: %d mismatch(es), %d refusal(s)\n", tw_bad, kRefusals);
    return bad + tw_bad;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: sanitize_host <bam> [tree.json]\n"); return 2; }
    if (pass_bit_selftest() != 0) return 5;
    char err[512] = {0};
    // BAM reader: every contig, with and without sequences, twice (buffer reuse), in reverse order too
    dut_bam *b = dut_bam_open(argv[1], err, sizeof(err));
    if (!b) { printf("open failed: %s\n", err); return 0; }           // corrupted inputs are allowed to fail cleanly
    const int n_ref = dut_bam_n_ref(b);
    cl_options opt = {4, 500, 10, 20, 10, 1, 0.1};
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < n_ref; ++k) {
            const int tid = pass ? n_ref - 1 - k : k;
            dut_records rec{}; const uint64_t *so = nullptr; const uint8_t *sq = nullptr;
            const int rc = dut_bam_read_contig(b, tid, &rec, pass ? &so : nullptr, pass ? &sq : nullptr);
            if (rc != CL_OK) { printf("tid %d: %s\n", tid, dut_bam_error(b)); continue; }
            unsigned long long h = checksum(rec.pos, rec.n * 4) ^ checksum(rec.qual, rec.qual_off[rec.n]) ^ checksum(rec.cigar, 4ull * rec.cigar_off[rec.n]) ^
                                   checksum(rec.qname, rec.qname_off[rec.n]);
            if (pass) h ^= checksum(sq, (so[rec.n] + 1) / 2);
            {   // the packed variant of the same contig: its bits and sums against the bytes just read
                const std::vector<uint8_t> q(rec.qual, rec.qual + rec.qual_off[rec.n]);
                const std::vector<uint64_t> qo(rec.qual_off, rec.qual_off + rec.n + 1);
                dut_records pr{};
                const uint8_t thr = (uint8_t)(pass ? 20 : 0);
                if (dut_bam_read_contig_bits(b, tid, thr, &pr) == CL_OK && pr.n == qo.size() - 1) {
                    unsigned long long wrong = pr.qual != nullptr;
                    for (uint64_t g = 0; g < q.size(); ++g) wrong += (((pr.pass_bits[g >> 6] >> (g & 63)) & 1ull) != 0) != (q[(size_t)g] >= thr);
                    for (uint64_t i = 0; i < pr.n; ++i) {
                        uint64_t y = 0, want = 0;
                        const uint64_t ql = qo[i + 1] - qo[i];
                        for (uint32_t k = pr.cigar_off[i]; k < pr.cigar_off[i + 1]; ++k) {
                            const uint32_t op = pr.cigar[k] & 15u, l = pr.cigar[k] >> 4;
                            if ((0x181u >> op) & 1u) for (uint64_t j = y; j < y + l && j < ql; ++j) want += q[(size_t)(qo[i] + j)] >= thr ? q[(size_t)(qo[i] + j)] : 0u;
                            if ((0x193u >> op) & 1u) y += l;
                        }
                        wrong += want != pr.pass_sum[i];
                    }
                    if (wrong) { printf("tid %d: the packed reader disagrees in %llu place(s)\n", tid, wrong); return 6; }
                    // (rec's arrays are the reader's own and are gone now: read again for what follows)
                    if (dut_bam_read_contig(b, tid, &rec, pass ? &so : nullptr, pass ? &sq : nullptr) != CL_OK) continue;
                }
            }
            std::vector<uint8_t> acc(rec.n + 1);
            uint32_t names = 0; uint64_t nacc = 0;
            const int ar = dut_admit_reads(&opt, tid, dut_bam_ref_len(b, tid), &rec, acc.data(), &names, &nacc);
            printf("tid %d pass %d: n %llu hash %016llx admit rc %d accepted %llu names %u\n", tid, pass, (unsigned long long)rec.n, h, ar,
                   (unsigned long long)nacc, names);
        }
    }
    dut_bam_close(b);
    dut_bam_stats *bs = dut_bam_stats_new(10000);
    if (dut_bam_stats_collect(bs, argv[1], err, sizeof(err)) == CL_OK)
        printf("stats: %s | %s | %s | %llu\n", dut_bam_stats_aligner(bs), dut_bam_stats_reference_build(bs), dut_bam_stats_infer_platform(bs),
               (unsigned long long)dut_bam_stats_average_read_length(bs));
    dut_bam_stats_free(bs);
    if (argc > 2) {
        dut_tree *t = dut_tree_load(argv[2], DUT_PROVIDER_FTDNA, DUT_TREE_YDNA, err, sizeof(err));
        if (!t) { printf("tree failed: %s\n", err); return 0; }
        uint32_t *sites = nullptr; uint8_t *rel = nullptr; size_t ns = 0;
        dut_tree_collect_sites(t, "GRCh38", "chrY", &sites, &rel, &ns);
        std::vector<uint32_t> hist(16 * (ns + 1), 0);
        static const int kCode[4] = {1, 2, 4, 8};                         // A C G T
        for (size_t i = 0; i < ns; ++i) { hist[16 * i + kCode[i % 4]] = 12 + (uint32_t)(i % 9); hist[16 * i + 15] += (uint32_t)(i % 3); }
        dut_snp_call *calls = nullptr; size_t nc = 0;
        dut_call_sites(sites, rel, hist.data(), ns, 10, &calls, &nc);
        dut_haplogroup_result *res = nullptr; size_t nr = 0;
        const int rc = dut_tree_score(t, calls, nc, "GRCh38", &res, &nr, err, sizeof(err));
        printf("tree: %zu nodes, %zu sites, %zu calls, score rc %d, %zu rows\n", dut_tree_built_nodes(t), ns, nc, rc, nr);
        if (rc == CL_OK) {
            const std::string out = std::string(argv[2]) + ".tsv";
            dut_write_haplogroup_report(out.c_str(), t, res, nr, calls, nc, "GRCh38", 1, err, sizeof(err));
        }
        dut_free(res); dut_free(calls); dut_free(sites); dut_free(rel);
        dut_tree_free(t);
    }
    // an allocation failure inside a parallel loop or on a helper thread must come back to the caller as an
    // exception on ITS thread (the C ABI wrappers turn it into a status), never end a worker (std::terminate)
    {
        std::atomic<size_t> done{0};
        bool caught = false;
        try {
            dut::parallel_for(20000, 7, [&](size_t i) { if (i == 4177) throw std::bad_alloc(); done.fetch_add(1); });
        } catch (const std::bad_alloc &) { caught = true; }
        int ran = 0;
        { dut::Thread t = dut::spawn_or_run([&]() { ran = 1; throw std::bad_alloc(); }); }
        printf("parallel_for: exception %s, helper ran %d, not every index ran %d\n", caught ? "caught" : "LOST", ran, done.load() < 20000 ? 1 : 0);
        if (!caught) return 3;
    }
    // the persistent workers: loops started from several threads at once, and from inside a chunk of another loop,
    // share them and each comes back complete (the caller always works on its own loop)
    {
        std::atomic<uint64_t> total{0};
        auto burst = [&](uint64_t salt) {
            for (int rep = 0; rep < 40; ++rep) {
                std::atomic<uint64_t> sum{0};
                const size_t n = 300 + 97 * (size_t)rep;
                dut::parallel_for(n, 3, [&](size_t i) {
                    if (i % 64 == 0) {                         // a loop inside a chunk
                        std::atomic<uint64_t> inner{0};
                        dut::parallel_for(50, 4, [&](size_t j) { inner.fetch_add(j + 1); });
                        if (inner.load() != 50 * 51 / 2) abort();
                    }
                    sum.fetch_add(i + salt);
                });
                if (sum.load() != n * (n - 1) / 2 + salt * n) abort();
                total.fetch_add(sum.load());
            }
        };
        {
            dut::Thread a = dut::spawn_or_run([&]() { burst(1); });
            dut::Thread b = dut::spawn_or_run([&]() { burst(2); });
            burst(3);
        }
        printf("worker pool: three callers, nested loops, total %llu\n", (unsigned long long)total.load());
    }
    // the crew of the pinned ring (host_parallel.h: started once, asleep between jobs) and the pool of large temporaries:
    // jobs of changing width back to back, each index exactly once; blocks taken and given back from several threads
    {
        dut::Crew crew;
        crew.ensure(3);
        unsigned long long ran = 0;
        for (int rep = 0; rep < 200; ++rep) {
            const int n = 1 + (rep * 7) % 9;
            std::vector<std::atomic<int>> hit(9);
            for (auto &h : hit) h.store(0);
            crew.start(n, [&](int t) { hit[(size_t)t].fetch_add(1); });
            crew.wait();
            for (int t = 0; t < 9; ++t) { if (hit[(size_t)t].load() != (t < n ? 1 : 0)) { printf("crew: job %d ran index %d %d time(s)\n", rep, t, hit[(size_t)t].load()); return 7; } ran += (unsigned long long)hit[(size_t)t].load(); }
        }
        std::atomic<unsigned long long> bytes{0};
        dut::parallel_for(64, 1, [&](size_t i) {
            dut::Scratch<uint64_t> a((1u << 17) + 1000 * i), b(100 + i);          // one pooled (>= 1 MB), one not
            a.get()[0] = i; a.get()[(1u << 17) + 1000 * i - 1] = i; b.get()[99 + i] = i;
            bytes.fetch_add(a.get()[0] + b.get()[99 + i]);
            dut::Scratch<uint64_t> c(std::move(a));
            if (a || !c) abort();
        });
        // (how many blocks the pool holds now depends on how the threads interleaved: not printed)
        printf("crew: %llu calls over 200 jobs; scratch pool: checksum %llu, %s\n", ran, bytes.load(), dut::scratch_pool().idle.size() <= dut::ScratchPool::kScratchKeep ? "within its limit" : "OVER ITS LIMIT");
    }
    // summary JSON with awkward names
    dut_contig_stats st[2]; memset(st, 0, sizeof(st));
    st[0].length = 20; st[0].n_covered_bases = 12; st[0].summed_coverage = 22; st[0].summed_baseq = 420; st[0].summed_mapq = 960; st[0].quality_bases = 14; st[0].n_reads = 3;
    st[1].length = 0;
    const char *names[2] = {"chr\"T\\\x01", "chrUn_x"};
    uint64_t counts[12] = {2, 2, 8, 6, 0, 2, 0, 0, 0, 0, 0, 0};
    dut_export_meta meta; memset(&meta, 0, sizeof(meta));
    meta.aligner = "BWA"; meta.reference_build = "GRCh38"; meta.sequencing_platform = "NovaSeq"; meta.read_length = 150;
    meta.bed_file = "x.bed"; meta.summary_html = "s.html";
    char *js = nullptr; size_t jl = 0;
    if (dut_coverage_output_json(st, names, counts, 2, &meta, &js, &jl) == CL_OK) printf("json %zu bytes\n", jl);
    dut_free(js);
    // BED writer with the coverage figures + the HTML report (host only), into the tree file's directory
    if (argc > 2) {
        const std::string dir = std::string(argv[2]).substr(0, std::string(argv[2]).find_last_of('/'));
        dut_profiler *pr = dut_profiler_new((dir + "/san.bed").c_str());
        if (pr) {
            dut_profiler_enable_plots(pr, 5000);
            const cl_interval iv1[4] = {{0, 3, CL_REF_N}, {3, 900, CL_CALLABLE}, {900, 2100, CL_POOR_MAPPING_QUALITY}, {2100, 5000, CL_CALLABLE}};
            const uint64_t c1[6] = {3, 3797, 0, 0, 0, 1200};
            dut_profiler_feed_contig(pr, names[0], iv1, 4, c1);
            dut_profiler_finish_plot(pr, names[0], 5000);
            dut_profiler_feed_contig(pr, "chrM", nullptr, 0, c1);            // inherits the previous contig's last line
            size_t nb = 0; uint32_t stride = 0;
            std::vector<uint32_t> a(512), b(512), c(512);
            dut_profiler_plot_bins(pr, "chrM", 16569, &stride, a.data(), b.data(), c.data(), 512, &nb);
            printf("plot: %d figure(s), %zu bins of %u\n", dut_profiler_finish_plot(pr, "chrM", 16569), nb, stride);
            dut_profiler_free(pr);
        }
        printf("html rc %d\n", dut_write_html_report(st, names, counts, 2, &meta, 10000, (dir + "/san.html").c_str()));
    }
    // the orchestration of the several-device call (threads, reader pairs, results handed to the BED writer in tid
    // order) over the stand-in engine above: the BED of 1, 2 and 3 "devices" must be the same text
    if (argc > 3) {
        const std::string dir = std::string(argv[3]).substr(0, std::string(argv[3]).find_last_of('/'));
        unsigned long long first = 0;
        for (int nd = 1; nd <= 3; ++nd) {
            const int devs[3] = {0, 1, 1};
            const std::string bed = dir + "/multi" + std::to_string(nd) + ".bed";
            char e2[512] = {0};
            const int rc = dut_coverage_files_multi(argv[1], argv[3], bed.c_str(), nullptr, nullptr, &opt, nullptr, 0, devs, (size_t)nd, 0u, e2, sizeof(e2));
            std::string text;
            if (FILE *f = fopen(bed.c_str(), "rb")) { char buf[4096]; size_t g; while ((g = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, g); fclose(f); }
            const unsigned long long h = checksum(text.data(), text.size());
            if (nd == 1) first = h;
            printf("multi %d device(s): rc %d%s%s, bed %zu bytes %s\n", nd, rc, rc ? " " : "", rc ? e2 : "", text.size(), h == first ? "same" : "DIFFERENT");
            if (rc == CL_OK && h != first) return 4;
        }
        const int bad[2] = {0, 99};
        char e3[512] = {0};
        printf("multi, a device that does not exist: rc %d\n", dut_coverage_files_multi(argv[1], argv[3], (dir + "/multi_bad.bed").c_str(), nullptr, nullptr, &opt, nullptr, 0, bad, 2, 0u, e3, sizeof(e3)));
    }
    return 0;
}
