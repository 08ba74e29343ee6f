// tile_walk.h -- the host walk over a tile of reads (cl_push_reads, cl_push_reads_bits), plain C++ without HIP, so that
// a stand-alone CPU program can run it under the sanitizers (tests/native/sanitize_host.cpp): the staged contig, the
// record of what a push accumulates, the checks of a tile and of each read, the first pass over a tile's CIGARs written
// once for both forms, and the whole walk of the pass-bit form.
//
// How a tile is taken back: everything a tile adds to the staged arrays is written BEYOND their sizes, into capacity
// reserved first, and the sizes and the push record follow in one step that cannot fail, when the tile is accepted.  A
// refused tile leaves nothing but unused capacity behind.
#pragma once
#include "../../include/callable_loci.h"
#include "engine_limits.h"
#include "host_stage.h"
#include "pass_rows.h"
#include "qual_pack.h"

#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

// The host staging arrays of a contig (hundreds of megabytes) are only needed between cl_contig_begin and
// cl_contig_upload.  A context hands them to this process-wide pool when its contig is uploaded and takes a set back
// at its next cl_contig_begin -- so does a fresh context: memory that has been touched before is written at several
// times the rate of newly mapped pages (staging a chr21-sized contig: 5 ms against 31 ms), and callers that keep one
// context per resident contig would otherwise fault a new set in for every contig.  At most kStagingSets sets are kept.
struct StagingSet {
    RawVec<uint8_t> ref, mapq;
    RawVec<int32_t> pos;
    RawVec<uint32_t> cigar_off, cigar;
    RawVec<unsigned long long> qual_off;
    // the index over the CIGARs, built by the one host walk that validates a tile (cl_push_reads): every read's end,
    // and for reads with more than kLongOps operations the (reference, query) position before every 64th operation
    // of the contig's CIGAR array
    RawVec<uint32_t> end, ck_x, ck_y;
    // per read, from the same walk: how many records the record forms get for it (gen_read_recs); their prefix sums
    // are taken at upload: read i's records are rec[rec_of[i] .. rec_of[i + 1])
    RawVec<uint32_t> rec_cnt, rec_of;
    // pass-bit form (the default): bit g = quality byte g of the contig passes min_base_quality (mod.rs:33), taken in
    // cl_push_reads' walk
    RawVec<uint64_t> qbits;               // the reads' bit strings (reference order; pass_rows.h), word-aligned per read
    RawVec<unsigned long long> rb_off;    // n + 1 word offsets into qbits (| dut::kRowSparse)
};
// Everything a context stages of its contig between cl_contig_begin and cl_contig_upload: the pooled arrays and the few
// that are too small to pool.  A new array is added to clear() -- and to swap_pooled() if it is pooled --, nowhere else.
struct Staging : StagingSet {
    std::vector<uint8_t> qual;            // quality bytes of small tiles, not yet on the device (byte forms)
    // reads whose reference span exceeds kWideSpan (ascending read index = ascending position)
    std::vector<uint32_t> wide_idx;
    std::vector<int32_t> wide_pos;
    std::vector<uint32_t> wide_rec_of;    // prefix sums of the wide reads' record counts (n_wide + 1 entries; built at upload)
    RawVec<uint32_t> sc_off, sc;          // pass-bit form: the CIGARs of the sparse reads (n + 1 offsets)
    void swap_pooled(StagingSet &o)
    {
        ref.swap(o.ref); mapq.swap(o.mapq); pos.swap(o.pos); cigar_off.swap(o.cigar_off); cigar.swap(o.cigar); qual_off.swap(o.qual_off);
        end.swap(o.end); ck_x.swap(o.ck_x); ck_y.swap(o.ck_y); rec_cnt.swap(o.rec_cnt); rec_of.swap(o.rec_of); qbits.swap(o.qbits); rb_off.swap(o.rb_off);
    }
    void clear()                          // (sizes only, the memory stays; but qual gives its memory back: only contigs of small tiles fill it)
    {
        ref.clear(); mapq.clear(); pos.clear(); cigar_off.clear(); cigar.clear(); qual_off.clear();
        end.clear(); ck_x.clear(); ck_y.clear(); rec_cnt.clear(); rec_of.clear(); qbits.clear(); rb_off.clear();
        std::vector<uint8_t>().swap(qual); wide_idx.clear(); wide_pos.clear(); wide_rec_of.clear(); sc_off.clear(); sc.clear();
    }
};
constexpr size_t kStagingSets = 2;
inline std::mutex g_staging_mu;
inline std::vector<std::unique_ptr<StagingSet>> g_staging;

// a context without staging memory of its own takes a pooled set (cl_contig_begin) ...
inline void take_staging(Staging &hs)
{
    if (hs.pos.cap || hs.cigar.cap || hs.qual_off.cap || hs.qbits.cap) return;
    std::unique_ptr<StagingSet> s;
    {
        std::lock_guard<std::mutex> g(g_staging_mu);
        if (g_staging.empty()) return;
        s = std::move(g_staging.back()); g_staging.pop_back();
    }
    hs.swap_pooled(*s);                                    // what the context had (nothing) is freed with s
}
// ... and gives its set back, empty, once the contig is on the device (cl_contig_upload); a full pool keeps the larger sets
inline void give_staging(Staging &hs)
{
    hs.clear();
    std::unique_ptr<StagingSet> s(new (std::nothrow) StagingSet());
    if (!s) return;
    hs.swap_pooled(*s);
    std::lock_guard<std::mutex> g(g_staging_mu);
    if (g_staging.size() < kStagingSets) { g_staging.push_back(std::move(s)); return; }
    size_t small = 0;
    for (size_t i = 1; i < g_staging.size(); ++i) if (g_staging[i]->cigar_off.cap < g_staging[small]->cigar_off.cap) small = i;
    if (g_staging[small]->cigar_off.cap < s->cigar_off.cap) g_staging[small].swap(s);      // s (the smaller one) is freed
}

// What the pushes of a contig have accumulated beside the staged arrays; PushRecord() is the state of a contig without a
// tile (cl_contig_begin, cl_contig_abort).  Only an accepted tile changes it.
struct PushRecord {
    uint64_t host_max_end = 0;       // largest pos + reference span over the pushed reads (32-bit clamped spans), for the extent
    // pass-bit form: the sum of the passing qualities over the M/=/X bases of the reads with mapq >= min_mapping_quality
    // (contig_profiler.rs:65-70: summed_baseq is per-read separable)
    uint64_t host_sum_q = 0;
    // ... and the reads' other separable sums (contig_profiler.rs:74, 79-82): reference spans of the reads
    // the pileup holds (-> summed_coverage) and mapq x span over those with mapq >= min_mapping_quality (-> summed_mapq)
    uint64_t host_sum_cov = 0, host_sum_mapq = 0;
    uint64_t host_n_ops = 0;         // CIGAR operations pushed (pass-bit form: none is staged; for cl_contig_layout)
    uint32_t host_err = 0;           // kErrCigar / kErrRange found by the walk (reported by cl_contig_collect)
    uint32_t span_n = 0, span_w = 0; // longest span among the ordinary / the wide reads
    uint32_t n_long = 0;             // reads with more than kLongOps operations
    bool has_long = false;           // ... there is one (its checkpoints are in hs.ck_x / hs.ck_y)
    bool rec_counted = true;         // false: a tile of long-read shape skipped the count (cl_contig_upload makes up for it if the contig gets the short-read form after all)
    uint64_t q_dev = 0;              // quality bytes of this contig that already are on the device (d_qual + kQualPad ..);
                                     // pass-bit form: the contig's quality values so far
};

// A refusal, as the status and the message the caller reports; {CL_OK, nullptr}: none.
struct Offence { cl_status st; const char *msg; };
constexpr Offence kNoOffence{CL_OK, nullptr};

// What cl_push_reads and cl_push_reads_bits check of a tile before they look at a read, over the arrays both tile structs
// have (n_staged: the contig's reads before this tile).  An empty tile is h.n == 0 without an offence.
struct TileHead { uint64_t n = 0, q0 = 0, ncig = 0, nq = 0; uint32_t cig0 = 0; };
inline Offence tile_header(size_t n_staged, uint64_t n, const int32_t *pos, const uint8_t *mapq, const uint32_t *cigar_off,
                           const uint32_t *cigar, const uint64_t *qual_off, TileHead &h)
{
    if (n == 0) return kNoOffence;
    if (!pos || !mapq || !cigar_off || !qual_off) return {CL_ERR_INVALID, "null tile array"};
    if (n_staged + n >= (1ull << 29)) return {CL_ERR_RANGE, "more than 2^29 reads in one contig"};
    h.cig0 = cigar_off[0]; h.q0 = qual_off[0];
    if (cigar_off[n] < h.cig0 || qual_off[n] < h.q0) return {CL_ERR_INVALID, "offset arrays must be non-decreasing"};
    h.ncig = (uint64_t)cigar_off[n] - h.cig0; h.nq = qual_off[n] - h.q0;
    if (h.ncig && !cigar) return {CL_ERR_INVALID, "null cigar array"};
    h.n = n;
    return kNoOffence;
}

// the first offence a tile's walk over its reads met (a chunk's `bad`, 1 .. 3), as the status and message of the refusal
inline Offence walk_offence(int bad)
{
    if (bad == 1) return {CL_ERR_INVALID, "read position outside [0, contig_len): the region fetch (mod.rs:53) never yields it"};
    if (bad == 2) return {CL_ERR_UNSORTED, "reads are not coordinate sorted"};
    return {CL_ERR_INVALID, "offset arrays must be non-decreasing"};
}
constexpr Offence kNoMemory{CL_ERR_NOMEM, "host staging allocation failed"};

// What the walk over a tile's reads keeps per chunk of reads; it reaches the push record only when the whole tile is
// accepted (walk_fold), so that a refused tile leaves the context as it was.
struct WalkChunk { int bad = 0; uint32_t err = 0, span_n = 0, span_w = 0; uint64_t max_end = 0; std::vector<uint32_t> wide; };
// read i before its CIGAR is looked at: position and order (offences 1, 2: the walk goes on), offsets (3: false, no walk)
inline bool walk_read_checks(WalkChunk &o, const cl_read_tile *t, size_t i, int32_t &last, uint32_t contig_len, const TileHead &h)
{
    const int32_t p = t->pos[i];
    if (p < 0 || (uint32_t)p >= contig_len) { if (!o.bad) o.bad = 1; }
    else if (p < last) { if (!o.bad) o.bad = 2; }
    last = p;
    const bool ok = t->cigar_off[i + 1] >= t->cigar_off[i] && t->qual_off[i + 1] >= t->qual_off[i] &&
                    t->cigar_off[i] >= h.cig0 && t->cigar_off[i + 1] <= h.cig0 + h.ncig && t->qual_off[i] >= h.q0 && t->qual_off[i + 1] <= h.q0 + h.nq;
    if (!ok && !o.bad) o.bad = 3;
    return ok;
}
// ... and once its CIGAR has given the reference length l: the end (beyond the engine's 32-bit coordinate range: flagged,
// the read then spans nothing), the longest ordinary span (it bounds every window's candidate range), the wide list
inline void walk_close_span(WalkChunk &o, size_t i, int32_t p, unsigned long long l, uint32_t &end)
{
    const uint32_t sp = l > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l;
    if (l <= 0xFFFF0000ull - (uint64_t)p) { end = (uint32_t)((uint64_t)p + l); o.max_end = std::max<uint64_t>(o.max_end, (uint64_t)p + l); }
    else o.err |= clk::kErrRange;
    if (sp > clk::kWideSpan) { o.wide.push_back((uint32_t)i); o.span_w = std::max(o.span_w, sp); }
    else o.span_n = std::max(o.span_n, sp);
}

// The first pass over a tile, the same for both forms: in chunks on all host threads (at most 65 536 reads; long reads --
// few records, thousands of operations each -- get smaller ones so that every thread has some), per read the checks that
// protect the later walks' indexing, the reference length of its CIGAR with the shapes htslib's resolve_cigar2 asserts on
// (a zero-length reference-consuming operation, a lone non-match operation that reaches a column), and its end into
// h_end[i] (pos + bam_cigar2rlen, the pileup node span).  What only one form does is its `form`:
//   form.blank(i)                          the form's entries of read i, before any check (a read that fails one keeps them)
//   form.ref_length(o, i, p, cig, nops, l) true: the form has walked this read's CIGAR itself and left its length in l
//   form.read(o, i, p, cig, nops, end)     the read is closed: what the form counts of it
// last0: the position of the contig's last read before this tile (0: none).  Nothing but h_end and what the form writes
// is touched; the chunks come back in tile order.
inline size_t walk_grain(size_t n) { return dut::grain_for(n, 65536); }
template <class Chunk, class Form>
inline std::vector<Chunk> walk_tile(const cl_read_tile *t, const TileHead &h, int32_t last0, uint32_t contig_len, uint32_t *h_end, const Form &form)
{
    const size_t n = h.n, grain = walk_grain(n), nchunk = (n + grain - 1) / grain;
    std::vector<Chunk> ch(nchunk);
    dut::parallel_for(nchunk, 1, [&](size_t k) {
        Chunk o;                                                // (on the walker's stack: neighbouring chunks of ch share cache lines)
        const size_t a = k * grain, b = std::min<size_t>(n, a + grain);
        int32_t last = a ? t->pos[a - 1] : last0;
        for (size_t i = a; i < b; ++i) {
            const int32_t p = t->pos[i];
            h_end[i] = (uint32_t)p; form.blank(i);
            if (!walk_read_checks(o, t, i, last, contig_len, h)) continue;
            const uint32_t q0i = t->cigar_off[i], nops = t->cigar_off[i + 1] - q0i;
            const uint32_t *cig = t->cigar + q0i;
            unsigned long long l = 0;
            if (!form.ref_length(o, i, p, cig, nops, l)) {
                uint32_t zero_len = 0;
                for (uint32_t q = 0; q < nops; ++q) {
                    const uint32_t cw = cig[q], len = cw >> 4;
                    const uint32_t radv = (0x18Du >> (cw & 15u)) & 1u;              // M D N = X consume the reference
                    l += len & (0u - radv);
                    zero_len |= radv & (len == 0u ? 1u : 0u);                      // zero-length reference-consuming op
                }
                if (zero_len) o.err |= clk::kErrCigar;
                // a read that reaches a column with a single non-match op is undefined in htslib
                if (l > 0 && nops == 1u && !(((0x181u >> (cig[0] & 15u)) & 1u) != 0u)) o.err |= clk::kErrCigar;
            }
            walk_close_span(o, i, p, l, h_end[i]);
            form.read(o, i, p, cig, nops, h_end[i]);
        }
        ch[k] = std::move(o);
    });
    return ch;
}
// the first offence in tile order decides the message
template <class Chunk> inline Offence first_offence(const std::vector<Chunk> &ch)
{
    for (const Chunk &o : ch) if (o.bad) return walk_offence(o.bad);
    return kNoOffence;
}
template <class Chunk> inline size_t wide_reads(const std::vector<Chunk> &ch)
{
    size_t n = 0;
    for (const Chunk &o : ch) n += o.wide.size();
    return n;
}
// the chunks of an accepted tile into the push record and the wide lists, whose capacity is there (rbase: the contig's
// reads before this tile); o.fold(acc) is what the form's chunk has beside WalkChunk
template <class Chunk> inline void walk_fold(Staging &hs, PushRecord &acc, const std::vector<Chunk> &ch, uint64_t rbase, const int32_t *pos)
{
    for (const Chunk &o : ch) {
        acc.host_err |= o.err;
        acc.span_n = std::max(acc.span_n, o.span_n); acc.span_w = std::max(acc.span_w, o.span_w);
        acc.host_max_end = std::max(acc.host_max_end, o.max_end);
        for (uint32_t i : o.wide) { hs.wide_idx.push_back((uint32_t)(rbase + i)); hs.wide_pos.push_back(pos[i]); }
        o.fold(acc);
    }
}

// n bits of `src` from bit offset sb into dst[0, ceil(n / 64)): whole words, zeros above bit n
inline void copy_bits_to_words(uint64_t *dst, const uint64_t *src, unsigned long long sb, unsigned long long n)
{
    const unsigned long long w0 = sb >> 6;
    const uint32_t s = (uint32_t)(sb & 63ull);
    const unsigned long long nw = (n + 63) >> 6;
    for (unsigned long long w = 0; w < nw; ++w) {
        const unsigned long long left = n - (w << 6);                    // bits still wanted from here on (>= 1)
        const uint32_t want = left >= 64ull ? 64u : (uint32_t)left;
        uint64_t v = src[w0 + w] >> s;
        if (s + want > 64u) v |= src[w0 + w + 1] << (64u - s);
        if (want < 64u) v &= (1ull << want) - 1ull;
        dst[w] = v;
    }
}

// what the pass-bit walk needs of a context's options
struct WalkOpts { uint32_t contig_len = 0, min_mapq = 0; uint8_t min_bq = 0; uint32_t head_span = clk::kHeadSpanMax; };

// what the pass-bit form does with a read in the first pass: its heads, its shares of the separable sums, and how many
// words of bits it will leave (rb_off[i], | kRowSparse with its operation count in sc_off[i])
struct BitsChunk : WalkChunk {
    uint64_t sum_q = 0, n_ops = 0, n_words = 0, n_sc = 0, sum_cov = 0, sum_mapq = 0;
    void fold(PushRecord &a) const { a.host_sum_q += sum_q; a.host_n_ops += n_ops; a.host_sum_cov += sum_cov; a.host_sum_mapq += sum_mapq; }
};
struct BitsForm {
    const cl_read_tile *t;
    uint32_t *rec_cnt, *sc_off;
    unsigned long long *rb_off;
    uint32_t min_mapq;
    uint64_t head_span;
    void blank(size_t i) const { rec_cnt[i] = 0u; rb_off[i] = 0ull; sc_off[i] = 0u; }
    bool ref_length(BitsChunk &, size_t, int32_t, const uint32_t *, uint32_t, unsigned long long &) const { return false; }
    void read(BitsChunk &o, size_t i, int32_t p, const uint32_t *, uint32_t nops, uint32_t end) const
    {
        o.n_ops += nops;
        const bool in_pileup = end != (uint32_t)p;
        const uint64_t span = end - (uint32_t)p;
        // the heads k_pileup_rows reads: one, unless the span is beyond what a head holds
        rec_cnt[i] = in_pileup ? (uint32_t)((span + head_span - 1) / head_span) : 0u;
        // the read's shares of summed_coverage and summed_mapq (contig_profiler.rs:79-82, :74 -- over its columns,
        // D and N included: SURVEY 8a-7)
        o.sum_cov += span;
        if (t->mapq[i] >= min_mapq) o.sum_mapq += (uint64_t)t->mapq[i] * span;
        const unsigned long long ql = t->qual_off[i + 1] - t->qual_off[i];
        if (!in_pileup || !ql || t->mapq[i] < min_mapq) return;            // in no row (mod.rs:25, :33)
        uint64_t nw;
        if (nops == 1u) nw = (std::min<uint64_t>(span, ql) + 63) >> 6;     // a plain match: its thresholded string as it is
        else if (span > 4 * ql + 1024) {                                   // a span that dwarfs the query: query order + the CIGAR
            nw = ((ql + 63) >> 6) | dut::kRowSparse;
            sc_off[i] = nops; o.n_sc += nops;
        } else nw = (span + 63) >> 6;                                      // mapped into reference order below
        rb_off[i] = nw;
        o.n_words += nw & ~dut::kRowSparse;
    }
};

// cl_push_reads of the pass-bit form: nothing goes to the device here.  One walk over the tile, in chunks on all host
// threads, does everything that needs the reads' CIGAR operations and quality bytes while both are in the cache:
// validation, every read's end, the base-quality test of mod.rs:33 -- one bit per base, qual_pack.cpp --, the read's share
// of summed_baseq (contig_profiler.rs:65-70) and, for every read with mapq >= min_mapping_quality that is not a plain
// match, its pass bits mapped through the CIGAR into REFERENCE order (pass_rows.h): what cl_contig_upload then lays out
// as rows is a string of bits per read, and no CIGAR is staged at all (but those of reads whose span dwarfs their query:
// long N gaps).  A refused tile leaves `hs` and `acc` as they were.
// (pbits / psum: the packed variant, cl_push_reads_bits -- the caller has taken the base-quality test: bit
// t->qual_off[i] + k of pbits <-> quality value k of read i, psum[i] the read's share of summed_baseq; t->qual is unused)
inline Offence push_reads_bits(Staging &hs, PushRecord &acc, const WalkOpts &wo, const cl_read_tile *t, const TileHead &h,
                               const uint64_t *pbits = nullptr, const uint32_t *psum = nullptr)
{
    const uint64_t n = h.n, q0 = h.q0, nq = h.nq;
    const uint64_t rbase = hs.pos.size();
    StageTimer tmr;
    const int32_t last0 = hs.pos.empty() ? 0 : hs.pos.back();
    try {
        hs.rec_cnt.reserve(rbase + n); hs.end.reserve(rbase + n);
        hs.rb_off.reserve(rbase + n + 1); hs.sc_off.reserve(rbase + n + 1);
    } catch (const std::bad_alloc &) {
        return kNoMemory;
    }
    // (entries [rbase, rbase + n) of the staging arrays are written below; their sizes follow when the tile is accepted)
    uint32_t *const h_end = hs.end.data() + rbase;
    unsigned long long *const rb_off = hs.rb_off.data() + rbase;         // first the reads' word counts (| kRowSparse), then their offsets
    uint32_t *const sc_off = hs.sc_off.data() + rbase;
    const uint8_t min_bq = wo.min_bq;
    const int plevel = dut::qual_pack_level();
    const uint8_t *const qsrc = t->qual ? t->qual + q0 : nullptr;
    // ---- first: what needs the CIGAR operations only -- validation, ends, how many words of bits every read will leave ----
    std::vector<BitsChunk> ch = walk_tile<BitsChunk>(t, h, last0, wo.contig_len, h_end,
                                                     BitsForm{t, hs.rec_cnt.data() + rbase, sc_off, rb_off, wo.min_mapq, wo.head_span});
    tmr.lap("push: validate + spans");
    // (entry rbase of the two offset arrays closes the tiles before this one; the walk above used it for this tile's
    // first read: put back whenever the tile is refused)
    const unsigned long long closing_rb = hs.qbits.size();
    const uint32_t closing_sc = (uint32_t)hs.sc.size();
    auto refuse = [&](Offence f) { rb_off[0] = closing_rb; sc_off[0] = closing_sc; return f; };
    if (const Offence f = first_offence(ch); f.st != CL_OK) return refuse(f);
    // ---- where every chunk's strings go: behind the contig's ----
    const size_t grain = walk_grain(n), nchunk = ch.size();
    std::vector<uint64_t> rb_base(nchunk + 1), sc_base(nchunk + 1);
    rb_base[0] = hs.qbits.size(); sc_base[0] = hs.sc.size();
    for (size_t k = 0; k < nchunk; ++k) { rb_base[k + 1] = rb_base[k] + ch[k].n_words; sc_base[k + 1] = sc_base[k] + ch[k].n_sc; }
    if (sc_base[nchunk] > 0xFFFFFFF0ull) return refuse({CL_ERR_RANGE, "more than 2^32 CIGAR operations of gapped reads in one contig"});
    const size_t n_wide_new = wide_reads(ch);
    try {
        hs.qbits.reserve(rb_base[nchunk] + 2); hs.sc.reserve(sc_base[nchunk] + 1);
        hs.pos.reserve(rbase + n); hs.mapq.reserve(rbase + n);
        hs.wide_idx.reserve(hs.wide_idx.size() + n_wide_new); hs.wide_pos.reserve(hs.wide_pos.size() + n_wide_new);
    } catch (const std::bad_alloc &) {
        return refuse(kNoMemory);
    }
    uint64_t *const bits = hs.qbits.data();
    uint32_t *const scw = hs.sc.data();
    // ---- then: what needs the quality bytes -- the base-quality test (one bit per base), the reads' shares of
    //      summed_baseq, and the bits of every read that is not a plain match mapped through its CIGAR into reference
    //      order -- written straight to their place (the chunks' ranges are disjoint) ----
    std::atomic<bool> oom{false};
    dut::parallel_for(nchunk, 1, [&](size_t k) {
        uint64_t sum_q = 0;
        const size_t a = k * grain, b = std::min<size_t>(n, a + grain);
        uint64_t wat = rb_base[k], sat = sc_base[k];
        RawVec<uint64_t> qw;                                    // a read's query-order bits
        RawVec<dut::QueryStretch> um;                           // where its inserted / clipped bases lie
        try {
        for (size_t i = a; i < b; ++i) {
            const unsigned long long cnt = rb_off[i];
            const uint64_t nw = cnt & ~dut::kRowSparse;
            rb_off[i] = wat | (cnt & dut::kRowSparse);
            const uint32_t nsc = sc_off[i];
            sc_off[i] = (uint32_t)sat;
            if (!nw) continue;
            const uint32_t q0i = t->cigar_off[i], nops = t->cigar_off[i + 1] - q0i;
            const uint32_t *cig = t->cigar + q0i;
            const unsigned long long ql = t->qual_off[i + 1] - t->qual_off[i];
            const uint8_t *q = qsrc ? qsrc + (t->qual_off[i] - q0) : nullptr;
            const uint64_t span = h_end[i] - (uint32_t)t->pos[i];
            if (pbits) {
                // the packed variant: the bits are there, in query order from bit qual_off[i]
                const bool sparse = (cnt & dut::kRowSparse) != 0ull;
                sum_q += psum[i];
                if (nops == 1u) copy_bits_to_words(bits + wat, pbits, t->qual_off[i], std::min<uint64_t>(span, ql));
                else if (sparse) {
                    copy_bits_to_words(bits + wat, pbits, t->qual_off[i], ql);
                    memcpy(scw + sat, cig, (size_t)nops * sizeof(uint32_t));
                } else {
                    const uint64_t nqw = (ql + 63) >> 6;
                    qw.resize(nqw + 2); qw[nqw] = 0ull; qw[nqw + 1] = 0ull;
                    copy_bits_to_words(qw.data(), pbits, t->qual_off[i], ql);
                    um.resize(nops + 1);
                    size_t n_um = 0; unsigned long long qlen = 0;
                    dut::ref_bits_from_query(qw.data(), ql, cig, nops, bits + wat, um.data(), &n_um, &qlen);
                }
            } else if (nops == 1u) {
                sum_q += dut::qual_pass_read(q, std::min<uint64_t>(span, ql), min_bq, bits + wat, plevel);
            } else {
                const uint64_t nqw = (ql + 63) >> 6;
                const bool sparse = (cnt & dut::kRowSparse) != 0ull;
                uint64_t *dstq;
                if (sparse) dstq = bits + wat;
                else { qw.resize(nqw + 2); dstq = qw.data(); dstq[nqw] = 0ull; dstq[nqw + 1] = 0ull; }   // (two readable words behind the bits: the mapping looks one word ahead of a clamped position)
                const uint64_t all = dut::qual_pass_read(q, ql, min_bq, dstq, plevel);      // every byte of the string that passes ...
                um.resize(nops + 1);
                size_t n_um = 0; unsigned long long qlen = 0;
                if (sparse) {
                    // (a gapped read keeps its query-order bits and its CIGAR; the mapping below runs into a scratch word
                    // count of zero: only the list of its inserted / clipped bases is wanted)
                    memcpy(scw + sat, cig, (size_t)nops * sizeof(uint32_t));
                    unsigned long long y = 0;
                    for (uint32_t j = 0; j < nops; ++j) {
                        const uint32_t cw = cig[j], op = cw & 15u, l = cw >> 4;
                        if (!((0x193u >> op) & 1u)) continue;
                        if (!((0x181u >> op) & 1u)) { um[n_um].y = y; um[n_um].l = l; ++n_um; }
                        y += l;
                    }
                    qlen = y;
                } else {
                    // ... mapped through the CIGAR into reference order, here where the operations are in the cache
                    dut::ref_bits_from_query(qw.data(), ql, cig, nops, bits + wat, um.data(), &n_um, &qlen);
                }
                sum_q += all - dut::unmatched_pass_sum(q, ql, um.data(), n_um, qlen, min_bq);   // ... minus those of inserted / clipped bases
            }
            wat += nw; sat += nsc;
        }
        } catch (const std::bad_alloc &) { oom.store(true); }
        ch[k].sum_q = sum_q;
    });
    tmr.lap("push: pass bits in reference order");
    if (oom.load()) return refuse(kNoMemory);
    // ---- the tile is accepted (nothing below can fail: the capacity is there) ----
    walk_fold(hs, acc, ch, rbase, t->pos);
    hs.qbits.resize(rb_base[nchunk]); hs.sc.resize(sc_base[nchunk]);
    hs.qbits.data()[rb_base[nchunk]] = 0ull;                    // the word deposit_bits may read behind the last string
    hs.end.resize(rbase + n); hs.rec_cnt.resize(rbase + n);
    hs.rb_off.resize(rbase + n + 1); hs.sc_off.resize(rbase + n + 1);
    rb_off[n] = rb_base[nchunk]; sc_off[n] = (uint32_t)sc_base[nchunk];
    hs.pos.append(t->pos, n);
    hs.mapq.append(t->mapq, n);
    tmr.lap("push: stage small arrays");
    acc.q_dev += nq;                                            // (the contig's quality values so far: none on the device)
    return kNoOffence;
}
