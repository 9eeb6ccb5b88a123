// mh_recode.hip — a compressed batch's training histogram and the batch coded again under another model, without writing
// the decoded bytes (include/mh.h, "RE-CODING BATCHES" and "ORDER 2 IN SEARCH AND RE-CODING").  The batch decoders hold every
// decoded byte in a register for one step; here that byte feeds a counter, or the destination model's code and a BitWriter,
// instead of a store.
//   histc_check_kernel       the batch checks (mhb::check_batch) of a coded histogram
//   recode_check_kernel      the batch checks; out_off, nbits and dropped zeroed
//   recode_idx_len_kernel    one lane per (stream, chunk): decodes under src, sums dst's code lengths and the symbols without a code
//   recode_comb_kernel       the chunks of failed streams count 0 bits; the dropped symbols of the others go to dropped[i]
//   (scan)                   chunk bits -> bit offsets (mh_batch_dev.hpp); then payload bytes -> out_off
//   recode_sizes_kernel      stream i: nbits from the scanned chunk bits, its bytes into out_off
//   recode_cap_kernel        index-free: more symbols than the destination index was sized for -> MHK_STATUS_CAPACITY
//   recode_zero_kernel       clears the payload (edge words are OR-ed) or reports that it does not fit
//   recode_idx_emit_kernel   decodes again and pushes dst's codes through BitWriter; the chunk's index entry
//   recode_walk_kernel       index-free, one lane per stream: count (scans) emit, under the walk cap of dec_walk_kernel
//   recode_tail_kernel       the bytes of the last, partial dword
//   recode_spans_kernel      (EDIT, include/mh.h "EDITING BATCHES") the span lists, in front of the length pass: a stream whose
//                            list is not ascending and disjoint is MH_ERR_ARG
//   spans_*_kernel           search records merged into spans (mh_dev_spans_from_hits): see "span lists" below
//   splice_*_kernel          (include/mh.h "SPLICING BATCHES" and "SPLICING WITH A REPLACEMENT TABLE") spans deleted or replaced
//                            by a string of another length: the same stages with a second scan for output positions and an
//                            index laid out by them.  One family, <TABLE>: one replacement for the call, or one per span, chosen
//                            by the span's tag from a table, and insertions; see "the splice" below
//   splice_spans_kernel      recode_spans_kernel for the table's rule: begin <= end, tag < n_reps
//   spans_tag_kernel        (mh_dev_spans_from_hits_tagged) the lowest pattern number of each merged span
//   histc_idx_kernel        one lane per (stream, chunk): counts the pairs as it decodes; a chunk that fails takes its own
//                            counts back; <FIX>: the chunks that passed inside a stream that failed take theirs back
//   histc_walk_kernel        index-free, one lane per stream: counts, and takes the stream's counts back when it fails
// Verdicts are the batch decoders' (mh_dev_decode_batch, _each, _batch_o2 by the source model): same checks, same statuses.
// Every loop is bounded by a symbol count or nbits_i.  One kernel family serves every order:
//   Dec<K, W>    the source decoder, one policy per model (mhb::Model).  Shared: the order-0/1 tables in LDS as load_tables
//                lays them out, one workgroup per CU.  Set: stream i's slots in L2.  Shared2: the model's order-2 tables
//                read from L2 as dec_idx_kernel<Shared2> reads them, entries masked with IDX2_POS and their context taken
//                from e >> 48.  Set and Shared2: workgroups of 256 lanes, eight per CU.
//   W            some side is order 2: the lane rolls a 16-bit context ((ctx << 8) | sym) & 0xFFFF, of which an order-0/1
//                model reads the last byte.  Else the context is the last symbol.
//   Enc<DLDS, W> the destination's (len, code) at (ctx & mask) << 8 | sym.  DLDS: an order-0/1 destination's len8 image (64
//                KiB order 1, 256 B order 0) in LDS behind the source's tables when it fits (a model set: the order-0
//                image only); else len8 comes from L2.  Codes come from L2: from code64, or under W from the packed enc64
//                of an order-2 model ((len8, code64) over 56 bits or without a packed table).
//   the seam     (SEAM: Shared source under W, so the destination or the histogram is order 2.)  An order-0/1 entry carries
//                one context byte, so the lane of chunk k does not know the symbol two in front of its first one.  The lane
//                of chunk k therefore owns symbols first + 1 ... first + nsym: it decodes one symbol into the next chunk,
//                whose two context bytes it knows; the lane of a stream's first chunk also owns symbol 0 under (prev0,
//                prev0).  recode_idx_len_kernel keeps that symbol's bits apart ("head") and the chunk's last two symbols
//                ("close"); recode_comb_kernel adds head(k - 1) to the bits of chunk k, so the scanned value is the bit
//                offset of chunk k's first code, its destination entry.  The extra symbol never sets a verdict: the next
//                chunk's own lane judges that chunk, and when the stream passed, that lane decoded the same bits in the
//                same context.  A chunk that is not its stream's last has >= 256 symbols, so the two symbols in front of a
//                chunk lie in the previous chunk.  An order-2 source and the index-free walk need none of this.  The
//                histogram's take-back repeats exactly what was counted, the extra symbol included (it is counted only by
//                a chunk that passed).
// The counters: a direct-mapped cache of (key -> u64) in the LDS the tables leave, 64-bit global atomics behind it into the
// caller's 256, 65 536 or 1 << 24 counts.
#include <type_traits>

#include "mh_recode.h"
#include "mh_batch_dev.hpp"
#include "mh_each_dev.hpp"
#include "../../include/mh.h"

namespace mhr {

using mhb::BATCH_STATUS_ARG;
using mhb::Model;
using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;

namespace {

using mhb::BitWriter;
using mhb::Chunk;
using mhb::fail;
using mhb::find_stream;
using mhb::grid_for;
using mhb::grid_threads;
using mhb::gtid;
using mhb::scan_exclusive;
using mhb::stopped;
using mhb::stream_fail;

constexpr int LDS_MAX = 163840;

// The symbol decoder of a lane, one policy per model; next() decodes one symbol in the lane's context ctx.
//   NT, PER_CU   the workgroup shape: that of the model's batch decoder
//   O2           the format of the batch's index entries (mhb::chunk_of)
template <Model K, bool W> struct Dec;
template <bool W> struct Dec<Model::Shared, W> {
    static constexpr int NT = mhb::B_THREADS, PER_CU = 1;
    static constexpr bool O2 = false;
    const uint16_t *lut;
    const uint32_t *sub_base;
    DecTables tabs;
    __device__ __forceinline__ Dec(const Src &s, unsigned char *smem) : tabs(mhb::load_tables(s.b, smem, lut, sub_base)) {}
    __device__ __forceinline__ void stream(const Src &, uint64_t) {}
    __device__ __forceinline__ uint32_t next(const Src &, const BitSrc &src, BitCursor &bc, uint32_t ctx, uint32_t &used, bool &bad) const {
        return mhk::decode_one(lut, sub_base, tabs, src, bc, W ? ctx & 0xFFu : ctx, used, bad);
    }
};
template <> struct Dec<Model::Set, false> {
    static constexpr int NT = 256, PER_CU = 8;
    static constexpr bool O2 = false;
    const uint32_t *row;
    bool o1;
    __device__ __forceinline__ Dec(const Src &, unsigned char *) : row(nullptr), o1(false) {}
    __device__ __forceinline__ void stream(const Src &s, uint64_t i) { row = s.set.ctx_slot + i * 256u; o1 = s.set.type[i] != 0; }
    __device__ __forceinline__ uint32_t next(const Src &s, const BitSrc &src, BitCursor &bc, uint32_t ctx, uint32_t &used, bool &bad) const {
        return mhe::decode_sym(s.set, row, o1 ? ctx : 0u, src, bc, used, bad);
    }
};
template <> struct Dec<Model::Shared2, true> {
    static constexpr int NT = 256, PER_CU = 8;
    static constexpr bool O2 = true;
    const uint16_t *prim;
    const uint32_t *sec_base;
    DecTables tabs;
    __device__ __forceinline__ Dec(const Src &s, unsigned char *) : prim(s.b.prim), sec_base(s.b.sec_base), tabs{s.b.sec, s.b.tree, s.b.P, 0u, 0u} {}
    __device__ __forceinline__ void stream(const Src &, uint64_t) {}
    __device__ __forceinline__ uint32_t next(const Src &, const BitSrc &src, BitCursor &bc, uint32_t ctx, uint32_t &used, bool &bad) const {
        return mhk::decode_one(prim, sec_base, tabs, src, bc, ctx, used, bad);
    }
};
template <Model K, bool W> constexpr bool SEAM = K == Model::Shared && W;

// the lane's context behind sym
template <bool W> __device__ __forceinline__ uint32_t roll(uint32_t ctx, uint32_t sym) { return W ? ((ctx << 8) | sym) & 0xFFFFu : sym; }
// the context in front of a stream's first symbol: prev0, under W (prev0, prev0) (an order-2 source: the call made it so)
template <Model K, bool W> __device__ __forceinline__ uint32_t start_ctx(const Src &s) {
    return SEAM<K, W> ? (s.b.prev0 & 0xFFu) * 0x101u : s.b.prev0;
}
// chunk w of the indexed batch, its entry's context as the lane starts in it; false when w is a gap.  Under SEAM the high
// byte is known only in a stream's first chunk (prev0), elsewhere the lane does not own symbol 0.
template <Model K, bool W>
__device__ __forceinline__ bool chunk_of(const Src &s, uint64_t w, Chunk &c) {
    if (!mhb::chunk_of<Dec<K, W>::O2>(s.b, w, c)) return false;
    if (SEAM<K, W>) c.ctx |= c.first ? 0u : (s.b.prev0 & 0xFFu) << 8;
    return true;
}
// symbol t of chunk c belongs to c's lane (else to the lane of the chunk in front, which knows both context bytes)
template <bool SEAM_> __device__ __forceinline__ bool owns(const Chunk &c, uint32_t t) { return !SEAM_ || t > 0u || c.first == 0u; }

// the destination's codes
template <bool DLDS, bool W> struct Enc {
    const uint8_t *g;
    const uint8_t *l;
    const unsigned long long *code64, *enc64;
    uint32_t mask;
    __device__ __forceinline__ Enc(const Dst &d, unsigned char *smem, uint32_t lds_at)
        : g(d.len8), l(smem + lds_at), code64(d.code64), enc64(d.enc64), mask(d.ctx_mask) {
        if (DLDS) {
            const uint32_t n16 = (d.ctx_mask ? 65536u : 256u) / 16u;
            uint4 *dl = reinterpret_cast<uint4 *>(smem + lds_at);
            for (uint32_t k = threadIdx.x; k < n16; k += blockDim.x) dl[k] = reinterpret_cast<const uint4 *>(d.len8)[k];
            __syncthreads();
        }
    }
    __device__ __forceinline__ uint32_t at(uint32_t ctx, uint32_t sym) const { return ((ctx & mask) << 8) | sym; }
    // one ds_read_u8 (DLDS) or a byte from L2; 0: the pair has no code, skipped (mh_model.hpp:21)
    __device__ __forceinline__ uint32_t len(uint32_t key) const {
        uint32_t v;
        if constexpr (DLDS) v = l[key]; else v = g[key];
        if constexpr (W) return v > 64u ? 0u : v; else return v;
    }
    // the pair's code into bw when `on`; returns its length (0: none)
    __device__ __forceinline__ uint32_t put(BitWriter &bw, uint32_t key, bool on) const {
        if constexpr (W) {
            const uint64_t e = enc64 ? enc64[key] : 0xFF00000000000000ull;
            uint32_t n = uint32_t(e >> 56);
            uint64_t c = e & 0x00FFFFFFFFFFFFFFull;
            if (n == 255u) {                                      // longer than 56 bits, or no packed table
                n = g[key];
                c = code64[key];
            }
            if (n > 64u) n = 0;
            if (n && on) bw.code(c, n);
            return n;
        } else {
            const uint32_t n = len(key);
            if (n && on) bw.code(code64[key], n);
            return n;
        }
    }
    // a destination index entry: the context part in dst's format
    __device__ __forceinline__ uint64_t entry(uint32_t ctx, uint64_t bit) const {
        if constexpr (W) return mask == 0xFFFFu ? (uint64_t(ctx) << 48) | bit : (uint64_t(ctx & 0xFFu) << 56) | bit;
        else return (uint64_t(ctx) << 56) | bit;
    }
};

// the edit     (EDIT: include/mh.h, "EDITING BATCHES" and, under W, "ORDER 2 IN EDITING AND SPLICING".)  Inside its stream's spans
//              a lane codes map[sym] for sym.  It keeps two contexts: ctx, the true symbol, feeds dec.next and roll, so the
//              decoder's dependent chain is what it is without the edit; dctx, the edited symbol, feeds E.at, E.put and
//              E.entry.  A lane seeks the first span that ends behind its first position by a binary search of the stream's
//              list and walks the list with its symbol counter: spans ascend and are disjoint (recode_spans_kernel fails
//              the streams whose list is not so before a lane reads it), so one step is one compare with the span's end and
//              one with its begin, the map lookup predicated on the second.  The cursor keeps the span as 32-bit offsets from
//              the position of the seek, saturated (a chunk has at most MH_CHUNK_MAX symbols and a walk at most
//              MH_BATCH_WALK_MAX_BITS, so a lane's own offsets stay far below 2^32 - 1, which stands for "never").  No list
//              (span_off null): one span over everything.  The map is 256 B of LDS behind the destination's image (Edit::map_lds; read from L2 when the
//              source's tables leave no room).
//              Under W dctx is the last two edited bytes, rolled as ctx is.  Under the seam the lane of chunk k does not own
//              symbol 0 of its chunk but edits it at its position and rolls it into dctx, so its first own code lies under
//              (y[first - 1], y[first]); close is dctx behind the chunk's last symbol, head the next chunk's first symbol,
//              edited at its own position, under close.  The map is pointwise: every lane computes the edited byte two in
//              front itself, no lane needs a word from another.
template <bool DLDS> __device__ __forceinline__ uint32_t map_at(const Dst &d, uint32_t lds_at) {
    return lds_at + (DLDS ? (d.ctx_mask ? 65536u : 256u) : 0u);
}
template <bool EDIT> using Params = std::conditional_t<EDIT, EditParams, RecodeParams>;
template <bool EDIT> struct Spans {
    template <typename P> __device__ __forceinline__ Spans(const P &, unsigned char *, uint32_t) {}
    __device__ __forceinline__ void seek(uint64_t, uint64_t) {}
    __device__ __forceinline__ uint32_t edit(uint32_t sym, uint32_t) { return sym; }
};
template <> struct Spans<true> {
    const unsigned long long *off, *sp;
    const uint8_t *g, *l;
    uint64_t r, rend, origin;
    uint32_t b, e;                      // the span at r, as offsets from origin
    bool lds;
    __device__ __forceinline__ Spans(const EditParams &p, unsigned char *smem, uint32_t at)
        : off(p.ed.span_off), sp(p.ed.spans), g(p.ed.map), l(smem + at), r(0), rend(0), origin(0), b(0u), e(~0u), lds(p.ed.map_lds != 0u) {
        if (lds) {
            for (uint32_t k = threadIdx.x; k < 256u; k += blockDim.x) smem[at + k] = g[k];
            __syncthreads();
        }
    }
    __device__ __forceinline__ uint32_t rel(uint64_t x) const {
        return x <= origin ? 0u : (x - origin >= 0xFFFFFFFFull ? ~0u : uint32_t(x - origin));
    }
    __device__ __forceinline__ void load() {
        if (r < rend) { b = rel(sp[2 * r]); e = rel(sp[2 * r + 1]); } else { b = e = ~0u; }
    }
    // the first span of stream i that ends behind pos
    __device__ __forceinline__ void seek(uint64_t i, uint64_t pos) {
        origin = pos;
        if (!off) return;
        uint64_t lo = off[i], hi = off[i + 1];
        rend = hi;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (sp[2 * mid + 1] > pos) hi = mid; else lo = mid + 1;
        }
        r = lo;
        load();
    }
    // the symbol at origin + pos as the destination sees it; pos goes up by one from the seek (the next span ends behind its
    // begin, which is not in front of this one's end: one step along the list is enough)
    __device__ __forceinline__ uint32_t edit(uint32_t sym, uint32_t pos) {
        if (pos >= e) { ++r; load(); }
        if (pos >= b) sym = lds ? l[sym] : g[sym];
        return sym;
    }
};
// the destination's context as a chunk's lane starts: the entry's byte, edited when the position in front of the chunk lies
// in a span (a stream's first chunk starts from prev0, which is no byte of the message).  The cursor's origin is that
// position: symbol t of the chunk is at offset t + at0(c).  An order-2 entry carries x[first - 2] and x[first - 1]: the
// origin lies BACK = 2 positions in front of the chunk and each of the two is mapped at its own position.
template <Model K, bool W> constexpr uint32_t BACK = Dec<K, W>::O2 ? 2u : 1u;
template <Model K, bool W, bool EDIT> __device__ __forceinline__ uint32_t start_dctx(Spans<EDIT> &sp, const Chunk &c) {
    if (!EDIT) return c.ctx;
    sp.seek(c.i, c.first ? c.first - BACK<K, W> : 0u);              // (a chunk behind the first starts at 256 or more)
    if (!c.first) return c.ctx;
    if constexpr (BACK<K, W> == 2u) {
        const uint32_t hi = sp.edit(c.ctx >> 8, 0u);
        return (hi << 8) | sp.edit(c.ctx & 0xFFu, 1u);
    } else {
        return sp.edit(c.ctx, 0u);
    }
}
template <Model K, bool W> __device__ __forceinline__ uint32_t at0(const Chunk &c) { return c.first ? BACK<K, W> : 0u; }

// ------------------------------------------------------------------------------------------------ the kernels that never decode
// (they read the source batch and the outputs, mhr::RecodeIO, and neither model)

__global__ __launch_bounds__(256) void histc_check_kernel(Src s, int *status, int *stop) {
    const uint64_t i = mhb::gtid();
    if (i > s.b.n) return;
    mhb::check_batch(s.b, i, status, stop);
}

__global__ __launch_bounds__(256) void recode_check_kernel(RecodeIO p, int *status, int *stop) {
    const uint64_t i = mhb::gtid();
    const uint64_t n = p.s.b.n;
    if (i > n) return;
    p.out_off[i] = 0;
    if (!p.s.b.index) p.s.b.sym_off[i] = 0;
    if (i < n) {
        p.out_nbits[i] = 0;
        if (p.dropped) p.dropped[i] = 0;
    }
    mhb::check_batch(p.s.b, i, status, stop);
}

// stream i: payload bits (indexed: from the scanned chunk bits; index-free: the count pass wrote them), bytes into out_off
__global__ __launch_bounds__(256) void recode_sizes_kernel(RecodeIO p, const unsigned long long *cbase, const int *stop) {
    if (mhb::stopped(stop)) return;
    const uint64_t i = mhb::gtid();
    const uint64_t n = p.s.b.n;
    if (i > n) return;
    if (i == n) { p.out_off[i] = 0; return; }
    unsigned long long bits;
    if (p.s.b.index) {
        const uint32_t cs = p.s.b.chunk_shift;
        const uint64_t w0 = (p.s.b.sym_off[i] >> cs) + i, w1 = (p.s.b.sym_off[i + 1] >> cs) + i + 1;
        bits = cbase[w1] - cbase[w0];
        p.out_nbits[i] = bits;
    } else {
        bits = p.out_nbits[i];
    }
    p.out_off[i] = (bits + 7) >> 3;
}

// index-free: the destination index was sized from sym_total; more symbols than that do not fit it (after the scans: offsets
// and lengths are complete)
__global__ void recode_cap_kernel(RecodeIO p, int *status, int *stop) {
    if (mhb::stopped(stop)) return;
    if (p.s.b.sym_off[p.s.b.n] > p.s.b.sym_total) { mhb::fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
}

// zeroes the payload bytes (codes are OR-ed into shared edge dwords) or reports that they do not fit
__global__ __launch_bounds__(256) void recode_zero_kernel(RecodeIO p, int *status, int *stop, uint32_t *tail) {
    if (mhb::stopped(stop)) return;
    const uint64_t bytes = p.out_off[p.s.b.n];
    if (bytes > p.cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { mhb::fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
        return;
    }
    const uint64_t nfull = bytes >> 2;
    uint32_t *o = reinterpret_cast<uint32_t *>(p.out);
    for (uint64_t k = mhb::gtid(); k < nfull; k += uint64_t(gridDim.x) * blockDim.x) o[k] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *tail = 0u;
}

__global__ void recode_tail_kernel(RecodeIO p, const uint32_t *tail, const int *stop) {
    if (mhb::stopped(stop)) return;
    const uint64_t bytes = p.out_off[p.s.b.n];
    if (!(bytes & 3u)) return;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(tail);
    for (uint64_t b = bytes & ~uint64_t(3); b < bytes; ++b) p.out[b] = t[b & 3u];
}

// ------------------------------------------------------------------------------------------------ span lists

// the stream of span r: the last i < n with off[i] <= r (n > 0)
__device__ __forceinline__ uint64_t span_stream(const unsigned long long *off, uint64_t n, uint64_t r) {
    uint64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The span lists of an edit, in front of the length pass: span_off as any offsets (else BATCH_STATUS_ARG and the call stops);
// span r of stream i must have begin < end and must not begin in front of the end of the stream's span before it, else the
// stream's verdict is MH_ERR_ARG and no lane reads its list.  One grid-stride pass over the spans.
__global__ __launch_bounds__(256) void recode_spans_kernel(EditParams p, int *status, int *stop) {
    if (stopped(stop)) return;
    const unsigned long long *off = p.ed.span_off, *sp = p.ed.spans;
    const uint64_t n = p.s.b.n, total = off[n], stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = gtid(); i <= n; i += stride)
        if (mhb::offsets_bad(off, n, total, i)) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
    if (!n) return;
    for (uint64_t r = gtid(); r < total; r += stride) {
        const uint64_t i = span_stream(off, n, r);
        const unsigned long long b = sp[2 * r], e = sp[2 * r + 1];
        if (b >= e || (r > off[i] && sp[2 * r - 1] > b)) stream_fail(p.s.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
    }
}

// Spans from search records (include/mh.h, "EDITING BATCHES").  The records of a stream ascend by end, not by begin: with
// M(r) the least begin of the stream's records r' >= r, records r - 1 and r lie in different spans exactly when
// end(r - 1) < M(r), and a span is (M(its first record), end(its last record)).  M is a reverse min-scan per stream:
//   spans_tile_kernel    tiles of SPAN_TILE records: the scan inside the tile; the tile's first and last stream and the scan
//                        value of its first record
//   spans_carry_kernel   one lane, from the last tile to the first: the least begin behind each tile in the tile's last stream
//   spans_mark_kernel    M complete; 1 for a record that starts a span (scanned next: the record's span number)
//   spans_emit_kernel    a span's first record writes its begin, its last record its end; stream i's span_off
// A total over hit_cap stops the call in spans_tile_kernel's front with MHK_STATUS_CAPACITY and span_off zeroed.  A record
// whose stream is not below n_streams: BATCH_STATUS_ARG and the call stops.
struct SpanParams {
    const unsigned long long *hit_off, *hits;
    uint64_t cap, n;
    unsigned long long *span_off, *spans;
    unsigned long long *mn, *num, *tile;      // mhr::SpanLayout
};
constexpr unsigned long long SPAN_NONE = ~0ull;

__global__ __launch_bounds__(256) void spans_front_kernel(SpanParams p, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i > p.n) return;
    p.span_off[i] = 0;
    if (i == p.n && p.hit_off[p.n] > p.cap) { fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
    if (mhb::offsets_bad(p.hit_off, p.n, p.hit_off[p.n], i)) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
}

__global__ __launch_bounds__(SPAN_TILE) void spans_tile_kernel(SpanParams p, int *status, int *stop) {
    __shared__ unsigned long long ss[SPAN_TILE], sv[SPAN_TILE];
    if (stopped(stop)) return;
    const uint64_t total = p.hit_off[p.n];
    const uint64_t base = uint64_t(blockIdx.x) * SPAN_TILE, r = base + threadIdx.x;
    if (base >= total) return;
    // (behind the last record: a stream of its own that no record shares)
    unsigned long long s = SPAN_NONE, v = SPAN_NONE;
    if (r < total) {
        s = p.hits[3 * r];
        v = p.hits[3 * r + 1];
        if (s >= p.n) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
    }
    ss[threadIdx.x] = s;
    sv[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < SPAN_TILE; d <<= 1) {
        const uint32_t k = threadIdx.x + d;
        const bool take = k < SPAN_TILE && ss[k] == s;               // streams ascend: the same stream d behind, so all between
        const unsigned long long x = take ? sv[k] : SPAN_NONE;
        __syncthreads();
        if (x < v) v = x;
        sv[threadIdx.x] = v;
        __syncthreads();
    }
    if (r < total) p.mn[r] = v;
    if (threadIdx.x == 0) {
        const uint64_t last = (total - base < SPAN_TILE ? total - base : SPAN_TILE) - 1;
        unsigned long long *t = p.tile + 4 * uint64_t(blockIdx.x);
        t[0] = s;
        t[1] = ss[last];
        t[2] = v;
    }
}

__global__ void spans_carry_kernel(SpanParams p, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t total = p.hit_off[p.n];
    const uint64_t nt = (total + SPAN_TILE - 1) / SPAN_TILE;
    unsigned long long carry = SPAN_NONE;                             // of tile k: the least begin behind it in its last stream
    for (uint64_t k = nt; k-- > 0;) {
        unsigned long long *t = p.tile + 4 * k;
        t[3] = carry;
        unsigned long long f = t[2];                                  // the first record's M
        if (t[0] == t[1] && carry < f) f = carry;                     // one stream fills the tile: what lies behind counts
        carry = (k && p.tile[4 * (k - 1) + 1] == t[0]) ? f : SPAN_NONE;
    }
}

__global__ __launch_bounds__(256) void spans_mark_kernel(SpanParams p, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t r = gtid();
    if (r > p.cap + 1) return;
    const uint64_t total = p.hit_off[p.n];
    unsigned long long start = 0;
    if (r < total) {
        const unsigned long long *t = p.tile + 4 * (r / SPAN_TILE);
        const unsigned long long s = p.hits[3 * r];
        unsigned long long m = p.mn[r];
        if (s == t[1] && t[3] < m) p.mn[r] = m = t[3];
        start = r == p.hit_off[s] || p.hits[3 * (r - 1) + 2] < m;
    }
    p.num[r] = start;
}

__global__ __launch_bounds__(256) void spans_emit_kernel(SpanParams p, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t r = gtid();
    const uint64_t total = p.hit_off[p.n];
    if (r <= p.n) p.span_off[r] = p.num[p.hit_off[r]];
    if (r >= total) return;
    const unsigned long long id = p.num[r], next = p.num[r + 1];      // (num has cap + 2 entries; num[total + 1] == num[total])
    const bool start = next != id;
    if (start) p.spans[2 * id] = p.mn[r];
    const unsigned long long s = p.hits[3 * r];
    if (r + 1 == p.hit_off[s + 1] || p.num[r + 2] != next) p.spans[2 * (start ? id : id - 1) + 1] = p.hits[3 * r + 2];
}

// ------------------------------------------------------------------------------------------------ histogram

// Direct-mapped counters in LDS: slot -> (key, u64 count); a key that finds its slot taken goes to the 64-bit global
// counter.  Counts go up and down (a failed chunk takes its counts back): the sums wrap modulo 2^64 and are exact.
// nslot == 0: no LDS left, global atomics only.  The slot hash goes by the key's width: 16 bits, or 24 under W.
template <bool W> struct KeyCache {
    static constexpr uint32_t EMPTY = 0xFFFFFFFFu;
    unsigned long long *cnt;
    uint32_t *tag;
    uint32_t shift, nslot, mask;
    unsigned long long *g;
    __device__ __forceinline__ void init(unsigned char *smem, uint32_t lds_at, uint32_t log2n, uint32_t order, unsigned long long *counts) {
        nslot = log2n ? 1u << log2n : 0u;
        shift = (W ? 32u : 16u) - log2n;
        cnt = reinterpret_cast<unsigned long long *>(smem + lds_at);
        tag = reinterpret_cast<uint32_t *>(cnt + nslot);
        mask = W && order == 2u ? 0xFFFFu : (order ? 0xFFu : 0u);
        g = counts;
        for (uint32_t k = threadIdx.x; k < nslot; k += blockDim.x) { tag[k] = EMPTY; cnt[k] = 0ull; }
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t hash(uint32_t p) const { return W ? (p * 2654435761u) >> shift : ((p * 40503u) & 0xFFFFu) >> shift; }
    __device__ __forceinline__ void add(uint32_t ctx, uint32_t sym, int delta) {
        const uint32_t p = W ? ((ctx & mask) << 8) | sym : (mask ? (ctx << 8) | sym : sym);    // (!W: ctx is one byte)
        const unsigned long long d = static_cast<unsigned long long>(static_cast<long long>(delta));
        if (nslot) {
            const uint32_t slot = mask ? hash(p) : p;                              // (nslot >= 256: order 0 never collides)
            uint32_t t = tag[slot];
            if (t == EMPTY) {
                const uint32_t old = atomicCAS(&tag[slot], EMPTY, p);
                t = old == EMPTY ? p : old;
            }
            if (t == p) { atomicAdd(&cnt[slot], d); return; }
        }
        atomicAdd(&g[p], d);
    }
    __device__ __forceinline__ void flush() {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < nslot; k += blockDim.x) {
            const unsigned long long v = cnt[k];
            if (v) atomicAdd(&g[tag[k]], v);
        }
    }
};

// `count` symbols of chunk c from its entry, the lane's own counted `delta` times (0: decode only); ext (SEAM only): when
// these symbols end exactly at the chunk's end, the first symbol of the next chunk is counted too.  Returns the symbols done;
// used / bad describe the `count` symbols alone.
template <Model K, bool W>
__device__ __forceinline__ uint32_t walk_chunk(const Src &s, const Dec<K, W> &dec, const Chunk &c, uint32_t count, bool ext, int delta,
                                               KeyCache<W> &kc, uint32_t &used, bool &bad) {
    uint64_t bit0;
    const BitSrc src = mhb::stream_src(s.b.payload, s.b.pay_off[c.i], c.nb, bit0);
    BitCursor bc;
    bc.init(src, bit0 + c.start);
    uint32_t ctx = c.ctx, t = 0;
    used = 0; bad = false;
    for (; t < count; ++t) {
        const uint32_t sym = dec.next(s, src, bc, ctx, used, bad);
        if (bad) break;
        if (delta && owns<SEAM<K, W>>(c, t)) kc.add(ctx, sym, delta);
        ctx = roll<W>(ctx, sym);
    }
    if constexpr (SEAM<K, W>) {
        if (ext && !c.last && !bad && used == c.end - c.start) {
            uint32_t u2 = used;
            bool b2 = false;
            const uint32_t sym = dec.next(s, src, bc, ctx, u2, b2);
            if (!b2 && delta) kc.add(ctx, sym, delta);
        }
    }
    return t;
}

template <Model K, bool W, bool FIX>
__global__ __launch_bounds__((Dec<K, W>::NT)) void histc_idx_kernel(HistParams p, uint64_t nwork, uint32_t lds_at, uint32_t log2n, int *status,
                                                                  const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    if (FIX && *reinterpret_cast<const volatile int *>(status) == 0) return;      // no stream failed: nothing to take back
    Dec<K, W> dec(p.s, smem);
    KeyCache<W> kc;
    kc.init(smem, lds_at, log2n, p.order, p.counts);
    for (uint64_t base = uint64_t(blockIdx.x) * blockDim.x; base < nwork; base += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t w = base + threadIdx.x;
        Chunk c;
        if (w < nwork && chunk_of<K, W>(p.s, w, c)) {
            dec.stream(p.s, c.i);
            const int verdict = p.s.b.stream_status[c.i];
            uint32_t used; bool bad;
            if (!FIX && verdict != MH_ERR_ARG) {
                if (!c.entry_ok()) {
                    stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                } else {
                    const uint32_t done = walk_chunk<K, W>(p.s, dec, c, c.nsym, true, 1, kc, used, bad);
                    if (bad || used != c.end - c.start) {           // (the extra symbol was not counted)
                        stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                        walk_chunk<K, W>(p.s, dec, c, done, false, -1, kc, used, bad);
                    }
                }
            }
            if (FIX && verdict == MH_ERR_CORRUPT && c.entry_ok()) {               // (a chunk that failed has taken its counts back)
                walk_chunk<K, W>(p.s, dec, c, c.nsym, false, 0, kc, used, bad);
                if (!bad && used == c.end - c.start) walk_chunk<K, W>(p.s, dec, c, c.nsym, true, -1, kc, used, bad);
            }
        }
    }
    kc.flush();
}

// at most `limit` symbols of stream i from bit 0, each counted `delta` times; returns the symbols done
template <Model K, bool W>
__device__ __forceinline__ uint64_t walk_stream(const Src &s, const Dec<K, W> &dec, uint64_t i, uint64_t nb, uint64_t limit, int delta,
                                                KeyCache<W> &kc, uint32_t &used, bool &bad) {
    uint64_t bit0;
    const BitSrc src = mhb::stream_src(s.b.payload, s.b.pay_off[i], nb, bit0);
    BitCursor bc;
    bc.init(src, bit0);
    uint32_t ctx = start_ctx<K, W>(s);
    uint64_t k = 0;
    used = 0; bad = false;
    // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
    while (used < nb && k < limit) {
        const uint32_t sym = dec.next(s, src, bc, ctx, used, bad);
        if (bad) break;
        kc.add(ctx, sym, delta);
        ctx = roll<W>(ctx, sym);
        ++k;
    }
    return k;
}

template <Model K, bool W>
__global__ __launch_bounds__((Dec<K, W>::NT)) void histc_walk_kernel(HistParams p, uint32_t lds_at, uint32_t log2n, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K, W> dec(p.s, smem);
    KeyCache<W> kc;
    kc.init(smem, lds_at, log2n, p.order, p.counts);
    const uint64_t n = p.s.b.n;
    for (uint64_t base = uint64_t(blockIdx.x) * blockDim.x; base < n; base += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        if (i < n && p.s.b.stream_status[i] == MH_OK) {
            const uint64_t nb = p.s.b.nbits[i];
            if (nb > p.s.b.walk_max_bits) {
                stream_fail(p.s.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
            } else {
                dec.stream(p.s, i);
                uint32_t used; bool bad;
                const uint64_t done = walk_stream<K, W>(p.s, dec, i, nb, ~uint64_t(0), 1, kc, used, bad);
                if (bad || used != nb) {                            // src/coding.cpp:158: the stream ends exactly at nbits
                    stream_fail(p.s.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                    walk_stream<K, W>(p.s, dec, i, nb, done, -1, kc, used, bad);
                }
            }
        }
    }
    kc.flush();
}

// ------------------------------------------------------------------------------------------------ re-code

template <Model K, bool DLDS, bool W, bool EDIT>
__global__ __launch_bounds__((Dec<K, W>::NT)) void recode_idx_len_kernel(Params<EDIT> p, uint64_t nwork, uint32_t lds_at, unsigned long long *cbits,
                                                                       uint32_t *cdrop, uint32_t *chead, uint32_t *cclose, int *status,
                                                                       const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K, W> dec(p.s, smem);
    const Enc<DLDS, W> E(p.dst, smem, lds_at);
    Spans<EDIT> sp(p, smem, map_at<DLDS>(p.dst, lds_at));
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of<K, W>(p.s, w, c) || p.s.b.stream_status[c.i] == MH_ERR_ARG) continue;
        if (!c.entry_ok()) { stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        dec.stream(p.s, c.i);
        uint32_t ctx = c.ctx, used = 0, bits = 0, drops = 0;
        uint32_t dctx = start_dctx<K, W, EDIT>(sp, c);
        bool bad = false;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {
            const uint32_t sym = dec.next(p.s, src, bc, ctx, used, bad);
            if (bad) break;
            const uint32_t dsym = sp.edit(sym, t + at0<K, W>(c));
            if (owns<SEAM<K, W>>(c, t)) {
                const uint32_t l = E.len(E.at(EDIT ? dctx : ctx, dsym));
                bits += l;
                drops += l == 0u;
            }
            if (EDIT) dctx = roll<W>(dctx, dsym);
            ctx = roll<W>(ctx, sym);
        }
        if (bad || used != c.end - c.start) { stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        if constexpr (SEAM<K, W>) {
            if (!c.last) {
                // the next chunk's first symbol, whose two context bytes only this lane knows.  No verdict: when the stream
                // passes, the next chunk's lane decoded the same bits in the same context.
                cclose[w] = EDIT ? dctx : ctx;
                uint32_t u2 = used;
                bool b2 = false;
                const uint32_t sym = dec.next(p.s, src, bc, ctx, u2, b2);
                if (!b2) {
                    const uint32_t l = E.len(E.at(EDIT ? dctx : ctx, sp.edit(sym, c.nsym + at0<K, W>(c))));
                    chead[w] = l;
                    drops += l == 0u;
                }
            }
        }
        cbits[w] = bits;
        cdrop[w] = drops;
    }
}

// the chunks of failed streams count 0 bits; chunk k of the others: its own bits and, behind a seam, its first symbol's,
// which the lane in front priced; the dropped symbols go to dropped[i]
template <bool SEAM_>
__global__ __launch_bounds__(256) void recode_comb_kernel(RecodeParams p, uint64_t nwork, unsigned long long *cbits, const uint32_t *cdrop,
                                                          const uint32_t *chead, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t w = gtid();
    if (w > nwork) return;
    unsigned long long v = 0;
    if (w < nwork) {
        const uint32_t cs = p.s.b.chunk_shift;
        const uint64_t i = find_stream(p.s.b.sym_off, p.s.b.n, cs, w);
        if (i < p.s.b.n) {
            const uint64_t a = p.s.b.sym_off[i], ni = p.s.b.sym_off[i + 1] - a;
            const uint64_t k = w - ((a >> cs) + i);
            if ((k << cs) < ni && p.s.b.stream_status[i] == MH_OK) {
                v = cbits[w];
                if constexpr (SEAM_) v += k ? chead[w - 1] : 0u;
                const uint32_t d = cdrop[w];
                if (d && p.dropped) atomicAdd(&p.dropped[i], static_cast<unsigned long long>(d));
            }
        }
    }
    cbits[w] = v;
}

template <Model K, bool DLDS, bool W, bool EDIT>
__global__ __launch_bounds__((Dec<K, W>::NT)) void recode_idx_emit_kernel(Params<EDIT> p, uint64_t nwork, uint32_t lds_at,
                                                                        const unsigned long long *cbase, const uint32_t *chead,
                                                                        const uint32_t *cclose, uint32_t *tail, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K, W> dec(p.s, smem);
    const Enc<DLDS, W> E(p.dst, smem, lds_at);
    Spans<EDIT> sp(p, smem, map_at<DLDS>(p.dst, lds_at));
    const uint64_t bytes = p.out_off[p.s.b.n];
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint32_t cs = p.s.b.chunk_shift;
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of<K, W>(p.s, w, c) || p.s.b.stream_status[c.i] != MH_OK) continue;
        const unsigned long long b0 = cbase[w];
        const uint64_t rel = b0 - cbase[(p.s.b.sym_off[c.i] >> cs) + c.i];          // relative to the stream's own payload
        const bool seam = SEAM<K, W> && c.first != 0u;                              // symbol 0 is the lane's in front
        uint32_t dctx = start_dctx<K, W, EDIT>(sp, c);
        if (p.out_index) p.out_index[w] = E.entry(seam ? cclose[w - 1] : (EDIT ? dctx : c.ctx), rel);
        if (!p.out) continue;
        if constexpr (!SEAM<K, W>) { if (cbase[w + 1] == b0) continue; }            // (SEAM: the lane's codes are not the chunk's)
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        dec.stream(p.s, c.i);
        BitWriter bw;
        bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[c.i]) * 8u + rel + (seam ? chead[w - 1] : 0u));
        uint32_t ctx = c.ctx, used = 0;
        bool bad = false;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {            // (the stream passed: bad stays false)
            const uint32_t sym = dec.next(p.s, src, bc, ctx, used, bad);
            const uint32_t dsym = sp.edit(sym, t + at0<K, W>(c));
            if (owns<SEAM<K, W>>(c, t)) E.put(bw, E.at(EDIT ? dctx : ctx, dsym), true);
            if (EDIT) dctx = roll<W>(dctx, dsym);
            ctx = roll<W>(ctx, sym);
        }
        if constexpr (SEAM<K, W>) {
            if (!c.last && !bad) {
                const uint32_t sym = dec.next(p.s, src, bc, ctx, used, bad);
                E.put(bw, E.at(EDIT ? dctx : ctx, sp.edit(sym, c.nsym + at0<K, W>(c))), !bad);
            }
        }
        bw.finish();
    }
}

// EMIT = false: the stream's verdict, its symbols into sym_off[i] (scanned next), its dst bits and dropped symbols;
// true: its codes from out_off[i] and its index entries
template <Model K, bool DLDS, bool W, bool EMIT, bool EDIT>
__global__ __launch_bounds__((Dec<K, W>::NT)) void recode_walk_kernel(Params<EDIT> p, uint32_t lds_at, uint32_t *tail, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K, W> dec(p.s, smem);
    const Enc<DLDS, W> E(p.dst, smem, lds_at);
    Spans<EDIT> sp(p, smem, map_at<DLDS>(p.dst, lds_at));
    const uint64_t n = p.s.b.n;
    const uint64_t bytes = EMIT ? p.out_off[n] : 0;
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint32_t ocs = p.out_chunk_shift;
    for (uint64_t i = gtid(); i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (p.s.b.stream_status[i] != MH_OK) continue;
        const uint64_t nb = p.s.b.nbits[i];
        uint64_t a = 0, count = ~uint64_t(0);
        if (EMIT) {
            a = p.s.b.sym_off[i];
            count = p.s.b.sym_off[i + 1] - a;
            if (!count) continue;
        } else if (nb > p.s.b.walk_max_bits) {
            stream_fail(p.s.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
            continue;
        }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0);
        dec.stream(p.s, i);
        BitWriter bw;
        if (EMIT && p.out) bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[i]) * 8u);
        uint32_t ctx = start_ctx<K, W>(p.s), used = 0;
        uint32_t dctx = ctx;
        sp.seek(i, 0);
        bool bad = false;
        uint64_t k = 0, bits = 0, drops = 0;
        // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
        while (used < nb && !bad && k < count) {
            if (EMIT && p.out_index && (k & ((uint64_t(1) << ocs) - 1u)) == 0) p.out_index[(a >> ocs) + i + (k >> ocs)] = E.entry(EDIT ? dctx : ctx, bits);
            const uint32_t sym = dec.next(p.s, src, bc, ctx, used, bad);
            if (bad) break;
            const uint32_t dsym = sp.edit(sym, uint32_t(k));
            const uint32_t key = E.at(EDIT ? dctx : ctx, dsym);
            if (EDIT) dctx = roll<W>(dctx, dsym);
            uint32_t l;
            if (EMIT) {
                l = E.put(bw, key, p.out != nullptr);
            } else {
                l = E.len(key);
                drops += l == 0u;
            }
            bits += l;
            ctx = roll<W>(ctx, sym);
            ++k;
        }
        if (EMIT) { if (p.out) bw.finish(); continue; }
        if (bad || used != nb) { stream_fail(p.s.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        p.s.b.sym_off[i] = k;                                       // src/coding.cpp:158: the stream ends exactly at nbits
        p.out_nbits[i] = bits;
        if (p.dropped) p.dropped[i] = drops;
    }
}

// ------------------------------------------------------------------------------------------------ splice

// the splice   (include/mh.h, "SPLICING BATCHES" and "SPLICING WITH A REPLACEMENT TABLE": order 0/1 on both sides; "ORDER 2 IN
//              EDITING AND SPLICING": an order-2 source under any destination, see "order 2" below.)  A span that
//              begins inside the message is replaced by a string of another length (0 bytes: deleted), so output positions
//              are not source positions.  A lane keeps ctx (the true symbol, for dec.next) and dctx (the last output byte;
//              under an order-2 source the last two), as the edit does, and walks its symbols with the cursor below.  The lane whose symbols contain a span's begin
//              owns its replacement (an insertion at a chunk boundary belongs to the lane of the chunk that starts there).
//              Indexed source, one lane per source chunk: the length pass counts the chunk's output symbols beside its bits,
//              a second scan turns them into output positions, and the emit pass writes a destination index entry in front
//              of every output symbol whose position is a multiple of the chunk size: each output boundary is met by
//              exactly one lane.
//   TABLE      One kernel family for both calls; TABLE selects how a span's replacement is found and nothing else.  false:
//              the call's one string, sp.rep / sp.rep_len, and spans obey begin < end (recode_spans_kernel).  true: span r
//              is replaced by table entry tag[r], and begin == end inserts in front of x[begin] (splice_spans_kernel: begin
//              <= end, tag < n_reps, else the stream fails alone and no lane reads its list).  With every tag 0, a one-entry
//              table and no insertion the two calls run the same steps on the same workspace layout.  The replacement is
//              read from L2, once per owned span.
//   cursor     Spans obey begin <= end <= next begin, so several may begin at one position: step() codes the replacements of
//              all spans that begin at the current position, in list order, before it says whether the symbol is coded.
//   start      (An order-0/1 source; "order 2" below says what changes for two bytes.)  The destination context of a lane
//              whose chunk starts at `first` is the last output byte in front of it.  With
//              first - 1 in no span that is the entry's byte; in a span with a non-empty replacement it is that
//              replacement's last byte; in a deleted span r it is sctx[r], which lies mid-chunk in general.
//              splice_back_kernel finds it per span before the length pass (!TABLE: launched only when rep_len == 0; TABLE:
//              always, the host does not know which entries are empty): one lane per deleted span that reaches over a chunk
//              boundary walks back through the touching spans in front of it while they are empty (bounded by the stream's
//              span count); a touching span with a non-empty replacement gives its last byte, else the lane decodes the
//              chunk that holds begin - 1 up to that symbol (or reads the next chunk's entry when begin is a boundary).  The
//              two hot kernels then look the byte up and keep no cross-lane dependency; the comb kernel stays a pure sum.
//              A decode that fails there stores nothing of value: the lane of that chunk fails the stream in the length
//              pass.
//   price      price[2k], price[2k + 1]: the bits and drops of entry k's bytes behind its first (splice_price_kernel, which
//              also checks the table); the length pass prices the first byte in dctx and adds them.  !TABLE: entry 0 is rep.
//   order 2    (SW<K>: an order-2 source, K = Shared2, under any destination; include/mh.h "ORDER 2 IN EDITING AND SPLICING";
//              TABLE only.)  ctx and dctx are 16-bit contexts, rolled; dctx is the last TWO output bytes, of which an order-0/1
//              destination reads the later one.  start: a replacement of two or more bytes supplies both; a shorter one has
//              sctx[r], both bytes behind it, and splice_back_kernel serves every span shorter than two bytes with a chunk
//              boundary F in (begin, end + 1]: at F = end + 1 x[F - 1] is the first byte behind the span and the byte in
//              front of it the last output byte behind the replacement.  It collects the two bytes from the back: the
//              replacement's, then those of the touching spans and insertions in front, then source bytes (the entry of the
//              chunk at that position decoded up to it, at most twice: behind one source byte a span may touch again), prev0
//              in front of position 0.  price: entry k's bytes from its THIRD on, triple (j - 2, j - 1, j) under the
//              destination's mask; the lanes code the first two in dctx.
template <Model K> constexpr bool SW = K == Model::Shared2;
template <bool TABLE> using SpParams = std::conditional_t<TABLE, SpliceTableParams, SpliceParams>;
template <bool TABLE> struct Cut {
    const unsigned long long *off, *sp, *rep_off;
    const uint32_t *tag;
    const uint8_t *bytes;
    const uint8_t *rep;                 // the replacement of the last fetch, its entry and length
    uint32_t k, rep_len;
    uint64_t r, rend, origin;
    uint32_t b, e;                      // the span at r, as offsets from origin (saturated; ~0u: never)
    bool own;                           // the span at r begins at or behind origin and its replacement is not coded yet
    __device__ __forceinline__ explicit Cut(const SpParams<TABLE> &p)
        : off(p.sp.span_off), sp(p.sp.spans), rep_off(nullptr), tag(nullptr), bytes(nullptr), rep(nullptr), k(0u), rep_len(0u),
          r(0), rend(0), origin(0), b(~0u), e(~0u), own(false) {
        if constexpr (TABLE) { rep_off = p.tb.rep_off; tag = p.tb.span_tag; bytes = p.tb.rep_bytes; }
        else { rep = p.sp.rep; rep_len = p.sp.rep_len; }
    }
    __device__ __forceinline__ uint32_t rel(uint64_t x) const {
        return x <= origin ? 0u : (x - origin >= 0xFFFFFFFFull ? ~0u : uint32_t(x - origin));
    }
    __device__ __forceinline__ void load() {
        if (r < rend) { b = rel(sp[2 * r]); e = rel(sp[2 * r + 1]); own = sp[2 * r] >= origin; } else { b = e = ~0u; own = false; }
    }
    // the replacement of span q.  !TABLE: the call's, entry 0, which the constructor set: no loads
    __device__ __forceinline__ void fetch(uint64_t q) {
        if constexpr (TABLE) {
            k = tag[q];
            const unsigned long long o = rep_off[k];
            rep = bytes + o;
            rep_len = uint32_t(rep_off[k + 1] - o);
        }
    }
    // stream i from its first symbol: every span of the list, an insertion at 0 included
    __device__ __forceinline__ void start(uint64_t i) {
        origin = 0;
        r = off[i];
        rend = off[i + 1];
        load();
    }
    // stream i from position first > 0: the first span that ends at or behind first (a span or an insertion in front of
    // first - 1 is another lane's); true when that span holds first - 1
    __device__ __forceinline__ bool seek(uint64_t i, uint64_t first) {
        origin = first;
        uint64_t lo = off[i], hi = off[i + 1];
        rend = hi;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (sp[2 * mid + 1] >= first) hi = mid; else lo = mid + 1;
        }
        r = lo;
        load();
        return r < rend && sp[2 * r] < first;
    }
    // the symbol at origin + pos, pos going up by one from the start: emit() runs once for every span that begins here (the
    // replacement fetched); true when the symbol lies in no span and is coded
    template <typename F> __device__ __forceinline__ bool step(uint32_t pos, F &&emit) {
        for (;;) {
            if (pos < b) return true;
            if (own && pos == b) { fetch(r); emit(); own = false; }
            if (pos < e) return false;
            ++r;
            load();
        }
    }
};

// The destination context as chunk c's lane starts (see "start" above); the cursor is left at the chunk's first symbol.
// W: the last two output bytes.  q is the last span that begins in front of `first`.  It holds first - 1: the two bytes behind
// its replacement, tail2(q).  It ends at first - 1 (an insertion there included): the later of those two, then the entry's
// x[first - 1].  Else both bytes of the entry.
template <bool W, bool TABLE> __device__ __forceinline__ uint32_t splice_start(Cut<TABLE> &cu, const Chunk &c, const uint32_t *sctx) {
    if (!c.first) { cu.start(c.i); return c.ctx; }
    const bool in = cu.seek(c.i, c.first);
    if constexpr (W) {
        if (!in && !(cu.r > cu.off[c.i] && cu.sp[2 * cu.r - 1] + 1u == c.first)) return c.ctx;
        const uint64_t q = in ? cu.r : cu.r - 1u;
        cu.fetch(q);
        const uint32_t t2 = cu.rep_len >= 2u ? (uint32_t(cu.rep[cu.rep_len - 2u]) << 8) | cu.rep[cu.rep_len - 1u] : sctx[q];
        return in ? t2 : ((t2 & 0xFFu) << 8) | (c.ctx & 0xFFu);
    } else {
        if (!in) return c.ctx;
        cu.fetch(cu.r);
        return cu.rep_len ? cu.rep[cu.rep_len - 1u] : sctx[cu.r];
    }
}
// the destination context behind a replacement of rep_len > 0 bytes that was entered in dctx
template <bool W> __device__ __forceinline__ uint32_t rep_ctx(uint32_t dctx, const uint8_t *rep, uint32_t rep_len) {
    if (!W) return rep[rep_len - 1u];
    return ((rep_len >= 2u ? uint32_t(rep[rep_len - 2u]) : dctx & 0xFFu) << 8) | rep[rep_len - 1u];
}

// the end of span q's replacement: empty, or its last byte at base[end - 1] (splice_back_kernel asks for the byte only
// where it needs it)
struct RepEnd {
    const uint8_t *base;
    uint64_t end;
    bool empty;
    __device__ __forceinline__ uint32_t last() const { return base[end - 1u]; }
};
template <bool TABLE> __device__ __forceinline__ RepEnd rep_end(const SpParams<TABLE> &p, uint64_t q) {
    if constexpr (TABLE) {
        const uint32_t k = p.tb.span_tag[q];
        const unsigned long long o0 = p.tb.rep_off[k], o1 = p.tb.rep_off[k + 1];
        return {p.tb.rep_bytes, o1, o1 == o0};
    } else {
        return {p.sp.rep, p.sp.rep_len, p.sp.rep_len == 0u};
    }
}

__global__ __launch_bounds__(256) void splice_check_kernel(SpliceParams p, int *status, int *stop) {
    const uint64_t i = mhb::gtid();
    const uint64_t n = p.s.b.n;
    if (i > n) return;
    p.out_off[i] = 0;
    p.sp.out_sym_off[i] = 0;
    if (!p.s.b.index) p.s.b.sym_off[i] = 0;
    if (i < n) {
        p.out_nbits[i] = 0;
        if (p.dropped) p.dropped[i] = 0;
    }
    mhb::check_batch(p.s.b, i, status, stop);
}

// recode_spans_kernel reads the list through EditParams: the same pointers, no map
inline EditParams spans_view(const SpliceParams &p) {
    EditParams e{};
    static_cast<RecodeParams &>(e) = p;
    e.ed.span_off = p.sp.span_off;
    e.ed.spans = p.sp.spans;
    return e;
}

// entry k's bits and drops behind its first byte into price[2k], price[2k + 1]: pair j in the context of byte j - 1.  One
// workgroup per entry.  TABLE: rep_off[0] == 0, no decreasing offsets, no entry over MH_SPLICE_MAX_REP bytes, else
// BATCH_STATUS_ARG and the call stops; an entry is read only when it lies inside the table's rep_off[n_reps] bytes.  !TABLE:
// the one entry (rep, rep_len), which the call checked.
// W: from the third byte on, byte j in the context of bytes j - 2 and j - 1.
template <bool TABLE, bool W>
__global__ __launch_bounds__(256) void splice_price_kernel(SpParams<TABLE> p, uint32_t *price, int *status, int *stop) {
    __shared__ uint32_t acc[2];
    uint64_t nr = 1;
    if constexpr (TABLE) {
        nr = p.tb.n_reps;
        if (blockIdx.x == 0 && threadIdx.x == 0 && p.tb.rep_off[0] != 0) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
    }
    for (uint64_t k = blockIdx.x; k < nr; k += gridDim.x) {
        const uint8_t *rep = p.sp.rep;
        uint32_t len = p.sp.rep_len;
        if constexpr (TABLE) {
            const unsigned long long o0 = p.tb.rep_off[k], o1 = p.tb.rep_off[k + 1];
            if (o1 < o0 || o1 - o0 > MH_SPLICE_MAX_REP || o1 > p.tb.rep_off[nr]) {
                if (threadIdx.x == 0) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
                continue;
            }
            rep = p.tb.rep_bytes + o0;
            len = uint32_t(o1 - o0);
        }
        if (threadIdx.x < 2u) acc[threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t j = threadIdx.x;
        if (j >= (W ? 2u : 1u) && j < len) {
            uint32_t l;
            if constexpr (W) {
                l = p.dst.len8[((((uint32_t(rep[j - 2u]) << 8) | rep[j - 1u]) & p.dst.ctx_mask) << 8) | rep[j]];
                if (l > 64u) l = 0u;
            } else {
                l = p.dst.len8[((uint32_t(rep[j - 1u]) & p.dst.ctx_mask) << 8) | rep[j]];
            }
            atomicAdd(&acc[0], l);
            if (!l) atomicAdd(&acc[1], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 2u) price[2 * k + threadIdx.x] = acc[threadIdx.x];
        __syncthreads();
    }
}

// recode_spans_kernel for the table's rule: span r of stream i with begin > end, beginning in front of the end of the span
// before it, or with a tag that is no table entry: the stream's verdict is MH_ERR_ARG.  Spans and no table: the call stops.
__global__ __launch_bounds__(256) void splice_spans_kernel(SpliceTableParams p, int *status, int *stop) {
    if (stopped(stop)) return;
    const unsigned long long *off = p.sp.span_off, *sp = p.sp.spans;
    const uint64_t n = p.s.b.n, total = off[n], stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = gtid(); i <= n; i += stride)
        if (mhb::offsets_bad(off, n, total, i)) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
    if (!n) return;
    if (total && !p.tb.n_reps) {
        if (gtid() == 0) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
        return;
    }
    for (uint64_t r = gtid(); r < total; r += stride) {
        const uint64_t i = span_stream(off, n, r);
        const unsigned long long b = sp[2 * r], e = sp[2 * r + 1];
        if (b > e || (r > off[i] && sp[2 * r - 1] > b) || p.tb.span_tag[r] >= p.tb.n_reps)
            stream_fail(p.s.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
    }
}

// the order-2 look-back's decode: the context behind the first `count` symbols of chunk c of stream i (count <= c.nsym; a
// decode that fails returns what it has)
template <Model K>
__device__ __forceinline__ uint32_t splice_ctx_at(const Src &s, Dec<K, SW<K>> &dec, uint64_t i, const Chunk &c, uint32_t count) {
    uint64_t bit0;
    const BitSrc src = mhb::stream_src(s.b.payload, s.b.pay_off[i], c.nb, bit0);
    BitCursor bc;
    bc.init(src, bit0 + c.start);
    dec.stream(s, i);
    uint32_t ctx = c.ctx, used = 0;
    bool bad = false;
    for (uint32_t t = 0; t < count && !bad; ++t) {
        const uint32_t sym = dec.next(s, src, bc, ctx, used, bad);
        if (bad) break;
        ctx = roll<SW<K>>(ctx, sym);
    }
    return ctx;
}

// span q's replacement (TABLE)
struct RepBytes {
    const uint8_t *b;
    uint32_t len;
};
__device__ __forceinline__ RepBytes rep_bytes(const SpliceTableParams &p, uint64_t q) {
    const uint32_t k = p.tb.span_tag[q];
    const unsigned long long o = p.tb.rep_off[k];
    return {p.tb.rep_bytes + o, uint32_t(p.tb.rep_off[k + 1] - o)};
}

// indexed: sctx[r] for every deleted span r over a chunk boundary, the last output byte in front of it (see "start" above).
// More spans than the workspace has room for: MHK_STATUS_CAPACITY and the call stops.  SW<K>: sctx[r] for every span r
// replaced by fewer than two bytes with a chunk boundary in (begin, end + 1], the last two output bytes behind its
// replacement (see "order 2" above).
template <Model K, bool TABLE>
__global__ __launch_bounds__((Dec<K, SW<K>>::NT)) void splice_back_kernel(SpParams<TABLE> p, uint32_t *sctx, int *status, int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K, SW<K>> dec(p.s, smem);
    const unsigned long long *off = p.sp.span_off, *sp = p.sp.spans;
    const uint64_t n = p.s.b.n, total = off[n];
    if (total > p.sp.span_cap) {
        if (gtid() == 0) { fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
        return;
    }
    if (!n) return;
    const uint32_t cs = p.s.b.chunk_shift;
    for (uint64_t r = gtid(); r < total; r += uint64_t(gridDim.x) * blockDim.x) {
        sctx[r] = 0u;
        // Two bodies on purpose.  The order-2 walk (two bytes, through touching spans and source bytes in turn) run with one
        // byte would serve order 0/1 too, but the order-0/1 kernels must compile to what they were: even sharing the decode
        // loop alone moved their four resource lines (+2 ... +8 instructions, 2 SGPR spills), so that body stays as it was.
        if constexpr (SW<K>) {
            if (((sp[2 * r + 1] + 1u) >> cs) == (sp[2 * r] >> cs)) continue;   // no chunk starts in (begin, end + 1]: no lane asks
            const uint64_t i = span_stream(off, n, r);
            if (p.s.b.stream_status[i] != MH_OK) continue;            // (a passed stream's tags are table entries)
            const RepBytes me = rep_bytes(p, r);
            if (me.len >= 2u) continue;                               // its own last two bytes serve
            const uint64_t a = p.s.b.sym_off[i], ni = p.s.b.sym_off[i + 1] - a;
            if (sp[2 * r] >= ni) continue;                            // the span is ignored
            // from the back: acc holds `got` bytes, the last output byte lowest
            uint32_t acc = me.len ? me.b[0] : 0u, got = me.len;
            uint64_t q = r, pos = sp[2 * r];                          // the output in front of x[pos], spans q and later passed
            uint64_t have = ~uint64_t(0);                             // two: (x[have - 2], x[have - 1])
            uint32_t two = 0;
            while (got < 2u) {                                        // (at most the stream's spans and two bytes more)
                if (q > off[i] && sp[2 * q - 1] == pos) {             // a span or an insertion in front touches
                    const RepBytes f = rep_bytes(p, --q);
                    for (uint32_t j = f.len; j > 0u && got < 2u; --j) acc |= uint32_t(f.b[j - 1u]) << (8u * got++);
                    pos = sp[2 * q];
                    continue;
                }
                if (!pos) { acc |= (p.s.b.prev0 & 0xFFu) << (8u * got++); continue; }
                if (have != pos && have != pos + 1u) {                // x[pos - 1] from the source, x[pos - 2] with it
                    Chunk c;
                    if (!chunk_of<K, true>(p.s, (a >> cs) + i + (pos >> cs), c) || !c.entry_ok()) break;
                    two = splice_ctx_at<K>(p.s, dec, i, c, uint32_t(pos - c.first));
                    have = pos;
                }
                acc |= (have == pos ? two & 0xFFu : (two >> 8) & 0xFFu) << (8u * got++);
                --pos;
            }
            sctx[r] = acc;
        } else {
            if ((sp[2 * r + 1] >> cs) == (sp[2 * r] >> cs)) continue;     // no chunk starts in (begin, end]: no lane asks
            const uint64_t i = span_stream(off, n, r);
            if (p.s.b.stream_status[i] != MH_OK) continue;                // (a passed stream's tags are table entries)
            if (!rep_end<TABLE>(p, r).empty) continue;                    // replaced: its own last byte serves
            const uint64_t a = p.s.b.sym_off[i], ni = p.s.b.sym_off[i + 1] - a;
            if (sp[2 * r] >= ni) continue;                                // the span is ignored
            uint64_t r0 = r;
            uint32_t got = ~0u;
            while (r0 > off[i] && sp[2 * r0 - 1] == sp[2 * r0]) {         // the touching span in front: through it while it is empty
                const RepEnd front = rep_end<TABLE>(p, r0 - 1);
                if (!front.empty) { got = front.last(); break; }
                --r0;
            }
            if (got != ~0u) { sctx[r] = got; continue; }
            const uint64_t begin = sp[2 * r0];
            if (!begin) { sctx[r] = p.s.b.prev0; continue; }
            const uint64_t wb = (a >> cs) + i, pos = begin - 1u;
            if (!(begin & ((uint64_t(1) << cs) - 1u))) { sctx[r] = uint32_t(p.s.b.index[wb + (begin >> cs)] >> 56); continue; }
            Chunk c;
            if (!chunk_of<K, false>(p.s, wb + (pos >> cs), c) || !c.entry_ok()) continue;
            uint64_t bit0;
            const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[i], c.nb, bit0);
            BitCursor bc;
            bc.init(src, bit0 + c.start);
            dec.stream(p.s, i);
            uint32_t ctx = c.ctx, used = 0;
            bool bad = false;
            const uint32_t count = uint32_t(pos - c.first) + 1u;          // <= c.nsym: pos < ni
            for (uint32_t t = 0; t < count && !bad; ++t) {
                const uint32_t sym = dec.next(p.s, src, bc, ctx, used, bad);
                if (bad) break;
                ctx = sym;
            }
            sctx[r] = ctx;
        }
    }
}

template <Model K, bool DLDS, bool TABLE>
__global__ __launch_bounds__((Dec<K, SW<K>>::NT)) void splice_idx_len_kernel(SpParams<TABLE> p, uint64_t nwork, uint32_t lds_at,
                                                                           unsigned long long *cbits, unsigned long long *csyms, uint32_t *cdrop,
                                                                           const uint32_t *sctx, const uint32_t *price, int *status,
                                                                           const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K, SW<K>> dec(p.s, smem);
    const Enc<DLDS, SW<K>> E(p.dst, smem, lds_at);
    Cut<TABLE> cu(p);
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of<K, SW<K>>(p.s, w, c) || p.s.b.stream_status[c.i] == MH_ERR_ARG) continue;
        if (!c.entry_ok()) { stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        dec.stream(p.s, c.i);
        uint32_t ctx = c.ctx, used = 0, bits = 0, drops = 0, osym = 0;
        uint32_t dctx = splice_start<SW<K>>(cu, c, sctx);
        bool bad = false;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {
            const uint32_t sym = dec.next(p.s, src, bc, ctx, used, bad);
            if (bad) break;
            const bool coded = cu.step(t, [&] {
                if (!cu.rep_len) return;
                const uint32_t l = E.len(E.at(dctx, cu.rep[0]));     // rep[0] in dctx; the rest is priced
                bits += l + price[2 * cu.k];
                drops += (l == 0u) + price[2 * cu.k + 1u];
                if constexpr (SW<K>) {                                // rep[1] too: behind rep[0], one byte of dctx still counts
                    if (cu.rep_len >= 2u) {
                        const uint32_t l1 = E.len(E.at(roll<true>(dctx, cu.rep[0]), cu.rep[1]));
                        bits += l1;
                        drops += l1 == 0u;
                    }
                }
                osym += cu.rep_len;
                dctx = rep_ctx<SW<K>>(dctx, cu.rep, cu.rep_len);
            });
            if (coded) {
                const uint32_t l = E.len(E.at(dctx, sym));
                bits += l;
                drops += l == 0u;
                dctx = roll<SW<K>>(dctx, sym);
                ++osym;
            }
            ctx = roll<SW<K>>(ctx, sym);
        }
        if (bad || used != c.end - c.start) { stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        cbits[w] = bits;
        csyms[w] = osym;
        cdrop[w] = drops;
    }
}

// the chunks of failed streams count no bits and no output symbols; the dropped symbols of the others go to dropped[i]
__global__ __launch_bounds__(256) void splice_comb_kernel(SpliceParams p, uint64_t nwork, unsigned long long *cbits, unsigned long long *csyms,
                                                          const uint32_t *cdrop, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t w = gtid();
    if (w > nwork) return;
    unsigned long long v = 0, y = 0;
    if (w < nwork) {
        const uint32_t cs = p.s.b.chunk_shift;
        const uint64_t i = find_stream(p.s.b.sym_off, p.s.b.n, cs, w);
        if (i < p.s.b.n) {
            const uint64_t a = p.s.b.sym_off[i], ni = p.s.b.sym_off[i + 1] - a;
            const uint64_t k = w - ((a >> cs) + i);
            if ((k << cs) < ni && p.s.b.stream_status[i] == MH_OK) {
                v = cbits[w];
                y = csyms[w];
                const uint32_t d = cdrop[w];
                if (d && p.dropped) atomicAdd(&p.dropped[i], static_cast<unsigned long long>(d));
            }
        }
    }
    cbits[w] = v;
    csyms[w] = y;
}

// stream i: payload bits and bytes as recode_sizes_kernel; indexed: out_sym_off[i] is the scanned output symbols at the
// stream's first chunk number (gaps and failed streams count none)
__global__ __launch_bounds__(256) void splice_sizes_kernel(SpliceParams p, const unsigned long long *cbase, const unsigned long long *obase,
                                                           const int *stop) {
    if (mhb::stopped(stop)) return;
    const uint64_t i = mhb::gtid();
    const uint64_t n = p.s.b.n;
    if (i > n) return;
    if (p.s.b.index) p.sp.out_sym_off[i] = obase[(p.s.b.sym_off[i] >> p.s.b.chunk_shift) + i];
    if (i == n) { p.out_off[i] = 0; return; }
    unsigned long long bits;
    if (p.s.b.index) {
        const uint32_t cs = p.s.b.chunk_shift;
        const uint64_t w0 = (p.s.b.sym_off[i] >> cs) + i, w1 = (p.s.b.sym_off[i + 1] >> cs) + i + 1;
        bits = cbase[w1] - cbase[w0];
        p.out_nbits[i] = bits;
    } else {
        bits = p.out_nbits[i];
    }
    p.out_off[i] = (bits + 7) >> 3;
}

// the destination index has index_cap entries; the output needs (out_sym_off[n] >> cs) + n (after the scans: offsets and
// lengths are complete)
__global__ void splice_cap_kernel(SpliceParams p, int *status, int *stop) {
    if (mhb::stopped(stop)) return;
    if ((p.sp.out_sym_off[p.s.b.n] >> p.out_chunk_shift) + p.s.b.n > p.sp.index_cap) { mhb::fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
}

// One output symbol of a lane's emit pass: the index entry in front of it when its position o is a chunk's first, its code.
struct SpliceOut {
    unsigned long long *slice;          // the stream's slice of the destination index, or nullptr
    uint32_t ocs;
    uint64_t o, bit;                    // stream-relative output position and bit
    bool on;
    template <bool DLDS, bool W>
    __device__ __forceinline__ void put(const Enc<DLDS, W> &E, BitWriter &bw, uint32_t &dctx, uint32_t sym) {
        if (slice && (o & ((uint64_t(1) << ocs) - 1u)) == 0) slice[o >> ocs] = E.entry(dctx, bit);
        bit += E.put(bw, E.at(dctx, sym), on);
        dctx = roll<W>(dctx, sym);
        ++o;
    }
};

template <Model K, bool DLDS, bool TABLE>
__global__ __launch_bounds__((Dec<K, SW<K>>::NT)) void splice_idx_emit_kernel(SpParams<TABLE> p, uint64_t nwork, uint32_t lds_at,
                                                                            const unsigned long long *cbase, const unsigned long long *obase,
                                                                            const uint32_t *sctx, uint32_t *tail, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K, SW<K>> dec(p.s, smem);
    const Enc<DLDS, SW<K>> E(p.dst, smem, lds_at);
    Cut<TABLE> cu(p);
    const uint64_t bytes = p.out_off[p.s.b.n];
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint32_t cs = p.s.b.chunk_shift;
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of<K, SW<K>>(p.s, w, c) || p.s.b.stream_status[c.i] != MH_OK) continue;
        if (obase[w + 1] == obase[w]) continue;                                   // a lane that produces nothing writes nothing
        const uint64_t w0 = (p.s.b.sym_off[c.i] >> cs) + c.i;
        SpliceOut so;
        so.o = obase[w] - obase[w0];
        so.bit = cbase[w] - cbase[w0];
        so.ocs = cs;
        so.on = p.out != nullptr;
        so.slice = p.out_index ? p.out_index + (p.sp.out_sym_off[c.i] >> cs) + c.i : nullptr;
        uint32_t dctx = splice_start<SW<K>>(cu, c, sctx);
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        dec.stream(p.s, c.i);
        BitWriter bw;
        if (so.on) bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[c.i]) * 8u + so.bit);
        uint32_t ctx = c.ctx, used = 0;
        bool bad = false;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {            // (the stream passed: bad stays false)
            const uint32_t sym = dec.next(p.s, src, bc, ctx, used, bad);
            const bool coded = cu.step(t, [&] {
                for (uint32_t j = 0; j < cu.rep_len; ++j) so.put<DLDS>(E, bw, dctx, cu.rep[j]);
            });
            if (coded) so.put<DLDS>(E, bw, dctx, sym);
            ctx = roll<SW<K>>(ctx, sym);
        }
        if (so.on) bw.finish();
    }
}

// Index-free, one lane per stream (recode_walk_kernel).  EMIT = false: the verdict, the stream's symbols into sym_off[i] and
// its output symbols into out_sym_off[i] (both scanned next), its dst bits and dropped symbols; true: codes and index entries.
template <Model K, bool DLDS, bool EMIT, bool TABLE>
__global__ __launch_bounds__((Dec<K, SW<K>>::NT)) void splice_walk_kernel(SpParams<TABLE> p, uint32_t lds_at, uint32_t *tail, int *status,
                                                                        const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K, SW<K>> dec(p.s, smem);
    const Enc<DLDS, SW<K>> E(p.dst, smem, lds_at);
    Cut<TABLE> cu(p);
    const uint64_t n = p.s.b.n;
    const uint64_t bytes = EMIT ? p.out_off[n] : 0;
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    for (uint64_t i = gtid(); i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (p.s.b.stream_status[i] != MH_OK) continue;
        const uint64_t nb = p.s.b.nbits[i];
        uint64_t count = ~uint64_t(0);
        if (EMIT) {
            count = p.s.b.sym_off[i + 1] - p.s.b.sym_off[i];
            if (p.sp.out_sym_off[i + 1] == p.sp.out_sym_off[i]) continue;
        } else if (nb > p.s.b.walk_max_bits) {
            stream_fail(p.s.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
            continue;
        }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0);
        dec.stream(p.s, i);
        SpliceOut so;
        so.o = 0; so.bit = 0; so.ocs = p.out_chunk_shift;
        so.on = EMIT && p.out != nullptr;
        so.slice = EMIT && p.out_index ? p.out_index + (p.sp.out_sym_off[i] >> so.ocs) + i : nullptr;
        BitWriter bw;
        if (so.on) bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[i]) * 8u);
        uint32_t ctx = start_ctx<K, SW<K>>(p.s), used = 0, drops = 0;
        uint32_t dctx = ctx;
        cu.start(i);
        bool bad = false;
        uint64_t k = 0;
        auto one = [&](uint32_t s) {
            if (EMIT) {
                so.put<DLDS>(E, bw, dctx, s);
            } else {
                const uint32_t l = E.len(E.at(dctx, s));
                so.bit += l; drops += l == 0u; dctx = roll<SW<K>>(dctx, s); ++so.o;
            }
        };
        // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
        while (used < nb && !bad && k < count) {
            const uint32_t sym = dec.next(p.s, src, bc, ctx, used, bad);
            if (bad) break;
            const bool coded = cu.step(uint32_t(k), [&] {
                for (uint32_t j = 0; j < cu.rep_len; ++j) one(cu.rep[j]);
            });
            if (coded) one(sym);
            ctx = roll<SW<K>>(ctx, sym);
            ++k;
        }
        if (EMIT) { if (so.on) bw.finish(); continue; }
        if (bad || used != nb) { stream_fail(p.s.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        p.s.b.sym_off[i] = k;                                       // src/coding.cpp:158: the stream ends exactly at nbits
        p.sp.out_sym_off[i] = so.o;
        p.out_nbits[i] = so.bit;
        if (p.dropped) p.dropped[i] = drops;
    }
}

// span tags (mh_dev_spans_from_hits_tagged), behind spans_emit_kernel: num[r] is record r's span number when it starts a
// span, one more than it otherwise.  First the starting record's pattern by a plain store, then the minimum with the others'.
template <bool MIN>
__global__ __launch_bounds__(256) void spans_tag_kernel(SpanParams p, const uint32_t *pattern, uint32_t *span_tag, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t r = gtid();
    if (r >= p.hit_off[p.n]) return;
    const unsigned long long id = p.num[r];
    const bool start = p.num[r + 1] != id;
    if (!MIN) { if (start) span_tag[id] = pattern[r]; }
    else if (!start) atomicMin(&span_tag[id - 1], pattern[r]);
}

// ------------------------------------------------------------------------------------------------ launches

template <Model K, bool W>
hipError_t launch_hist(const HistParams &p, void *d_ws, hipStream_t st) {
    constexpr int NT = Dec<K, W>::NT, PER_CU = Dec<K, W>::PER_CU;
    constexpr bool LDS_TABLES = K == Model::Shared;
    const size_t lds_tables = LDS_TABLES ? mhb::tables_lds(p.s.b) : 0;
    if (lds_tables > size_t(LDS_MAX)) return hipErrorInvalidValue;
    // the counters take what the tables leave, 12 bytes a slot: 256 .. 4096 slots (tables in L2, eight workgroups per CU:
    // 1024), or none
    uint32_t log2n = 0;
    const size_t room = LDS_TABLES ? size_t(LDS_MAX) - lds_tables : size_t(12288);
    for (uint32_t k = 8; k <= 12; ++k)
        if ((size_t(12) << k) <= room) log2n = k;
    const size_t lds = lds_tables + (log2n ? size_t(12) << log2n : 0);
    const uint32_t lds_at = uint32_t(lds_tables);
    if (LDS_TABLES) {
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(histc_idx_kernel<K, W, false>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(histc_idx_kernel<K, W, true>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(histc_walk_kernel<K, W>), LDS_MAX);
        if (attr != hipSuccess) return attr;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.s.b.n;
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    const size_t ncounts = p.order == 2u ? (size_t(1) << 24) : (p.order ? 65536u : 256u);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e == hipSuccess) e = hipMemsetAsync(p.counts, 0, ncounts * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(histc_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p.s, status, stop);
    if (p.s.b.index) {
        const uint64_t nw = mhb::work_items(n, p.s.b.sym_total, 1u << p.s.b.chunk_shift);
        hipLaunchKernelGGL((histc_idx_kernel<K, W, false>), dim3(grid_for(nw, NT, PER_CU)), dim3(NT), lds, st, p, nw, lds_at, log2n, status, stop);
        hipLaunchKernelGGL((histc_idx_kernel<K, W, true>), dim3(grid_for(nw, NT, PER_CU)), dim3(NT), lds, st, p, nw, lds_at, log2n, status, stop);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((histc_walk_kernel<K, W>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, lds_at, log2n, status, stop);
    return hipGetLastError();
}

// EDIT: the map's 256 bytes of LDS lie behind everything the plain call lays out, which therefore stays where it is; when
// they do not fit (a source whose tables fill the LDS) the lanes read the map from L2
template <Model K, bool DLDS, bool W, bool EDIT = false>
hipError_t launch_rc(Params<EDIT> p, size_t lds_tables, void *d_ws, hipStream_t st) {
    constexpr int NT = Dec<K, W>::NT, PER_CU = Dec<K, W>::PER_CU;
    size_t lds = lds_tables + (DLDS ? (p.dst.ctx_mask ? 65536 : 256) : 0);
    const uint32_t lds_at = uint32_t(lds_tables);
    if constexpr (EDIT) {
        p.ed.map_lds = lds + 256 <= size_t(LDS_MAX) ? 1u : 0u;
        if (p.ed.map_lds) lds += 256;
    }
    if (K == Model::Shared) {
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(recode_idx_len_kernel<K, DLDS, W, EDIT>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(recode_idx_emit_kernel<K, DLDS, W, EDIT>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(recode_walk_kernel<K, DLDS, W, false, EDIT>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(recode_walk_kernel<K, DLDS, W, true, EDIT>), LDS_MAX);
        if (attr != hipSuccess) return attr;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.s.b.n;
    const uint64_t nw = p.s.b.index ? mhb::work_items(n, p.s.b.sym_total, 1u << p.s.b.chunk_shift) : 0;
    const RecodeLayout L = recode_layout(n, nw, SEAM<K, W>);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    uint32_t *tail = reinterpret_cast<uint32_t *>(ws + TAIL_AT);
    auto *cbits = reinterpret_cast<unsigned long long *>(ws + L.off_bits);
    auto *cdrop = reinterpret_cast<uint32_t *>(ws + L.off_drop);
    uint32_t *chead = SEAM<K, W> ? reinterpret_cast<uint32_t *>(ws + L.off_head) : nullptr;
    uint32_t *cclose = SEAM<K, W> ? reinterpret_cast<uint32_t *>(ws + L.off_close) : nullptr;
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e == hipSuccess && nw) e = hipMemsetAsync(ws + L.off_bits, 0, L.off_sums - L.off_bits, st);   // chunk bits, dropped counts, heads
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(recode_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, status, stop);
    if constexpr (EDIT) {
        if (p.ed.span_off) hipLaunchKernelGGL(recode_spans_kernel, dim3(grid_for(uint64_t(1) << 40, 256, 8)), dim3(256), 0, st, p, status, stop);
    }
    if (p.s.b.index) {
        hipLaunchKernelGGL((recode_idx_len_kernel<K, DLDS, W, EDIT>), dim3(grid_for(nw, NT, PER_CU)), dim3(NT), lds, st, p, nw, lds_at, cbits, cdrop,
                           chead, cclose, status, stop);
        hipLaunchKernelGGL((recode_comb_kernel<SEAM<K, W>>), grid_threads(nw + 1, 256), dim3(256), 0, st, p, nw, cbits, cdrop, chead, stop);
        if ((e = scan_exclusive(cbits, nw + 1, sums, stop, st)) != hipSuccess) return e;
    } else {
        hipLaunchKernelGGL((recode_walk_kernel<K, DLDS, W, false, EDIT>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, lds_at, tail,
                           status, stop);
        if ((e = scan_exclusive(p.s.b.sym_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(recode_sizes_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, cbits, stop);
    if ((e = scan_exclusive(p.out_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    if (!p.s.b.index && p.out_index) hipLaunchKernelGGL(recode_cap_kernel, dim3(1), dim3(1), 0, st, p, status, stop);
    if (p.out) hipLaunchKernelGGL(recode_zero_kernel, dim3(grid_for(p.cap / 4 + 1, 256, 8)), dim3(256), 0, st, p, status, stop, tail);
    if (p.s.b.index) {
        if (p.out || p.out_index)
            hipLaunchKernelGGL((recode_idx_emit_kernel<K, DLDS, W, EDIT>), dim3(grid_for(nw, NT, PER_CU)), dim3(NT), lds, st, p, nw, lds_at, cbits,
                               chead, cclose, tail, stop);
    } else if (p.out || p.out_index) {
        hipLaunchKernelGGL((recode_walk_kernel<K, DLDS, W, true, EDIT>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, lds_at, tail,
                           status, stop);
    }
    if (p.out) hipLaunchKernelGGL(recode_tail_kernel, dim3(1), dim3(1), 0, st, p, tail, stop);
    return hipGetLastError();
}

// the splice: no LDS beyond the tables and the destination's image.  TABLE: the look-back pre-pass runs on every indexed
// call, so the launches depend on indexed versus index-free alone; !TABLE: it runs when rep_len == 0.
template <Model K, bool DLDS, bool TABLE>
hipError_t launch_sp(SpParams<TABLE> p, size_t lds_tables, void *d_ws, size_t ws_bytes, hipStream_t st) {
    constexpr int NT = Dec<K, SW<K>>::NT, PER_CU = Dec<K, SW<K>>::PER_CU;
    const size_t lds = lds_tables + (DLDS ? (p.dst.ctx_mask ? 65536 : 256) : 0);
    const uint32_t lds_at = uint32_t(lds_tables);
    if (K == Model::Shared) {
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(splice_idx_len_kernel<K, DLDS, TABLE>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(splice_idx_emit_kernel<K, DLDS, TABLE>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(splice_walk_kernel<K, DLDS, false, TABLE>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(splice_walk_kernel<K, DLDS, true, TABLE>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(splice_back_kernel<K, TABLE>), LDS_MAX);
        if (attr != hipSuccess) return attr;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.s.b.n;
    const uint64_t nw = p.s.b.index ? mhb::work_items(n, p.s.b.sym_total, 1u << p.s.b.chunk_shift) : 0;
    uint64_t nr = 1;                                                  // table entries: price[2k], price[2k + 1]
    if constexpr (TABLE) nr = p.tb.n_reps;
    const SpliceLayout L = splice_table_layout(n, nw, 0, nr);         // (one entry lays out as splice_layout)
    p.sp.span_cap = (ws_bytes - L.off_sctx) / 4;
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    uint32_t *tail = reinterpret_cast<uint32_t *>(ws + TAIL_AT);
    auto *cbits = reinterpret_cast<unsigned long long *>(ws + L.off_bits);
    auto *csyms = reinterpret_cast<unsigned long long *>(ws + L.off_syms);
    auto *cdrop = reinterpret_cast<uint32_t *>(ws + L.off_drop);
    auto *price = reinterpret_cast<uint32_t *>(ws + L.off_price);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    auto *sctx = reinterpret_cast<uint32_t *>(ws + L.off_sctx);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e == hipSuccess && nw) e = hipMemsetAsync(ws + L.off_bits, 0, L.off_price - L.off_bits, st);   // chunk bits, output symbols, dropped counts
    if (e != hipSuccess) return e;
    const dim3 span_grid(grid_for(uint64_t(1) << 40, 256, 8));
    hipLaunchKernelGGL(splice_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, status, stop);
    if constexpr (!TABLE) hipLaunchKernelGGL(recode_spans_kernel, span_grid, dim3(256), 0, st, spans_view(p), status, stop);
    hipLaunchKernelGGL((splice_price_kernel<TABLE, SW<K>>), dim3(uint32_t(nr < 1 ? 1 : (nr > 65536 ? 65536 : nr))), dim3(256), 0, st, p, price, status, stop);
    if constexpr (TABLE) hipLaunchKernelGGL(splice_spans_kernel, span_grid, dim3(256), 0, st, p, status, stop);   // (behind the table's checks)
    if (p.s.b.index) {
        if (TABLE || !p.sp.rep_len)
            hipLaunchKernelGGL((splice_back_kernel<K, TABLE>), dim3(grid_for(uint64_t(1) << 40, NT, PER_CU)), dim3(NT), lds_tables, st, p, sctx, status,
                               stop);
        hipLaunchKernelGGL((splice_idx_len_kernel<K, DLDS, TABLE>), dim3(grid_for(nw, NT, PER_CU)), dim3(NT), lds, st, p, nw, lds_at, cbits, csyms,
                           cdrop, sctx, price, status, stop);
        hipLaunchKernelGGL(splice_comb_kernel, grid_threads(nw + 1, 256), dim3(256), 0, st, p, nw, cbits, csyms, cdrop, stop);
        if ((e = scan_exclusive(cbits, nw + 1, sums, stop, st)) != hipSuccess) return e;
        if ((e = scan_exclusive(csyms, nw + 1, sums, stop, st)) != hipSuccess) return e;
    } else {
        hipLaunchKernelGGL((splice_walk_kernel<K, DLDS, false, TABLE>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, lds_at, tail, status,
                           stop);
        if ((e = scan_exclusive(p.s.b.sym_off, n + 1, sums, stop, st)) != hipSuccess) return e;
        if ((e = scan_exclusive(p.sp.out_sym_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(splice_sizes_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, cbits, csyms, stop);
    if ((e = scan_exclusive(p.out_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    if (p.out_index) hipLaunchKernelGGL(splice_cap_kernel, dim3(1), dim3(1), 0, st, p, status, stop);
    if (p.out) hipLaunchKernelGGL(recode_zero_kernel, dim3(grid_for(p.cap / 4 + 1, 256, 8)), dim3(256), 0, st, p, status, stop, tail);
    if (p.s.b.index) {
        if (p.out || p.out_index)
            hipLaunchKernelGGL((splice_idx_emit_kernel<K, DLDS, TABLE>), dim3(grid_for(nw, NT, PER_CU)), dim3(NT), lds, st, p, nw, lds_at, cbits, csyms,
                               sctx, tail, stop);
    } else if (p.out || p.out_index) {
        hipLaunchKernelGGL((splice_walk_kernel<K, DLDS, true, TABLE>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, lds_at, tail, status,
                           stop);
    }
    if (p.out) hipLaunchKernelGGL(recode_tail_kernel, dim3(1), dim3(1), 0, st, p, tail, stop);
    return hipGetLastError();
}

// the branches of launch_recode_edit, each with the splice in place of the edit
template <bool TABLE>
hipError_t launch_splice(const SpParams<TABLE> &p, Model model, void *d_ws, size_t ws_bytes, hipStream_t st) {
    if (model == Model::Shared2) {                                    // any destination; tables in L2, no image in LDS
        if constexpr (TABLE) return launch_sp<Model::Shared2, false, true>(p, 0, d_ws, ws_bytes, st);
        else return hipErrorInvalidValue;
    }
    if (p.dst.ctx_mask == 0xFFFFu) return hipErrorInvalidValue;
    if (model == Model::Set)
        return p.dst.ctx_mask ? launch_sp<Model::Set, false, TABLE>(p, 0, d_ws, ws_bytes, st)
                              : launch_sp<Model::Set, true, TABLE>(p, 0, d_ws, ws_bytes, st);
    const size_t lds = mhb::tables_lds(p.s.b);
    if (lds > size_t(LDS_MAX)) return hipErrorInvalidValue;
    const size_t img = p.dst.ctx_mask ? 65536 : 256;
    return lds + img <= size_t(LDS_MAX) ? launch_sp<Model::Shared, true, TABLE>(p, lds, d_ws, ws_bytes, st)
                                        : launch_sp<Model::Shared, false, TABLE>(p, lds, d_ws, ws_bytes, st);
}

}  // namespace

hipError_t launch_recode_splice_table(const SpliceTableParams &p, Model model, void *d_ws, size_t ws_bytes, hipStream_t st) {
    return launch_splice<true>(p, model, d_ws, ws_bytes, st);
}

hipError_t launch_recode_splice(const SpliceParams &p, Model model, void *d_ws, size_t ws_bytes, hipStream_t st) {
    return launch_splice<false>(p, model, d_ws, ws_bytes, st);
}

hipError_t launch_histogram_coded(const HistParams &p, Model model, void *d_ws, hipStream_t st) {
    if (model == Model::Shared2) return launch_hist<Model::Shared2, true>(p, d_ws, st);
    if (model == Model::Set) return p.order == 2u ? hipErrorInvalidValue : launch_hist<Model::Set, false>(p, d_ws, st);
    return p.order == 2u ? launch_hist<Model::Shared, true>(p, d_ws, st) : launch_hist<Model::Shared, false>(p, d_ws, st);
}

hipError_t launch_recode(const RecodeParams &p, Model model, void *d_ws, hipStream_t st) {
    const bool dst2 = p.dst.ctx_mask == 0xFFFFu;
    // tables in L2 and eight workgroups to a CU: of the destination only an order-0 image (256 B) goes to LDS, and that
    // under a model set alone
    if (model == Model::Shared2) return launch_rc<Model::Shared2, false, true>(p, 0, d_ws, st);
    if (model == Model::Set) {
        if (dst2) return hipErrorInvalidValue;
        return p.dst.ctx_mask ? launch_rc<Model::Set, false, false>(p, 0, d_ws, st) : launch_rc<Model::Set, true, false>(p, 0, d_ws, st);
    }
    const size_t lds = mhb::tables_lds(p.s.b);
    if (lds > size_t(LDS_MAX)) return hipErrorInvalidValue;
    if (dst2) return launch_rc<Model::Shared, false, true>(p, lds, d_ws, st);
    const size_t img = p.dst.ctx_mask ? 65536 : 256;
    return lds + img <= size_t(LDS_MAX) ? launch_rc<Model::Shared, true, false>(p, lds, d_ws, st)
                                        : launch_rc<Model::Shared, false, false>(p, lds, d_ws, st);
}

// the branches of launch_recode, each with the edit
hipError_t launch_recode_edit(const EditParams &p, Model model, void *d_ws, hipStream_t st) {
    const bool dst2 = p.dst.ctx_mask == 0xFFFFu;
    if (model == Model::Shared2) return launch_rc<Model::Shared2, false, true, true>(p, 0, d_ws, st);
    if (model == Model::Set && dst2) return hipErrorInvalidValue;
    if (model == Model::Set)
        return p.dst.ctx_mask ? launch_rc<Model::Set, false, false, true>(p, 0, d_ws, st) : launch_rc<Model::Set, true, false, true>(p, 0, d_ws, st);
    const size_t lds = mhb::tables_lds(p.s.b);
    if (lds > size_t(LDS_MAX)) return hipErrorInvalidValue;
    if (dst2) return launch_rc<Model::Shared, false, true, true>(p, lds, d_ws, st);
    const size_t img = p.dst.ctx_mask ? 65536 : 256;
    return lds + img <= size_t(LDS_MAX) ? launch_rc<Model::Shared, true, false, true>(p, lds, d_ws, st)
                                        : launch_rc<Model::Shared, false, false, true>(p, lds, d_ws, st);
}

hipError_t launch_spans_from_hits(const unsigned long long *hit_off, const unsigned long long *hits, uint64_t hit_cap, uint64_t n_streams,
                                  unsigned long long *span_off, unsigned long long *spans, void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const SpanLayout L = span_layout(hit_cap);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    SpanParams p{hit_off, hits, hit_cap, n_streams, span_off, spans, reinterpret_cast<unsigned long long *>(ws + L.off_min),
                 reinterpret_cast<unsigned long long *>(ws + L.off_num), reinterpret_cast<unsigned long long *>(ws + L.off_tile)};
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    const uint64_t tiles = (hit_cap + SPAN_TILE - 1) / SPAN_TILE;
    hipLaunchKernelGGL(spans_front_kernel, grid_threads(n_streams + 1, 256), dim3(256), 0, st, p, status, stop);
    if (tiles) hipLaunchKernelGGL(spans_tile_kernel, dim3(uint32_t(tiles)), dim3(SPAN_TILE), 0, st, p, status, stop);
    if (tiles) hipLaunchKernelGGL(spans_carry_kernel, dim3(1), dim3(1), 0, st, p, stop);
    hipLaunchKernelGGL(spans_mark_kernel, grid_threads(hit_cap + 2, 256), dim3(256), 0, st, p, stop);
    if ((e = scan_exclusive(p.num, hit_cap + 2, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(spans_emit_kernel, grid_threads((hit_cap > n_streams ? hit_cap : n_streams) + 1, 256), dim3(256), 0, st, p, stop);
    return hipGetLastError();
}

// the untagged launches, then two more over the records (the numbers stay in the workspace)
hipError_t launch_spans_from_hits_tagged(const unsigned long long *hit_off, const unsigned long long *hits, const uint32_t *hit_pattern,
                                         uint64_t hit_cap, uint64_t n_streams, unsigned long long *span_off, unsigned long long *spans,
                                         uint32_t *span_tag, void *d_ws, hipStream_t st) {
    const hipError_t e = launch_spans_from_hits(hit_off, hits, hit_cap, n_streams, span_off, spans, d_ws, st);
    if (e != hipSuccess || !hit_cap) return e;
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const SpanLayout L = span_layout(hit_cap);
    int *stop = reinterpret_cast<int *>(ws) + 1;
    SpanParams p{hit_off, hits, hit_cap, n_streams, span_off, spans, reinterpret_cast<unsigned long long *>(ws + L.off_min),
                 reinterpret_cast<unsigned long long *>(ws + L.off_num), reinterpret_cast<unsigned long long *>(ws + L.off_tile)};
    hipLaunchKernelGGL(spans_tag_kernel<false>, grid_threads(hit_cap, 256), dim3(256), 0, st, p, hit_pattern, span_tag, stop);
    hipLaunchKernelGGL(spans_tag_kernel<true>, grid_threads(hit_cap, 256), dim3(256), 0, st, p, hit_pattern, span_tag, stop);
    return hipGetLastError();
}

}  // namespace mhr
