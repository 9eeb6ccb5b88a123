// mh_recode.h — launch interface between the re-coding calls of the C ABI (mh_api_recode.cpp) and their kernels
// (mh_recode.hip): the context histogram of a compressed batch and the batch coded again under another model, both taken
// from the decoded symbols while they sit in a register (include/mh.h, "RE-CODING BATCHES" and the re-coding part of "ORDER 2
// IN SEARCH AND RE-CODING").  The batch layouts (packed
// payloads, closed-form index slices) are those of mh_batch.h; the per-stream models those of mh_each.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"
#include "mh_each.h"

namespace mhr {

// the source: the batch and, under a shared model, its decode tables (out / out_cap unused); the models under a set
struct Src {
    mhb::DecBatchParams b;
    mhe::SetDev set;
};

// the destination model's encoder tables at (ctx & ctx_mask) << 8 | sym: order 2 keeps both context bytes (0xFFFF) and may
// have the packed table enc64 (len << 56 | code; len 255: longer than 56 bits, read len8 / code64), order 1 the last byte
// (0xFF), order 0 none (0: row 0 serves every context)
struct Dst {
    const uint8_t *len8;
    const unsigned long long *code64;
    const unsigned long long *enc64;    // order 2 only, may be nullptr
    uint32_t ctx_mask;
};

// histogram workspace: status block | per-stream status (when the caller passes none)
struct HistLayout {
    size_t off_status, total;
};
inline HistLayout hist_layout(uint64_t n_streams) {
    HistLayout l;
    l.off_status = 64;
    l.total = (l.off_status + size_t(n_streams) * 4 + 255) & ~size_t(255);
    return l;
}

// re-code workspace: status block (status, stop, -, -, tail word) | per-stream status (when the caller passes none) | per
// chunk number: destination bits (u64, W + 1, scanned in place), dropped symbols (u32) and, with seam (an order-0/1 batch
// coded under order-2 contexts, mh_recode.hip), head bits (u32: the next chunk's first symbol under dst) and closing context
// (u32: the chunk's last two symbols) | scan block sums
struct RecodeLayout {
    size_t off_status, off_bits, off_drop, off_head, off_close, off_sums, total;
};
constexpr size_t TAIL_AT = 16;
inline RecodeLayout recode_layout(uint64_t n_streams, uint64_t nwork, bool seam) {
    RecodeLayout l;
    const uint64_t len = (nwork > n_streams ? nwork : n_streams) + 1;
    l.off_status = 64;
    l.off_bits = (l.off_status + size_t(n_streams) * 4 + 15) & ~size_t(15);
    l.off_drop = l.off_bits + size_t(nwork + 1) * 8;
    l.off_head = l.off_drop + size_t(nwork) * 4;
    l.off_close = l.off_head + (seam ? size_t(nwork) * 4 : 0);
    l.off_sums = (l.off_close + (seam ? size_t(nwork) * 4 : 0) + 15) & ~size_t(15);
    l.total = (l.off_sums + size_t(mhb::scan_blocks(len) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

struct HistParams {
    Src s;
    uint32_t order;                 // of the histogram: 0 (256 counts), 1 (65 536) or 2 (1 << 24)
    unsigned long long *counts;
};

// the source and the outputs: the kernels that never decode take this part alone
struct RecodeIO {
    Src s;                          // index-free: s.b.sym_off is written, s.b.index null
    uint8_t *out;                   // packed payloads, 16-byte aligned; nullptr: count only
    uint64_t cap;
    unsigned long long *out_off;    // n + 1 (written)
    unsigned long long *out_nbits;  // n (written)
    unsigned long long *out_index;  // slices of the destination index in dst's entry format, or nullptr
    unsigned long long *dropped;    // n, or nullptr
    uint32_t out_chunk_shift;       // chunk of the destination index (indexed source: the source's)
};

struct RecodeParams : RecodeIO {
    Dst dst;
};

// the edit of a masked re-code (include/mh.h, "EDITING BATCHES"): inside stream i's spans [span_off[i], span_off[i + 1]) of
// (begin, end) pairs, byte b of the decoded message is coded as map[b]
struct Edit {
    const unsigned long long *span_off;   // n + 1, or nullptr: every byte of every stream is inside
    const unsigned long long *spans;
    const uint8_t *map;                   // 256 bytes
    uint32_t map_lds;                     // set by the launcher: the map has its 256 bytes of LDS behind the tables
};

struct EditParams : RecodeParams {
    Edit ed;
};

// the splice of a splicing re-code (include/mh.h, "SPLICING BATCHES"): every span of stream i that begins inside the decoded
// message is replaced by the rep_len bytes of rep (0: deleted), so the output has its own lengths, out_sym_off, and its index
// is laid out by output positions.  One kernel family serves this call and the table's (mh_recode.hip, TABLE): rep and rep_len
// are read by the single-replacement call alone (!TABLE), every other field by both
struct Splice {
    const unsigned long long *span_off;   // n + 1
    const unsigned long long *spans;
    const uint8_t *rep;                   // !TABLE: rep_len bytes (may be nullptr when 0)
    uint32_t rep_len;                     // !TABLE: 0 .. MH_SPLICE_MAX_REP
    uint64_t span_cap;                    // set by the launcher: the spans the workspace has room for (!TABLE: used when rep_len == 0)
    unsigned long long *out_sym_off;      // n + 1 (written): the exclusive scan of the output lengths
    uint64_t index_cap;                   // entries of out_index
};

struct SpliceParams : RecodeParams {
    Splice sp;
};

// splice workspace: status block | per-stream status | per chunk number: destination bits (u64, W + 1, scanned in place),
// output symbols (u64, W + 1, scanned in place), dropped symbols (u32) | the bits and drops of rep[1..] (2 x u32) | scan
// block sums | per span: the destination context behind a deleted span (u32; written and read only when rep_len == 0; an
// order-2 source: the last two output bytes behind a replacement shorter than two bytes).  The
// spans come last: the call is not told their number, it takes what ws_bytes leaves behind off_sctx as its room
struct SpliceLayout {
    size_t off_status, off_bits, off_syms, off_drop, off_price, off_sums, off_sctx, total;
};
inline SpliceLayout splice_layout(uint64_t n_streams, uint64_t nwork, uint64_t n_spans) {
    SpliceLayout l;
    const uint64_t len = (nwork > n_streams ? nwork : n_streams) + 1;
    l.off_status = 64;
    l.off_bits = (l.off_status + size_t(n_streams) * 4 + 15) & ~size_t(15);
    l.off_syms = l.off_bits + size_t(nwork + 1) * 8;
    l.off_drop = l.off_syms + size_t(nwork + 1) * 8;
    l.off_price = l.off_drop + size_t(nwork) * 4;
    l.off_sums = (l.off_price + 8 + 15) & ~size_t(15);
    l.off_sctx = l.off_sums + size_t(mhb::scan_blocks(len) + 1) * 8;
    l.total = (l.off_sctx + size_t(n_spans) * 4 + 255) & ~size_t(255);
    return l;
}

// the table of a table splice (include/mh.h, "SPLICING WITH A REPLACEMENT TABLE"): span r is replaced by entry span_tag[r],
// the bytes rep_bytes[rep_off[k] .. rep_off[k + 1]).  Read under TABLE alone, where sp.rep / sp.rep_len are unused; the
// single-replacement kernels take SpliceParams and carry none of this in their argument block
struct SpliceTable {
    const uint32_t *span_tag;             // one per span
    const unsigned long long *rep_off;    // n_reps + 1
    const uint8_t *rep_bytes;
    uint64_t n_reps;
};

struct SpliceTableParams : SpliceParams {
    SpliceTable tb;
};

// table splice workspace: the splice's, with the bits and drops of rep_k[1..] per table entry (2 x u32 each; one entry's
// room at least, so a one-entry table lays out as the single replacement does)
inline SpliceLayout splice_table_layout(uint64_t n_streams, uint64_t nwork, uint64_t n_spans, uint64_t n_reps) {
    SpliceLayout l = splice_layout(n_streams, nwork, 0);
    const uint64_t len = (nwork > n_streams ? nwork : n_streams) + 1;
    l.off_sums = (l.off_price + size_t(n_reps ? n_reps : 1) * 8 + 15) & ~size_t(15);
    l.off_sctx = l.off_sums + size_t(mhb::scan_blocks(len) + 1) * 8;
    l.total = (l.off_sctx + size_t(n_spans) * 4 + 255) & ~size_t(255);
    return l;
}

// spans from search records: status block | per record: the reverse min-scan of the begins (u64), span starts and, scanned in
// place, span numbers (u64, cap + 2) | per tile of SPAN_TILE records: first stream, last stream, the first record's scan
// value, the carry from the tiles behind | scan block sums | per stream: nothing beyond the offsets the caller passes
struct SpanLayout {
    size_t off_min, off_num, off_tile, off_sums, total;
};
constexpr uint32_t SPAN_TILE = 256;
inline SpanLayout span_layout(uint64_t hit_cap) {
    SpanLayout l;
    const uint64_t tiles = (hit_cap + SPAN_TILE - 1) / SPAN_TILE;
    l.off_min = 64;
    l.off_num = l.off_min + size_t(hit_cap) * 8;
    l.off_tile = l.off_num + size_t(hit_cap + 2) * 8;
    l.off_sums = l.off_tile + size_t(tiles) * 32;
    l.total = (l.off_sums + size_t(mhb::scan_blocks(hit_cap + 2) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

// model: what the batch was coded under (mhb::Model, mh_batch.h); s.b's tables and s.b.prev0 as that model's batch decoder
// takes them.  Any order of the histogram or of dst under a shared model; a model set with an order-2 side is refused.
hipError_t launch_histogram_coded(const HistParams &p, mhb::Model model, void *d_ws, hipStream_t st);
hipError_t launch_recode(const RecodeParams &p, mhb::Model model, void *d_ws, hipStream_t st);
// the same with the edit applied, any orders under a shared model (include/mh.h, "ORDER 2 IN EDITING AND SPLICING": an order-2
// side takes the workspace of recode_layout(…, seam = true)); a model set with an order-2 destination is refused
hipError_t launch_recode_edit(const EditParams &p, mhb::Model model, void *d_ws, hipStream_t st);
// the splice in place of the edit; order 0/1 on both sides, p.sp.span_off not null
hipError_t launch_recode_splice(const SpliceParams &p, mhb::Model model, void *d_ws, size_t ws_bytes, hipStream_t st);
// the table splice: a replacement per span, insertions (begin == end) legal; order 0/1 on both sides, or an order-2 source
// (Shared2) under any destination, on the same workspace layout: sctx[r] then holds two bytes.  An order-0/1 source under an
// order-2 destination is refused
hipError_t launch_recode_splice_table(const SpliceTableParams &p, mhb::Model model, void *d_ws, size_t ws_bytes, hipStream_t st);
// the records of a find call (ascending (stream, end, pattern)) merged into maximal spans; a total over hit_cap: the status
// word is MHK_STATUS_CAPACITY, span_off all zeros
hipError_t launch_spans_from_hits(const unsigned long long *hit_off, const unsigned long long *hits, uint64_t hit_cap, uint64_t n_streams,
                                  unsigned long long *span_off, unsigned long long *spans, void *d_ws, hipStream_t st);
// the same, and span_tag[r]: the lowest hit_pattern among the records merged into span r
hipError_t launch_spans_from_hits_tagged(const unsigned long long *hit_off, const unsigned long long *hits, const uint32_t *hit_pattern,
                                         uint64_t hit_cap, uint64_t n_streams, unsigned long long *span_off, unsigned long long *spans,
                                         uint32_t *span_tag, void *d_ws, hipStream_t st);

}  // namespace mhr
