// mh_batch_states.hip — segment states of a batch of index-free streams of order 0, 1 or 2 (include/mh.h, "SEGMENT STATES OF
// INDEX-FREE BATCHES" and "SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES").  Every stream's payload is cut into SEG_BITS-bit segments, numbered in closed form
// (mh_batch_states.h); a segment owns the symbols whose code starts inside it.  One lane decodes one segment.
//   bseg_check_kernel    offsets non-decreasing, [0] == 0, [n] == pay_total (else MH_ERR_ARG for the call); per stream
//                        MH_ERR_ARG when nbits_i lies beyond its payload bytes
//   bseg_spec_kernel     segment 0 from (prev0, 0); every other one from a guess: WARMUP_BITS of its predecessor's bits
//                        decoded from context prev0 first (Huffman streams re-synchronise); order 2: the whole predecessor
//                        from (prev0, prev0), recovering from contexts without codes (Shared2D::warmup)
//   bseg_repair_kernel   REPAIR_PASSES launches over ping-pong record buffers: a segment whose entry differs from its
//                        predecessor's end (both read from the buffer the previous launch wrote) is decoded again from that
//                        end; a pass returns at once when the one before changed nothing
//   bseg_mark_kernel     first and last inconsistent segment of every stream
//   bseg_walk_kernel     one lane per stream that still has one: a sequential walk from its first inconsistent segment
//                        until its state meets a recorded entry behind which every segment is consistent; a walk longer
//                        than walk_max_bits refuses the stream (MH_ERR_ARG) — fixed-length-code lattices never re-synchronise;
//                        every walked stream is counted in the header (mh_dev_batch_states_stats)
//   bseg_proof_kernel    entry(k) == end(k - 1), entry(0) == (prev0, 0), no null table entry on the path, the last segment
//                        ends exactly at nbits_i (src/coding.cpp:124,158): by induction the records are the true states;
//                        a stream that fails is MH_ERR_CORRUPT
//   bseg_count_kernel, batch_scan_*, bseg_finish_kernel    symbol counts -> exclusive scan -> sym_off, statuses, the tag
//   bseg_gate_kernel     index / emit: the workspace holds states of this batch (else MH_ERR_ARG), the index fits
//   bseg_index_kernel    one lane per segment with a chunk boundary: decodes from its settled entry up to its last boundary
//   bseg_emit_kernel     one lane per segment: its symbols through ByteOut
// Every record a launch reads was written entirely by an earlier launch; within a launch a record is written by the one
// lane that decoded it (the torn-record race of the single-stream builder cannot occur).  The number of launches does not
// depend on the data and nothing synchronises the host.
// The decoder is a policy (SharedD, SetD, Shared2D): it steps one symbol from a context to the next one and names the state
// format (context << SHIFT | position, POS masks the position) and the byte a context ends in.
#include "mh_batch_states.h"
#include "mh_batch_dev.hpp"
#include "mh_decode_dev.hpp"
#include "mh_dev.hpp"
#include "mh_each_dev.hpp"
#include "../../include/mh.h"

namespace mhs {

using mhb::fail;
using mhb::find_stream;
using mhb::gtid;
using mhb::stopped;
using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;

namespace {

// decoder of the shared model: tables in LDS (the batch decoder's layout)
struct SharedD {
    static constexpr uint32_t SHIFT = 56;
    static constexpr unsigned long long POS = MH_INDEX_BIT_MASK;
    static constexpr bool RECOVER = false;
    static __device__ __forceinline__ uint32_t byte(uint32_t ctx) { return ctx; }
    const uint16_t *lut;
    const uint32_t *sub_base;
    DecTables tabs;
    __device__ __forceinline__ void setup(const StParams &p, unsigned char *smem) { tabs = mhb::load_tables(p.tabs, smem, lut, sub_base); }
    __device__ __forceinline__ void select(const StParams &, uint64_t) {}
    __device__ __forceinline__ uint32_t step(const BitSrc &src, BitCursor &bc, uint32_t prev, uint32_t &used, bool &bad) const {
        return mhk::decode_one(lut, sub_base, tabs, src, bc, prev, used, bad);
    }
};

// decoder of a model set: stream i's first level and walk tree (L2)
struct SetD {
    static constexpr uint32_t SHIFT = 56;
    static constexpr unsigned long long POS = MH_INDEX_BIT_MASK;
    static constexpr bool RECOVER = false;
    static __device__ __forceinline__ uint32_t byte(uint32_t ctx) { return ctx; }
    mhe::SetDev s;
    const uint32_t *row;
    bool o1;
    __device__ __forceinline__ void setup(const StParams &p, unsigned char *) { s = p.set; }
    __device__ __forceinline__ void select(const StParams &p, uint64_t i) {
        row = p.set.ctx_slot + i * 256u;
        o1 = p.set.type[i] != 0;
    }
    __device__ __forceinline__ uint32_t step(const BitSrc &src, BitCursor &bc, uint32_t prev, uint32_t &used, bool &bad) const {
        return mhe::decode_sym(s, row, o1 ? prev : 0u, src, bc, used, bad);
    }
};

// decoder of the shared order-2 model: the general form, every level gathered from L2 (dec_idx_kernel<Shared2>'s reads); the
// context holds the last two symbols
struct Shared2D {
    static constexpr uint32_t SHIFT = 48;
    static constexpr unsigned long long POS = MH_INDEX2_BIT_MASK;
    static constexpr bool RECOVER = true;
    static __device__ __forceinline__ uint32_t byte(uint32_t ctx) { return ctx & 0xFFu; }
    const uint16_t *prim;
    const uint32_t *sec_base;
    DecTables tabs;
    const uint16_t *rep;
    const uint32_t *live;
    __device__ __forceinline__ void setup(const StParams &p, unsigned char *) {
        prim = p.tabs.prim; sec_base = p.tabs.sec_base; rep = p.rep; live = p.live;
        tabs = DecTables{p.tabs.sec, p.tabs.tree, p.tabs.P, 0u, 0u};
    }
    __device__ __forceinline__ void select(const StParams &, uint64_t) {}
    __device__ __forceinline__ uint32_t step(const BitSrc &src, BitCursor &bc, uint32_t ctx, uint32_t &used, bool &bad) const {
        const uint32_t sym = mhk::decode_one(prim, sec_base, tabs, src, bc, ctx, used, bad);
        return ((ctx << 8) | sym) & 0xFFFFu;
    }
    // The entry guess of the segment that starts at bit `at`: the bits [from, at) decoded from the start context.  Most of the
    // 65536 contexts have no codes, and a guessed context runs into one almost at once; the warm-up then goes on
    //   - in rep[b], the heaviest live context that ends in the current context's last byte b, at the same bit, or
    //   - where there is none, in the start context one bit further;
    //   - a live context whose codes the bits do not match (one symbol, the end of the payload) keeps the context and skips a bit.
    // Every round consumes a bit or moves to a live context, whose round consumes one.  (A failed step leaves the cursor
    // anywhere: it is set up again.)
    __device__ unsigned long long warmup(const BitSrc &src, uint64_t bit0, unsigned long long state0, uint64_t from, uint64_t at) const {
        const uint32_t ctx0 = uint32_t(state0 >> SHIFT);
        uint32_t ctx = ctx0;
        uint64_t pos = from;
        BitCursor bc;
        bc.init(src, bit0 + pos);
        while (pos < at) {
            uint32_t used = 0;
            bool bad = false;
            const uint32_t next = step(src, bc, ctx, used, bad);
            if (!bad) { ctx = next; pos += used; continue; }
            if ((live[ctx >> 5] >> (ctx & 31u)) & 1u) ++pos;
            else {
                const uint32_t r = rep[ctx & 0xFFu];
                if (r != 0xFFFFu && r != ctx) ctx = r;
                else { ctx = ctx0; ++pos; }
            }
            bc.init(src, bit0 + pos);
        }
        return ((unsigned long long)ctx << SHIFT) | pos;
    }
};

__device__ __forceinline__ uint64_t gstride() { return uint64_t(gridDim.x) * blockDim.x; }
__device__ __forceinline__ uint64_t nseg_of(uint64_t nb) { return nb ? (nb + SEG_BITS - 1) / SEG_BITS : 1; }
__device__ __forceinline__ uint64_t seg_base(const StParams &p, uint64_t i) { return (p.pay_off[i] >> SEG_SHIFT) + i; }

// the stream and segment of segment number u; false for a gap number or a stream that is not MH_OK
struct Seg {
    uint64_t i, k, nseg, nb, base;
};
__device__ __forceinline__ bool seg_of(const StParams &p, const int *status, uint64_t u, Seg &s) {
    s.i = find_stream(p.pay_off, p.n, SEG_SHIFT, u);
    if (s.i >= p.n) return false;
    s.base = seg_base(p, s.i);
    s.k = u - s.base;
    s.nb = p.nbits[s.i];
    s.nseg = nseg_of(s.nb);
    return s.k < s.nseg && status[s.i] == MH_OK;
}
__device__ __forceinline__ uint64_t seg_lim(const Seg &s, uint64_t k) {
    const uint64_t e = (k + 1) * SEG_BITS;
    return e < s.nb ? e : s.nb;
}

// decodes from `entry` while the position is below lim: the segment's record (end == SEG_BAD on a null table entry)
template <class D>
__device__ SegRec decode_seg(const D &d, const BitSrc &src, uint64_t bit0, unsigned long long entry, uint64_t lim) {
    SegRec r;
    r.entry = entry;
    r.count = 0;
    const uint64_t pos = entry & D::POS;
    uint32_t prev = uint32_t(entry >> D::SHIFT);
    if (pos >= lim) { r.end = entry; return r; }
    const uint32_t span = uint32_t(lim - pos);          // < 2 * SEG_BITS: an entry lies less than one code past its segment start
    BitCursor bc;
    bc.init(src, bit0 + pos);
    uint32_t used = 0;
    bool bad = false;
    unsigned long long cnt = 0;
    while (used < span) {                               // every code has at least one bit
        prev = d.step(src, bc, prev, used, bad);
        if (bad) { r.end = SEG_BAD; r.count = cnt; return r; }
        ++cnt;
    }
    r.end = (uint64_t(prev) << D::SHIFT) | (pos + used);
    r.count = cnt;
    return r;
}

__device__ __forceinline__ BitSrc src_of(const StParams &p, const Seg &s, uint64_t &bit0) {
    return mhb::stream_src(p.payload, p.pay_off[s.i], s.nb, bit0);
}

// ------------------------------------------------------------------------------------------------ states

__global__ void bseg_check_kernel(StParams p, int *hdr, int *status, unsigned long long *first, unsigned long long *last) {
    const uint64_t i = gtid();
    if (i > p.n) return;
    const bool bad = mhb::offsets_bad(p.pay_off, p.n, p.pay_total, i);
    if (bad) { fail(hdr + HDR_STATUS, mhb::BATCH_STATUS_ARG); atomicExch(hdr + HDR_STOP, 1); }
    if (i == 0) hdr[HDR_CHANGED] = 1;                   // the speculation wrote every record: pass 1 runs
    if (i == p.n) return;
    int s = MH_OK;
    if (!bad && p.nbits[i] > (p.pay_off[i + 1] - p.pay_off[i]) * 8u) { s = MH_ERR_ARG; fail(hdr + HDR_STATUS, mhb::BATCH_STATUS_ARG); }
    status[i] = s;
    first[i] = ~0ull;
    last[i] = 0;
}

template <class D>
__global__ void bseg_spec_kernel(StParams p, const int *hdr, const int *status, SegRec *rec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(hdr + HDR_STOP)) return;
    D d;
    d.setup(p, smem);
    for (uint64_t u = gtid(); u < p.segs; u += gstride()) {
        Seg s;
        if (!seg_of(p, status, u, s)) continue;
        d.select(p, s.i);
        uint64_t bit0;
        const BitSrc src = src_of(p, s, bit0);
        unsigned long long entry = p.state0;
        if (s.k) {
            const uint64_t at = s.k * SEG_BITS;
            if constexpr (D::RECOVER) {
                entry = d.warmup(src, bit0, p.state0, at > WARMUP2_BITS ? at - WARMUP2_BITS : 0, at);
            } else {
                const SegRec w = decode_seg(d, src, bit0, p.state0 | (at - WARMUP_BITS), at);
                entry = w.end != SEG_BAD ? w.end : (p.state0 | at);
            }
        }
        rec[u] = decode_seg(d, src, bit0, entry, seg_lim(s, s.k));
    }
}

template <class D>
__global__ void bseg_repair_kernel(StParams p, int *hdr, const int *status, const SegRec *in, SegRec *out, int pass) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(hdr + HDR_STOP) || hdr[HDR_CHANGED + pass - 1] == 0) return;     // nothing changed: both buffers agree
    D d;
    d.setup(p, smem);
    bool changed = false;
    for (uint64_t u = gtid(); u < p.segs; u += gstride()) {
        Seg s;
        if (!seg_of(p, status, u, s)) continue;
        SegRec r = in[u];
        if (s.k) {
            const unsigned long long pe = in[u - 1].end;
            if (pe != SEG_BAD && pe != r.entry) {
                d.select(p, s.i);
                uint64_t bit0;
                const BitSrc src = src_of(p, s, bit0);
                r = decode_seg(d, src, bit0, pe, seg_lim(s, s.k));
                changed = true;                         // (any rewrite counts: an early return needs both buffers equal)
            }
        }
        out[u] = r;
    }
    if (changed) hdr[HDR_CHANGED + pass] = 1;
}

__global__ void bseg_mark_kernel(StParams p, const int *hdr, const int *status, const SegRec *rec, unsigned long long *first,
                                 unsigned long long *last) {
    if (stopped(hdr + HDR_STOP)) return;
    for (uint64_t u = gtid(); u < p.segs; u += gstride()) {
        Seg s;
        if (!seg_of(p, status, u, s) || s.k == 0) continue;
        if (rec[u - 1].end != rec[u].entry || rec[u - 1].end == SEG_BAD) {
            atomicMin(first + s.i, (unsigned long long)s.k);
            atomicMax(last + s.i, (unsigned long long)s.k);
        }
    }
}

template <class D>
__global__ void bseg_walk_kernel(StParams p, int *hdr, int *status, SegRec *rec, const unsigned long long *first,
                                 const unsigned long long *last) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(hdr + HDR_STOP)) return;
    D d;
    d.setup(p, smem);
    for (uint64_t i = gtid(); i < p.n; i += gstride()) {
        const unsigned long long f = first[i];
        if (f == ~0ull || status[i] != MH_OK) continue;
        Seg s;
        s.i = i;
        s.base = seg_base(p, i);
        s.nb = p.nbits[i];
        s.nseg = nseg_of(s.nb);
        const uint64_t L = last[i];
        unsigned long long state = rec[s.base + f - 1].end;
        if (state == SEG_BAD) continue;                 // a null table entry on the true path: the proof reports it
        atomicAdd(hdr + HDR_WALKED, 1);
        d.select(p, i);
        uint64_t bit0;
        const BitSrc src = src_of(p, s, bit0);
        const uint64_t from = f * SEG_BITS;
        for (uint64_t m = f; m < s.nseg; ) {
            if ((state & D::POS) - from > p.walk_max_bits) {
                if (atomicCAS(status + i, MH_OK, MH_ERR_ARG) == MH_OK) fail(hdr + HDR_STATUS, mhb::BATCH_STATUS_ARG);
                break;
            }
            const SegRec r = decode_seg(d, src, bit0, state, seg_lim(s, m));
            rec[s.base + m] = r;
            if (r.end == SEG_BAD) break;
            state = r.end;
            ++m;
            if (m > L && m < s.nseg && rec[s.base + m].entry == state) break;   // every segment behind is consistent
        }
    }
}

__global__ void bseg_proof_kernel(StParams p, int *hdr, int *status, const SegRec *rec) {
    if (stopped(hdr + HDR_STOP)) return;
    for (uint64_t u = gtid(); u < p.segs; u += gstride()) {
        Seg s;
        if (!seg_of(p, status, u, s)) continue;
        const SegRec r = rec[u];
        const unsigned long long want = s.k ? rec[u - 1].end : p.state0;
        const bool bad = r.entry != want || r.end == SEG_BAD || (s.k + 1 == s.nseg && (r.end & p.pos_mask) != s.nb);
        if (bad && atomicCAS(status + s.i, MH_OK, MH_ERR_CORRUPT) == MH_OK) fail(hdr + HDR_STATUS, mhk::MHK_STATUS_CORRUPT);
    }
}

__global__ void bseg_count_kernel(StParams p, const int *hdr, const int *status, const SegRec *rec, unsigned long long *counts) {
    if (stopped(hdr + HDR_STOP)) return;
    for (uint64_t u = gtid(); u < p.segs; u += gstride()) {
        Seg s;
        counts[u] = seg_of(p, status, u, s) ? rec[u].count : 0ull;
    }
}

// (offsets out of order: every stream's status is MH_ERR_ARG, nothing else is written)
__global__ void bseg_finish_kernel(StParams p, int *hdr, const int *status, const unsigned long long *scanned) {
    const uint64_t i = gtid();
    if (i > p.n) return;
    if (stopped(hdr + HDR_STOP)) {
        if (i < p.n && p.caller_status) p.caller_status[i] = MH_ERR_ARG;
        return;
    }
    p.sym_off[i] = scanned[i == p.n ? p.segs - 1 : seg_base(p, i)];
    if (i < p.n && p.caller_status) p.caller_status[i] = status[i];
    if (i == 0) {
        hdr[HDR_STATES_STATUS] = hdr[HDR_STATUS];
        unsigned long long *tag = reinterpret_cast<unsigned long long *>(reinterpret_cast<unsigned char *>(hdr) + HDR_TAG);
        for (int w = 0; w < TAG_WORDS; ++w) tag[w] = p.tag[w];
    }
}

// ------------------------------------------------------------------------------------------------ index, emit

// the batch's settled states are in the workspace (tag), the index fits; the status word restarts from the states' one
__global__ void bseg_gate_kernel(StParams p, int *hdr, const unsigned long long *scanned) {
    const unsigned long long *tag = reinterpret_cast<const unsigned long long *>(reinterpret_cast<const unsigned char *>(hdr) + HDR_TAG);
    bool same = true;
    for (int w = 0; w < TAG_WORDS; ++w) same &= tag[w] == p.tag[w];
    if (!same) { hdr[HDR_STATUS] = mhb::BATCH_STATUS_ARG; hdr[HDR_STOP] = 1; return; }
    hdr[HDR_STATUS] = hdr[HDR_STATES_STATUS];
    hdr[HDR_STOP] = 0;
    if (p.index && scanned[p.segs - 1] / (uint64_t(1) << p.chunk_shift) + p.n + 1 > p.index_cap) {
        fail(hdr + HDR_STATUS, mhk::MHK_STATUS_CAPACITY);
        hdr[HDR_STOP] = STOP_CAPACITY;
    }
}

// caller's statuses from the states' ones; emit: the streams that do not fit out_cap.  After a call-wide error of the gate
// every stream gets it (MH_ERR_ARG: no states of this batch, whose per-stream words may belong to another batch;
// MH_ERR_CAPACITY: the index does not fit) and nothing is written.
__global__ void bseg_streams_kernel(StParams p, int *hdr, const int *status, const unsigned long long *scanned) {
    const uint64_t i = gtid();
    if (i >= p.n) return;
    if (stopped(hdr + HDR_STOP)) {
        if (p.caller_status) p.caller_status[i] = hdr[HDR_STOP] == STOP_CAPACITY ? MH_ERR_CAPACITY : MH_ERR_ARG;
        return;
    }
    int s = status[i];
    if (s == MH_OK && !p.index) {                              // emit
        const uint64_t end = scanned[i + 1 == p.n ? p.segs - 1 : seg_base(p, i + 1)];
        if (end > p.out_cap) { s = MH_ERR_CAPACITY; fail(hdr + HDR_STATUS, mhk::MHK_STATUS_CAPACITY); }
    }
    if (p.caller_status) p.caller_status[i] = s;
}

template <class D>
__global__ void bseg_index_kernel(StParams p, const int *hdr, const int *status, const SegRec *rec, const unsigned long long *scanned) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(hdr + HDR_STOP)) return;
    D d;
    d.setup(p, smem);
    const uint32_t cs = p.chunk_shift;
    const uint64_t cmask = (uint64_t(1) << cs) - 1u;
    for (uint64_t u = gtid(); u < p.segs; u += gstride()) {
        Seg s;
        if (!seg_of(p, status, u, s)) continue;
        const SegRec r = rec[u];
        const uint64_t a = scanned[s.base];                       // sym_off[i]
        const uint64_t s0 = scanned[u] - a;                       // stream-relative number of the segment's first symbol
        const uint64_t s1 = s0 + r.count;
        const uint64_t c0 = (s0 + cmask) >> cs;                   // first chunk that starts in [s0, s1)
        if ((c0 << cs) >= s1) continue;
        const uint64_t t_last = ((s1 - 1) >> cs << cs) - s0;      // symbol of the last chunk start, relative to s0
        unsigned long long *slice = p.index + (a >> cs) + s.i;
        d.select(p, s.i);
        uint64_t bit0;
        const BitSrc src = src_of(p, s, bit0);
        const uint64_t pos = r.entry & D::POS;
        BitCursor bc;
        bc.init(src, bit0 + pos);
        uint32_t prev = uint32_t(r.entry >> D::SHIFT), used = 0;
        bool bad = false;
        for (uint64_t t = 0;; ++t) {
            if (((s0 + t) & cmask) == 0) slice[(s0 + t) >> cs] = (uint64_t(prev) << D::SHIFT) | (pos + used);
            if (t == t_last) break;
            prev = d.step(src, bc, prev, used, bad);
        }
    }
}

template <class D>
__global__ void bseg_emit_kernel(StParams p, const int *hdr, const int *status, const SegRec *rec, const unsigned long long *scanned) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(hdr + HDR_STOP)) return;
    D d;
    d.setup(p, smem);
    for (uint64_t u = gtid(); u < p.segs; u += gstride()) {
        Seg s;
        if (!seg_of(p, status, u, s)) continue;
        const SegRec r = rec[u];
        if (!r.count) continue;
        const uint64_t end = scanned[s.i + 1 == p.n ? p.segs - 1 : seg_base(p, s.i + 1)];
        if (end > p.out_cap) continue;                            // the stream does not fit: MH_ERR_CAPACITY, nothing written
        d.select(p, s.i);
        uint64_t bit0;
        const BitSrc src = src_of(p, s, bit0);
        BitCursor bc;
        bc.init(src, bit0 + (r.entry & D::POS));
        uint32_t prev = uint32_t(r.entry >> D::SHIFT), used = 0;
        bool bad = false;
        mhb::ByteOut bo;
        bo.init(p.out, scanned[u]);
        for (uint64_t t = 0; t < r.count; ++t) {
            prev = d.step(src, bc, prev, used, bad);
            bo.put(D::byte(prev));
        }
        bo.flush();
    }
}

// ------------------------------------------------------------------------------------------------ launchers

struct Ws {
    int *hdr, *status;
    unsigned long long *first, *last, *counts, *sums;
    SegRec *rec[2];
};
Ws ws_of(const StParams &p, void *d_ws) {
    unsigned char *b = static_cast<unsigned char *>(d_ws);
    const Layout L = layout(p.n, p.pay_total);
    Ws w;
    w.hdr = reinterpret_cast<int *>(b);
    w.status = reinterpret_cast<int *>(b + L.off_status);
    w.first = reinterpret_cast<unsigned long long *>(b + L.off_first);
    w.last = reinterpret_cast<unsigned long long *>(b + L.off_last);
    w.rec[0] = reinterpret_cast<SegRec *>(b + L.off_rec0);
    w.rec[1] = reinterpret_cast<SegRec *>(b + L.off_rec1);
    w.counts = reinterpret_cast<unsigned long long *>(b + L.off_counts);
    w.sums = reinterpret_cast<unsigned long long *>(b + L.off_sums);
    return w;
}

// the records every launch after the repair passes reads: the buffer pass K wrote (or, when a pass returned early, the
// other one, whose contents are the same)
constexpr int FINAL = REPAIR_PASSES & 1;

struct Shape {
    dim3 grid, block;
    size_t lds;
};
template <class D>
Shape shape_of(const StParams &p, uint64_t items) {
    if (p.kind == KIND_SHARED) return Shape{dim3(mhb::grid_for(items, mhb::B_THREADS, 1)), dim3(mhb::B_THREADS), p.lds};
    return Shape{dim3(mhb::grid_for(items, ST_THREADS, 8)), dim3(ST_THREADS), 0};
}

template <class D>
hipError_t allow(const StParams &p) {
    if (p.kind != KIND_SHARED) return hipSuccess;
    const int lds_max = 163840;
    hipError_t e = mhk::allow_lds(reinterpret_cast<const void *>(bseg_spec_kernel<D>), lds_max);
    if (e == hipSuccess) e = mhk::allow_lds(reinterpret_cast<const void *>(bseg_repair_kernel<D>), lds_max);
    if (e == hipSuccess) e = mhk::allow_lds(reinterpret_cast<const void *>(bseg_walk_kernel<D>), lds_max);
    if (e == hipSuccess) e = mhk::allow_lds(reinterpret_cast<const void *>(bseg_index_kernel<D>), lds_max);
    if (e == hipSuccess) e = mhk::allow_lds(reinterpret_cast<const void *>(bseg_emit_kernel<D>), lds_max);
    return e;
}

inline dim3 threads_grid(uint64_t items) { return dim3(uint32_t(items ? (items + 255) / 256 : 1)); }
inline dim3 flat_grid(uint64_t items) { return dim3(mhb::grid_for(items, 256, 8)); }

template <class D>
hipError_t run_states(const StParams &p, void *d_ws, hipStream_t st) {
    hipError_t e = allow<D>(p);
    if (e != hipSuccess) return e;
    const Ws w = ws_of(p, d_ws);
    if ((e = hipMemsetAsync(d_ws, 0, HDR_BYTES, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(bseg_check_kernel, threads_grid(p.n + 1), dim3(256), 0, st, p, w.hdr, w.status, w.first, w.last);
    const Shape seg = shape_of<D>(p, p.segs);
    hipLaunchKernelGGL(bseg_spec_kernel<D>, seg.grid, seg.block, seg.lds, st, p, w.hdr, w.status, w.rec[0]);
    for (int pass = 1; pass <= REPAIR_PASSES; ++pass)
        hipLaunchKernelGGL(bseg_repair_kernel<D>, seg.grid, seg.block, seg.lds, st, p, w.hdr, w.status, w.rec[(pass - 1) & 1],
                           w.rec[pass & 1], pass);
    SegRec *rec = w.rec[FINAL];
    hipLaunchKernelGGL(bseg_mark_kernel, flat_grid(p.segs), dim3(256), 0, st, p, w.hdr, w.status, rec, w.first, w.last);
    const Shape per_stream = shape_of<D>(p, p.n);
    hipLaunchKernelGGL(bseg_walk_kernel<D>, per_stream.grid, per_stream.block, per_stream.lds, st, p, w.hdr, w.status, rec, w.first, w.last);
    hipLaunchKernelGGL(bseg_proof_kernel, flat_grid(p.segs), dim3(256), 0, st, p, w.hdr, w.status, rec);
    hipLaunchKernelGGL(bseg_count_kernel, flat_grid(p.segs), dim3(256), 0, st, p, w.hdr, w.status, rec, w.counts);
    if ((e = mhb::scan_exclusive(w.counts, p.segs, w.sums, w.hdr + HDR_STOP, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(bseg_finish_kernel, threads_grid(p.n + 1), dim3(256), 0, st, p, w.hdr, w.status, w.counts);
    return hipGetLastError();
}

template <class D>
hipError_t run_index(const StParams &p, void *d_ws, hipStream_t st) {
    hipError_t e = allow<D>(p);
    if (e != hipSuccess) return e;
    const Ws w = ws_of(p, d_ws);
    hipLaunchKernelGGL(bseg_gate_kernel, dim3(1), dim3(1), 0, st, p, w.hdr, w.counts);
    hipLaunchKernelGGL(bseg_streams_kernel, threads_grid(p.n), dim3(256), 0, st, p, w.hdr, w.status, w.counts);
    const Shape seg = shape_of<D>(p, p.segs);
    hipLaunchKernelGGL(bseg_index_kernel<D>, seg.grid, seg.block, seg.lds, st, p, w.hdr, w.status, w.rec[FINAL], w.counts);
    return hipGetLastError();
}

template <class D>
hipError_t run_emit(const StParams &p, void *d_ws, hipStream_t st) {
    hipError_t e = allow<D>(p);
    if (e != hipSuccess) return e;
    const Ws w = ws_of(p, d_ws);
    hipLaunchKernelGGL(bseg_gate_kernel, dim3(1), dim3(1), 0, st, p, w.hdr, w.counts);
    hipLaunchKernelGGL(bseg_streams_kernel, threads_grid(p.n), dim3(256), 0, st, p, w.hdr, w.status, w.counts);
    const Shape seg = shape_of<D>(p, p.segs);
    hipLaunchKernelGGL(bseg_emit_kernel<D>, seg.grid, seg.block, seg.lds, st, p, w.hdr, w.status, w.rec[FINAL], w.counts);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_states(const StParams &p, void *d_ws, hipStream_t st) {
    if (p.kind == KIND_SHARED2) return run_states<Shared2D>(p, d_ws, st);
    return p.kind == KIND_SHARED ? run_states<SharedD>(p, d_ws, st) : run_states<SetD>(p, d_ws, st);
}
hipError_t launch_index(const StParams &p, void *d_ws, hipStream_t st) {
    if (p.kind == KIND_SHARED2) return run_index<Shared2D>(p, d_ws, st);
    return p.kind == KIND_SHARED ? run_index<SharedD>(p, d_ws, st) : run_index<SetD>(p, d_ws, st);
}
hipError_t launch_emit(const StParams &p, void *d_ws, hipStream_t st) {
    if (p.kind == KIND_SHARED2) return run_emit<Shared2D>(p, d_ws, st);
    return p.kind == KIND_SHARED ? run_emit<SharedD>(p, d_ws, st) : run_emit<SetD>(p, d_ws, st);
}

}  // namespace mhs
