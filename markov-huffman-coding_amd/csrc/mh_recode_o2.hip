// mh_recode_o2.hip — the coded histogram and the re-coding of a batch with an ORDER-2 side (include/mh.h, "ORDER 2 IN SEARCH
// AND RE-CODING"): an order-0/1 batch counted or coded under order-2 contexts, an order-2 batch counted or coded under any
// order.  The passes are those of mh_recode.hip; what differs:
//   Dec<S2>      the source decoder.  S2: the model's order-2 tables read from L2 as batch2_dec_idx_kernel reads them,
//                workgroups of 256 lanes, eight per CU, entries masked with IDX2_POS and their context taken from e >> 48.
//                Order 0/1: the tables in LDS as load_tables lays them out, one workgroup per CU (mh_recode.hip's shape).
//                Every lane rolls a 16-bit context c16 = ((c16 << 8) | sym) & 0xFFFF whatever the orders are.
//   Enc          the destination's (len, code) at (c16 & mask) << 8 | sym, read from L2: lengths from len8 in the length
//                pass, codes from the packed enc64 of an order-2 model ((len8, code64) over 56 bits) or from code64.
//   the seam     an order-0/1 entry carries one context byte, so the lane of chunk k does not know the symbol two in front
//                of its first one.  With an order-0/1 source the lane of chunk k therefore owns symbols first + 1 ...
//                first + nsym: it decodes one symbol into the next chunk, whose two context bytes it knows; the lane of a
//                stream's first chunk also owns symbol 0 under (prev0, prev0).  recode2_idx_len_kernel keeps that symbol's
//                bits apart ("head") and the chunk's last two symbols ("close"); recode2_comb_kernel adds head(k - 1) to
//                the bits of chunk k, so the scanned value is the bit offset of chunk k's first code, its destination entry.
//                The extra symbol never sets a verdict: the next chunk's own lane judges that chunk, and when the stream
//                passed, that lane decoded the same bits in the same context.  A chunk that is not its stream's last has
//                >= 256 symbols, so the two symbols in front of a chunk lie in the previous chunk.  An order-2 source and
//                the index-free walk need none of this.
//   histc2_*     count-and-take-back as in mh_recode.hip; the take-back repeats exactly what was counted, the extra symbol
//                included (it is counted only by a chunk that passed).  Counters: a direct-mapped cache in LDS in front of
//                64-bit global atomics into the caller's 256, 65 536 or 1 << 24 counts.
// Verdicts are mh_dev_decode_batch's (order-0/1 source) or mh_dev_decode_batch_o2's (order-2 source): same checks, same
// statuses.  Every loop is bounded by a symbol count or nbits_i.
#include "mh_recode_o2.h"
#include "mh_batch_dev.hpp"
#include "mh_recode_dev.hpp"
#include "../../include/mh.h"

namespace mhr {

using mhb::BATCH_STATUS_ARG;
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

constexpr int NT_LDS = mhb::B_THREADS;             // order-0/1 source: one workgroup per CU beside the tables
constexpr int NT_L2 = 256;                         // order-2 source: batch2_dec_idx_kernel's shape
constexpr int LDS_MAX = 163840;
template <bool S2> constexpr int nt_of() { return S2 ? NT_L2 : NT_LDS; }

__device__ __forceinline__ uint32_t roll(uint32_t c16, uint32_t sym) { return ((c16 << 8) | sym) & 0xFFFFu; }

// the symbol decoder of a lane, in the 16-bit context c16 (an order-0/1 model reads its last byte)
template <bool S2> struct Dec;
template <> struct Dec<false> {
    const uint16_t *lut;
    const uint32_t *sub_base;
    DecTables tabs;
    __device__ __forceinline__ Dec(const Src &s, unsigned char *smem) : tabs(mhb::load_tables(s.b, smem, lut, sub_base)) {}
    __device__ __forceinline__ uint32_t next(const BitSrc &src, BitCursor &bc, uint32_t c16, uint32_t &used, bool &bad) const {
        return mhk::decode_one(lut, sub_base, tabs, src, bc, c16 & 0xFFu, used, bad);
    }
};
template <> struct Dec<true> {
    const uint16_t *prim;
    const uint32_t *sec_base;
    DecTables tabs;
    __device__ __forceinline__ Dec(const Src &s, unsigned char *) : prim(s.b.prim), sec_base(s.b.sec_base), tabs{s.b.sec, s.b.tree, s.b.P, 0u, 0u} {}
    __device__ __forceinline__ uint32_t next(const BitSrc &src, BitCursor &bc, uint32_t c16, uint32_t &used, bool &bad) const {
        return mhk::decode_one(prim, sec_base, tabs, src, bc, c16, used, bad);
    }
};

// (c16, sym) -> the index of a count or of a code: both context bytes (order 2), the last one (order 1) or none (order 0)
__device__ __forceinline__ uint32_t ctx_mask_of(uint32_t order) { return order == 2u ? 0xFFFFu : (order ? 0xFFu : 0u); }

// the destination's codes, read from L2
struct Enc {
    const uint8_t *len8;
    const unsigned long long *code64, *enc64;
    uint32_t mask;
    __device__ __forceinline__ explicit Enc(const Dst2 &d) : len8(d.len8), code64(d.code64), enc64(d.order == 2u ? d.enc64 : nullptr), mask(ctx_mask_of(d.order)) {}
    __device__ __forceinline__ uint32_t at(uint32_t c16, uint32_t sym) const { return ((c16 & mask) << 8) | sym; }
    __device__ __forceinline__ uint32_t len(uint32_t key) const {
        const uint32_t l = len8[key];
        return l > 64u ? 0u : l;                                  // 0: the pair has no code, skipped (mh_model.hpp:21)
    }
    __device__ __forceinline__ void code(uint32_t key, uint32_t &l, uint64_t &c) const {
        const uint64_t e = enc64 ? enc64[key] : 0xFF00000000000000ull;
        l = uint32_t(e >> 56);
        c = e & 0x00FFFFFFFFFFFFFFull;
        if (l == 255u) {                                          // longer than 56 bits, or no packed table
            l = len8[key];
            c = code64[key];
        }
        if (l > 64u) l = 0;
    }
    // the context part of a destination index entry
    __device__ __forceinline__ uint64_t entry(uint32_t c16, uint64_t bit) const {
        return mask == 0xFFFFu ? (uint64_t(c16) << 48) | bit : (uint64_t(c16 & 0xFFu) << 56) | bit;
    }
};

// the context in front of a stream's first symbol: (prev0, prev0)
template <bool S2> __device__ __forceinline__ uint32_t start16(const Src &s) { return S2 ? s.b.prev0 : ((s.b.prev0 & 0xFFu) * 0x101u); }

// chunk w of the indexed batch with its entry's context widened to the 16 bits the lane starts in; false when w is a gap.
// Order-0/1 source: the high byte is known only in a stream's first chunk (prev0), elsewhere the lane does not own symbol 0.
template <bool S2>
__device__ __forceinline__ bool chunk_of(const Src &s, uint64_t w, Chunk &c) {
    if (!mhb::chunk_of<S2>(s.b, w, c)) return false;
    if (!S2) c.ctx |= c.first ? 0u : (s.b.prev0 & 0xFFu) << 8;
    return true;
}
// symbol t of chunk c belongs to c's lane (else to the lane of the chunk in front, which knows both context bytes)
template <bool S2> __device__ __forceinline__ bool owns(const Chunk &c, uint32_t t) { return S2 || t > 0u || c.first == 0u; }

// ------------------------------------------------------------------------------------------------ histogram

// Direct-mapped counters in LDS: slot -> (key, u64 count); a key that finds its slot taken goes to the 64-bit global
// counter.  Counts go up and down (a failed chunk takes its counts back): the sums wrap modulo 2^64 and are exact.
// nslot == 0: no LDS left, global atomics only.
struct KeyCache {
    static constexpr uint32_t EMPTY = 0xFFFFFFFFu;
    unsigned long long *cnt;
    uint32_t *tag;
    uint32_t shift, nslot, mask;
    unsigned long long *g;
    __device__ __forceinline__ void init(unsigned char *smem, uint32_t lds_at, uint32_t log2n, uint32_t order, unsigned long long *counts) {
        nslot = log2n ? 1u << log2n : 0u;
        shift = 32u - log2n;
        cnt = reinterpret_cast<unsigned long long *>(smem + lds_at);
        tag = reinterpret_cast<uint32_t *>(cnt + nslot);
        mask = ctx_mask_of(order);
        g = counts;
        for (uint32_t k = threadIdx.x; k < nslot; k += blockDim.x) { tag[k] = EMPTY; cnt[k] = 0ull; }
        __syncthreads();
    }
    __device__ __forceinline__ void add(uint32_t c16, uint32_t sym, int delta) {
        const uint32_t p = ((c16 & mask) << 8) | sym;
        const unsigned long long d = static_cast<unsigned long long>(static_cast<long long>(delta));
        if (nslot) {
            const uint32_t slot = mask ? (p * 2654435761u) >> shift : p;           // (nslot >= 256: order 0 never collides)
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

// `count` symbols of chunk c from its entry, the lane's own counted `delta` times (0: decode only); ext: when these symbols
// end exactly at the chunk's end, the first symbol of the next chunk is counted too (order-0/1 source).  Returns the symbols
// done; used / bad describe the `count` symbols alone.
template <bool S2>
__device__ __forceinline__ uint32_t walk_chunk(const Src &s, const Dec<S2> &dec, const Chunk &c, uint32_t count, bool ext, int delta, KeyCache &kc,
                                               uint32_t &used, bool &bad) {
    uint64_t bit0;
    const BitSrc src = mhb::stream_src(s.b.payload, s.b.pay_off[c.i], c.nb, bit0);
    BitCursor bc;
    bc.init(src, bit0 + c.start);
    uint32_t c16 = c.ctx, t = 0;
    used = 0; bad = false;
    for (; t < count; ++t) {
        const uint32_t sym = dec.next(src, bc, c16, used, bad);
        if (bad) break;
        if (delta && owns<S2>(c, t)) kc.add(c16, sym, delta);
        c16 = roll(c16, sym);
    }
    if (!S2 && ext && !c.last && !bad && used == c.end - c.start) {
        uint32_t u2 = used;
        bool b2 = false;
        const uint32_t sym = dec.next(src, bc, c16, u2, b2);
        if (!b2 && delta) kc.add(c16, sym, delta);
    }
    return t;
}

template <bool S2, bool FIX>
__global__ __launch_bounds__(nt_of<S2>()) void histc2_idx_kernel(Hist2Params p, uint64_t nwork, uint32_t lds_at, uint32_t log2n, int *status,
                                                                 const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    if (FIX && *reinterpret_cast<const volatile int *>(status) == 0) return;      // no stream failed: nothing to take back
    Dec<S2> dec(p.s, smem);
    KeyCache kc;
    kc.init(smem, lds_at, log2n, p.order, p.counts);
    for (uint64_t base = uint64_t(blockIdx.x) * blockDim.x; base < nwork; base += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t w = base + threadIdx.x;
        Chunk c;
        if (w < nwork && chunk_of<S2>(p.s, w, c)) {
            const int verdict = p.s.b.stream_status[c.i];
            uint32_t used; bool bad;
            if (!FIX && verdict != MH_ERR_ARG) {
                if (!c.entry_ok()) {
                    stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                } else {
                    const uint32_t done = walk_chunk<S2>(p.s, dec, c, c.nsym, true, 1, kc, used, bad);
                    if (bad || used != c.end - c.start) {           // (the extra symbol was not counted)
                        stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                        walk_chunk<S2>(p.s, dec, c, done, false, -1, kc, used, bad);
                    }
                }
            }
            if (FIX && verdict == MH_ERR_CORRUPT && c.entry_ok()) {               // (a chunk that failed has taken its counts back)
                walk_chunk<S2>(p.s, dec, c, c.nsym, false, 0, kc, used, bad);
                if (!bad && used == c.end - c.start) walk_chunk<S2>(p.s, dec, c, c.nsym, true, -1, kc, used, bad);
            }
        }
    }
    kc.flush();
}

// at most `limit` symbols of stream i from bit 0, each counted `delta` times; returns the symbols done
template <bool S2>
__device__ __forceinline__ uint64_t walk_stream(const Src &s, const Dec<S2> &dec, uint64_t i, uint64_t nb, uint64_t limit, int delta, KeyCache &kc,
                                                uint32_t &used, bool &bad) {
    uint64_t bit0;
    const BitSrc src = mhb::stream_src(s.b.payload, s.b.pay_off[i], nb, bit0);
    BitCursor bc;
    bc.init(src, bit0);
    uint32_t c16 = start16<S2>(s);
    uint64_t k = 0;
    used = 0; bad = false;
    // every code has at least one bit: at most nb steps
    while (used < nb && k < limit) {
        const uint32_t sym = dec.next(src, bc, c16, used, bad);
        if (bad) break;
        kc.add(c16, sym, delta);
        c16 = roll(c16, sym);
        ++k;
    }
    return k;
}

template <bool S2>
__global__ __launch_bounds__(nt_of<S2>()) void histc2_walk_kernel(Hist2Params p, uint32_t lds_at, uint32_t log2n, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<S2> dec(p.s, smem);
    KeyCache kc;
    kc.init(smem, lds_at, log2n, p.order, p.counts);
    const uint64_t n = p.s.b.n;
    for (uint64_t base = uint64_t(blockIdx.x) * blockDim.x; base < n; base += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        if (i < n && p.s.b.stream_status[i] == MH_OK) {
            const uint64_t nb = p.s.b.nbits[i];
            if (nb > p.s.b.walk_max_bits) {
                stream_fail(p.s.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
            } else {
                uint32_t used; bool bad;
                const uint64_t done = walk_stream<S2>(p.s, dec, i, nb, ~uint64_t(0), 1, kc, used, bad);
                if (bad || used != nb) {                            // the stream ends exactly at nbits
                    stream_fail(p.s.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                    walk_stream<S2>(p.s, dec, i, nb, done, -1, kc, used, bad);
                }
            }
        }
    }
    kc.flush();
}

// ------------------------------------------------------------------------------------------------ re-code

template <bool S2>
__global__ __launch_bounds__(nt_of<S2>()) void recode2_idx_len_kernel(Recode2Params p, uint64_t nwork, unsigned long long *cbits, uint32_t *cdrop,
                                                                      uint32_t *chead, uint32_t *cclose, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<S2> dec(p.s, smem);
    const Enc E(p.dst);
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of<S2>(p.s, w, c) || p.s.b.stream_status[c.i] == MH_ERR_ARG) continue;
        if (!c.entry_ok()) { stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        uint32_t c16 = c.ctx, used = 0, bits = 0, drops = 0;
        bool bad = false;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {
            const uint32_t sym = dec.next(src, bc, c16, used, bad);
            if (bad) break;
            if (owns<S2>(c, t)) {
                const uint32_t l = E.len(E.at(c16, sym));
                bits += l;
                drops += l == 0u;
            }
            c16 = roll(c16, sym);
        }
        if (bad || used != c.end - c.start) { stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        if (!S2 && !c.last) {
            // the next chunk's first symbol, whose two context bytes only this lane knows.  No verdict: when the stream
            // passes, the next chunk's lane decoded the same bits in the same context.
            cclose[w] = c16;
            uint32_t u2 = used;
            bool b2 = false;
            const uint32_t sym = dec.next(src, bc, c16, u2, b2);
            if (!b2) {
                const uint32_t l = E.len(E.at(c16, sym));
                chead[w] = l;
                drops += l == 0u;
            }
        }
        cbits[w] = bits;
        cdrop[w] = drops;
    }
}

// the chunks of failed streams count 0 bits; chunk k of the others: its own bits and, behind a seam, its first symbol's,
// which the lane in front priced; the dropped symbols go to dropped[i]
template <bool S2>
__global__ __launch_bounds__(256) void recode2_comb_kernel(Recode2Params p, uint64_t nwork, unsigned long long *cbits, const uint32_t *cdrop,
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
                v = cbits[w] + ((!S2 && k) ? chead[w - 1] : 0u);
                const uint32_t d = cdrop[w];
                if (d && p.dropped) atomicAdd(&p.dropped[i], static_cast<unsigned long long>(d));
            }
        }
    }
    cbits[w] = v;
}

template <bool S2>
__global__ __launch_bounds__(nt_of<S2>()) void recode2_idx_emit_kernel(Recode2Params p, uint64_t nwork, const unsigned long long *cbase,
                                                                       const uint32_t *chead, const uint32_t *cclose, uint32_t *tail,
                                                                       const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<S2> dec(p.s, smem);
    const Enc E(p.dst);
    const uint64_t bytes = p.out_off[p.s.b.n];
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint32_t cs = p.s.b.chunk_shift;
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of<S2>(p.s, w, c) || p.s.b.stream_status[c.i] != MH_OK) continue;
        const unsigned long long b0 = cbase[w];
        const uint64_t rel = b0 - cbase[(p.s.b.sym_off[c.i] >> cs) + c.i];          // relative to the stream's own payload
        const bool seam = !S2 && c.first != 0u;                                     // symbol 0 is the lane's in front
        if (p.out_index) p.out_index[w] = E.entry(seam ? cclose[w - 1] : c.ctx, rel);
        if (!p.out) continue;
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        BitWriter bw;
        bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[c.i]) * 8u + rel + (seam ? chead[w - 1] : 0u));
        uint32_t c16 = c.ctx, used = 0, l;
        uint64_t code;
        bool bad = false, any = false;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {            // (the stream passed: bad stays false)
            const uint32_t sym = dec.next(src, bc, c16, used, bad);
            if (owns<S2>(c, t)) {
                E.code(E.at(c16, sym), l, code);
                if (l) { bw.code(code, l); any = true; }            // 0: the pair has no code, skipped (mh_model.hpp:21)
            }
            c16 = roll(c16, sym);
        }
        if (!S2 && !c.last && !bad) {
            const uint32_t sym = dec.next(src, bc, c16, used, bad);
            E.code(E.at(c16, sym), l, code);
            if (l && !bad) { bw.code(code, l); any = true; }
        }
        if (any) bw.finish();
    }
}

// EMIT = false: the stream's verdict, its symbols into sym_off[i] (scanned next), its dst bits and dropped symbols;
// true: its codes from out_off[i] and its index entries
template <bool S2, bool EMIT>
__global__ __launch_bounds__(nt_of<S2>()) void recode2_walk_kernel(Recode2Params p, uint32_t *tail, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<S2> dec(p.s, smem);
    const Enc E(p.dst);
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
        BitWriter bw;
        if (EMIT && p.out) bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[i]) * 8u);
        uint32_t c16 = start16<S2>(p.s), used = 0;
        bool bad = false;
        uint64_t k = 0, bits = 0, drops = 0;
        // every code has at least one bit: at most nb steps
        while (used < nb && !bad && k < count) {
            if (EMIT && p.out_index && (k & ((uint64_t(1) << ocs) - 1u)) == 0) p.out_index[(a >> ocs) + i + (k >> ocs)] = E.entry(c16, bits);
            const uint32_t sym = dec.next(src, bc, c16, used, bad);
            if (bad) break;
            const uint32_t key = E.at(c16, sym);
            uint32_t l;
            if (EMIT) {
                uint64_t code;
                E.code(key, l, code);
                if (l && p.out) bw.code(code, l);
            } else {
                l = E.len(key);
                drops += l == 0u;
            }
            bits += l;
            c16 = roll(c16, sym);
            ++k;
        }
        if (EMIT) { if (p.out && bits) bw.finish(); continue; }
        if (bad || used != nb) { stream_fail(p.s.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        p.s.b.sym_off[i] = k;                                       // the stream ends exactly at nbits
        p.out_nbits[i] = bits;
        if (p.dropped) p.dropped[i] = drops;
    }
}

template <bool S2>
hipError_t launch_hist(const Hist2Params &p, void *d_ws, hipStream_t st) {
    constexpr int NT = nt_of<S2>();
    constexpr int PER_CU = S2 ? 8 : 1;
    const size_t lds_tables = S2 ? 0 : mhb::tables_lds(p.s.b);
    if (lds_tables > size_t(LDS_MAX)) return hipErrorInvalidValue;
    // the counters take what the tables leave, 12 bytes a slot: 256 .. 4096 slots (order-2 source, eight workgroups per
    // CU: 1024), or none
    uint32_t log2n = 0;
    const size_t room = S2 ? size_t(12288) : size_t(LDS_MAX) - lds_tables;
    for (uint32_t k = 8; k <= 12; ++k)
        if ((size_t(12) << k) <= room) log2n = k;
    const size_t lds = lds_tables + (log2n ? size_t(12) << log2n : 0);
    const uint32_t lds_at = uint32_t(lds_tables);
    if (!S2) {
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(histc2_idx_kernel<S2, false>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(histc2_idx_kernel<S2, true>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(histc2_walk_kernel<S2>), LDS_MAX);
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
        const uint64_t W = mhb::work_items(n, p.s.b.sym_total, 1u << p.s.b.chunk_shift);
        hipLaunchKernelGGL((histc2_idx_kernel<S2, false>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, lds_at, log2n, status, stop);
        hipLaunchKernelGGL((histc2_idx_kernel<S2, true>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, lds_at, log2n, status, stop);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((histc2_walk_kernel<S2>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, lds_at, log2n, status, stop);
    return hipGetLastError();
}

template <bool S2>
hipError_t launch_rc(const Recode2Params &p, void *d_ws, hipStream_t st) {
    constexpr int NT = nt_of<S2>();
    constexpr int PER_CU = S2 ? 8 : 1;
    const size_t lds = S2 ? 0 : mhb::tables_lds(p.s.b);
    if (lds > size_t(LDS_MAX)) return hipErrorInvalidValue;
    if (!S2) {
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(recode2_idx_len_kernel<S2>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(recode2_idx_emit_kernel<S2>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(recode2_walk_kernel<S2, false>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(recode2_walk_kernel<S2, true>), LDS_MAX);
        if (attr != hipSuccess) return attr;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.s.b.n;
    const uint64_t W = p.s.b.index ? mhb::work_items(n, p.s.b.sym_total, 1u << p.s.b.chunk_shift) : 0;
    const Recode2Layout L = recode2_layout(n, W);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    uint32_t *tail = reinterpret_cast<uint32_t *>(ws + TAIL_AT);
    auto *cbits = reinterpret_cast<unsigned long long *>(ws + L.off_bits);
    auto *cdrop = reinterpret_cast<uint32_t *>(ws + L.off_drop);
    auto *chead = reinterpret_cast<uint32_t *>(ws + L.off_head);
    auto *cclose = reinterpret_cast<uint32_t *>(ws + L.off_close);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e == hipSuccess && W) e = hipMemsetAsync(ws + L.off_bits, 0, L.off_sums - L.off_bits, st);    // chunk bits, dropped counts, heads
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(recode_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, status, stop);
    if (p.s.b.index) {
        hipLaunchKernelGGL((recode2_idx_len_kernel<S2>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, cbits, cdrop, chead, cclose,
                           status, stop);
        hipLaunchKernelGGL((recode2_comb_kernel<S2>), grid_threads(W + 1, 256), dim3(256), 0, st, p, W, cbits, cdrop, chead, stop);
        if ((e = scan_exclusive(cbits, W + 1, sums, stop, st)) != hipSuccess) return e;
    } else {
        hipLaunchKernelGGL((recode2_walk_kernel<S2, false>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, tail, status, stop);
        if ((e = scan_exclusive(p.s.b.sym_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(recode_sizes_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, cbits, stop);
    if ((e = scan_exclusive(p.out_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    if (!p.s.b.index && p.out_index) hipLaunchKernelGGL(recode_cap_kernel, dim3(1), dim3(1), 0, st, p, status, stop);
    if (p.out) hipLaunchKernelGGL(recode_zero_kernel, dim3(grid_for(p.cap / 4 + 1, 256, 8)), dim3(256), 0, st, p, status, stop, tail);
    if (p.s.b.index) {
        if (p.out || p.out_index)
            hipLaunchKernelGGL((recode2_idx_emit_kernel<S2>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, cbits, chead, cclose, tail,
                               stop);
    } else if (p.out || p.out_index) {
        hipLaunchKernelGGL((recode2_walk_kernel<S2, true>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, tail, status, stop);
    }
    if (p.out) hipLaunchKernelGGL(recode_tail_kernel, dim3(1), dim3(1), 0, st, p, tail, stop);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_histogram_coded_o2(const Hist2Params &p, void *d_ws, hipStream_t st) {
    return p.src2 ? launch_hist<true>(p, d_ws, st) : launch_hist<false>(p, d_ws, st);
}

hipError_t launch_recode_o2(const Recode2Params &p, void *d_ws, hipStream_t st) {
    return p.src2 ? launch_rc<true>(p, d_ws, st) : launch_rc<false>(p, d_ws, st);
}

}  // namespace mhr
