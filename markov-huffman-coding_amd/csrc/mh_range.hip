// mh_range.hip — random access for every order and model kind (include/mh.h, "RANDOM ACCESS: BYTE RANGES OF AN INDEXED
// STREAM", "RANDOM ACCESS INTO BATCHES", "RANDOM ACCESS INTO ORDER-2 STREAMS"): byte ranges of one indexed stream, and lookups
// (stream, begin, end) into a batch.  A work unit is a chunk of the chunk index, or a piece of MH_FINE_SYMBOLS symbols when
// the fine index is given (ranges); without a batch index it is the whole stream, walked by one lane from bit 0.  An item is
// one (range or lookup, unit) pair: the symbols of the unit that lie in the range.
//   count_kernel<Params>            one thread per range or lookup: checks it (lookups: and the offsets of its stream), writes
//                                   its status and the number of units it touches (0: empty or refused)
//   batch_scan_*                    exclusive scan of the counts: item bases, entry n = the item total
//   range_kernel<Format>            one lane per item on a grid-stride loop up to the total (read on the device): the lane
//                                   starts where the index format puts its unit, decodes the symbols in front of the range
//                                   without storing them, then stores its share of the range through ByteOut
//   lookup_kernel<Tables, INDEXED>  the same over pay_off / nbits / sym_off / index slices, or one lane per lookup walking an
//                                   index-free stream from bit 0 in context prev0
// Only the offsets of the streams a lookup names are read, so the cost does not depend on the batch's stream count.
//   Tables   the symbol decoder of a lane, one policy per model (mhb::Model): SharedTables, SetTables, Shared2Tables, with
//            item_of and tables_room in mh_range_dev.hpp, which the span tokens (mh_token.hip) share.
//   Format   where a unit of a single stream starts and what bounds it: the part of include/mh.h in which the two orders
//            differ (Format01, Format2).  Everything else of range_kernel is written once.
// The scan, the bit source of a window and ByteOut are mh_batch_dev.hpp's, used as they are.
#include "mh_range_dev.hpp"

namespace mhq {

using mhb::BATCH_STATUS_ARG;
using mhb::Model;

namespace {

constexpr uint32_t FINE2_NONE = 0xFFFFu;            // an order-2 fine entry whose distance does not fit 16 bits

__device__ __forceinline__ void item_fail(int *item_status, int *status, uint64_t j, int mh_code, int dev_code) {
    atomicCAS(&item_status[j], MH_OK, mh_code);
    mhb::fail(status, dev_code);
}

// item j's share of a unit: `skip` symbols decoded and dropped, then `store` symbols to the item's output from byte `ahead`
template <typename Tables, typename P>
__device__ __forceinline__ void decode_share(const Tables &tb, const P &p, const BitSrc &src, BitCursor &bc, uint32_t &ctx, uint32_t skip,
                                             uint32_t store, uint64_t j, uint64_t ahead, uint32_t &used, bool &bad) {
    for (uint32_t t = 0; t < skip && !bad; ++t) tb.next(p, src, bc, ctx, used, bad);
    mhb::ByteOut bo;
    bo.init(p.out, p.out_at[j] + ahead);
    for (uint32_t t = 0; t < store && !bad; ++t) bo.put(tb.next(p, src, bc, ctx, used, bad));
    bo.flush();
}

// ------------------------------------------------------------------------------------------------ count

// range j of one stream: its status, and the units it touches
__device__ __forceinline__ int check_item(const RangeParams &p, uint64_t j, uint64_t &cnt) {
    const uint64_t b = p.ranges[2 * j], e = p.ranges[2 * j + 1];
    cnt = 0;
    if (b > e || e > p.n_symbols) return MH_ERR_ARG;
    if (b == e) return MH_OK;
    const uint64_t at = p.out_at[j];
    if (at > p.out_cap || e - b > p.out_cap - at) return MH_ERR_CAPACITY;
    cnt = ((e - 1) >> p.unit_shift) - (b >> p.unit_shift) + 1;
    return MH_OK;
}

// lookup j into a batch: its status, and the units it touches
__device__ __forceinline__ int check_item(const LookupParams &p, uint64_t j, uint64_t &cnt) {
    const uint64_t i = p.lookups[3 * j], b = p.lookups[3 * j + 1], e = p.lookups[3 * j + 2];
    cnt = 0;
    if (i >= p.n_streams || b > e) return MH_ERR_ARG;
    const uint64_t p0 = p.pay_off[i], p1 = p.pay_off[i + 1], nb = p.nbits[i];
    if (p1 < p0 || nb > (p1 - p0) * 8u) return MH_ERR_ARG;
    if (p.sym_off) {
        const uint64_t s0 = p.sym_off[i], s1 = p.sym_off[i + 1];
        if (s1 < s0 || e > s1 - s0) return MH_ERR_ARG;
    } else if (e > nb) {
        return MH_ERR_ARG;                                    // every code has at least one bit: n_i <= nbits_i
    }
    if (b == e) return MH_OK;
    const uint64_t at = p.out_at[j];
    if (at > p.out_cap || e - b > p.out_cap - at) return MH_ERR_CAPACITY;
    if (p.index) cnt = ((e - 1) >> p.chunk_shift) - (b >> p.chunk_shift) + 1;
    else if (nb > p.walk_max_bits) return MH_ERR_ARG;
    else cnt = 1;
    return MH_OK;
}

template <typename Params>
__global__ void count_kernel(Params p, unsigned long long *bases, int *status) {
    const uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j > p.n) return;
    if (j == p.n) { bases[j] = 0; return; }
    uint64_t cnt;
    const int st = check_item(p, j, cnt);
    p.status[j] = st;
    bases[j] = cnt;
    if (st != MH_OK) mhb::fail(status, st == MH_ERR_ARG ? BATCH_STATUS_ARG : mhk::MHK_STATUS_CAPACITY);
}

// ------------------------------------------------------------------------------------------------ one stream

// Where the lane of a unit starts and what bounds it.  s: payload bit offset from the stream start; s_sym: the symbol there;
// ctx: the context in front of it; exact: the item must use exactly the bits [s, next); corrupt: the entries contradict each
// other or nbits.  A format's lim(s, next, exact) is the last bit the window must hold before the lane decodes.
struct Start {
    uint64_t s, s_sym, next;
    uint32_t ctx;
    bool exact, corrupt;
};

// Order 0/1: every unit has its own entry.  With a fine index the entry holds the low 24 bits of the offset; its chunk's entry
// supplies the rest (a chunk spans fewer than 2^24 bits).
struct Format01 {
    using Tables = SharedTables;
    static constexpr bool JUDGES_OVERRUN = false;        // lim = next: no lane reads past the window
    __device__ __forceinline__ Format01(const RangeParams &) {}
    static __device__ __forceinline__ uint64_t unit_pos(const RangeParams &p, uint64_t u, uint32_t &ctx) {
        if (!p.fine) {
            const uint64_t e = p.index[u];
            ctx = uint32_t(e >> 56);
            return e & MH_INDEX_BIT_MASK;
        }
        const uint64_t base = p.index[(u << p.unit_shift) >> p.chunk_shift] & MH_INDEX_BIT_MASK;
        const uint32_t f = p.fine[u];
        ctx = f >> 24;
        return base + ((f - uint32_t(base)) & mhk::FINE_POS_MASK);
    }
    __device__ __forceinline__ void locate(const RangeParams &p, uint64_t u, uint64_t ustart, uint64_t uend, uint64_t last, Start &a) const {
        uint32_t pctx;
        a.s = unit_pos(p, u, a.ctx);
        a.s_sym = ustart;
        a.corrupt = a.s > p.nbits || (u > 0 && a.s < unit_pos(p, u - 1, pctx));
        // an item that ends on a unit boundary must use exactly the bits up to the next entry (nbits after the last symbol)
        a.exact = last == uend || last == p.n_symbols;
        a.next = last == p.n_symbols ? p.nbits : (u + 1 < p.n_units ? unit_pos(p, u + 1, pctx) : p.nbits);
    }
    // the whole unit must lie in the window, even where the range ends earlier
    static __device__ __forceinline__ uint64_t lim(const RangeParams &p, uint64_t s, uint64_t next, bool) { return (next >= s && next <= p.nbits) ? next : s; }
};

// Order 2: entries are ctx16 << 48 | offset; a fine entry is ctx16 << 16 | its distance from the chunk's entry, or FINE2_NONE.
struct Format2 {
    using Tables = Shared2Tables;
    static constexpr bool JUDGES_OVERRUN = true;         // lim = s inside a unit: a decode that reads past the window is refused afterwards
    uint64_t C, nchunks;                                 // symbols of a chunk, chunks of the stream
    __device__ __forceinline__ Format2(const RangeParams &p) : C(uint64_t(1) << p.chunk_shift), nchunks((p.n_symbols + C - 1) >> p.chunk_shift) {}
    __device__ __forceinline__ void locate(const RangeParams &p, uint64_t u, uint64_t ustart, uint64_t uend, uint64_t last, Start &a) const {
        constexpr uint64_t POS = Shared2Tables::POS;
        const uint32_t us = p.unit_shift, cs = p.chunk_shift;
        // the unit's chunk and its span [cpos, chi]
        const uint64_t c = ustart >> cs;
        const uint64_t ce = p.index[c], cpos = ce & POS;
        const uint64_t cnext = c + 1 < nchunks ? (p.index[c + 1] & POS) : p.nbits;
        const uint64_t chi = cnext < p.nbits ? cnext : p.nbits;
        bool corrupt = cpos > p.nbits || (c > 0 && cpos < (p.index[c - 1] & POS));
        // start: the unit's own fine entry, the nearest earlier usable piece of the chunk, or the chunk's entry
        uint64_t s = cpos, s_sym = c << cs;
        uint32_t ctx = Shared2Tables::entry_ctx(ce);
        if (p.fine) {
            for (uint64_t q = u; q > (c << (cs - us)); --q) {
                const uint32_t f = p.fine[q];
                if ((f & 0xFFFFu) == FINE2_NONE) continue;
                s = cpos + (f & 0xFFFFu);
                s_sym = q << us;
                ctx = f >> 16;
                corrupt |= s > chi;
                break;
            }
        }
        // an item that ends on a unit boundary must use exactly the bits up to the next entry (nbits after the last symbol);
        // a piece boundary whose fine entry does not fit gives no bound: the item is checked as one that ends inside a unit
        bool exact = false;
        uint64_t next = 0;
        if (last == p.n_symbols) { exact = true; next = p.nbits; }
        else if (last == uend && (uend & (C - 1)) == 0) { exact = true; next = cnext; }
        else if (last == uend) {
            const uint32_t f = p.fine[u + 1];
            if ((f & 0xFFFFu) != FINE2_NONE) {
                exact = true;
                next = cpos + (f & 0xFFFFu);
                corrupt |= next > chi;
            }
        }
        a.s = s; a.s_sym = s_sym; a.next = next; a.ctx = ctx; a.exact = exact; a.corrupt = corrupt;
    }
    static __device__ __forceinline__ uint64_t lim(const RangeParams &, uint64_t s, uint64_t next, bool exact) { return exact ? next : s; }
};

template <typename Format>
__global__ __launch_bounds__(Format::Tables::BOUND) void range_kernel(RangeParams p, const unsigned long long *bases, int *status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typename Format::Tables tb;
    tb.init(p, smem);
    const Format fmt(p);
    const uint64_t total = bases[p.n];
    const uint32_t us = p.unit_shift;
    const uint64_t U = uint64_t(1) << us;
    // the window as a bit source: reads stay inside the aligned dwords that hold its bytes (stream_src with the window at
    // byte offset a of the dword in front of it)
    const uint32_t a = uint32_t(reinterpret_cast<uintptr_t>(p.payload) & 3u);
    uint64_t bit0;
    const BitSrc src = mhb::stream_src(p.payload - a, a, p.win_bytes * 8u, bit0);
    const uint64_t win_lo = p.win_base * 8u, win_hi = (p.win_base + p.win_bytes) * 8u;
    for (uint64_t w = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < total; w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t j = item_of(bases, p.n, w);
        const uint64_t b = p.ranges[2 * j], e = p.ranges[2 * j + 1];
        const uint64_t u = (b >> us) + (w - bases[j]);
        const uint64_t ustart = u << us, uend = ustart + U;
        const uint64_t first = b > ustart ? b : ustart;
        const uint64_t last = e < uend ? e : uend;
        Start at;
        fmt.locate(p, u, ustart, uend, last, at);
        if (at.exact) at.corrupt |= at.next < at.s || at.next > p.nbits;
        if (at.corrupt) { item_fail(p.status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        if (at.s < win_lo || Format::lim(p, at.s, at.next, at.exact) > win_hi) { item_fail(p.status, status, j, MH_ERR_ARG, BATCH_STATUS_ARG); continue; }
        BitCursor bc;
        bc.init(src, bit0 + (at.s - win_lo));
        uint32_t used = 0;
        bool bad = false;
        decode_share(tb, p, src, bc, at.ctx, uint32_t(first - at.s_sym), uint32_t(last - first), j, first - b, used, bad);
        if (bad || at.s + used > p.nbits || (at.exact && used != at.next - at.s)) item_fail(p.status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
        else if (Format::JUDGES_OVERRUN && at.s + used > win_hi) item_fail(p.status, status, j, MH_ERR_ARG, BATCH_STATUS_ARG);
    }
}

// ------------------------------------------------------------------------------------------------ batch lookups

template <typename Tables, bool INDEXED>
__global__ __launch_bounds__(Tables::BOUND) void lookup_kernel(LookupParams p, const unsigned long long *bases, int *status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Tables tb;
    tb.init(p, smem);
    const uint64_t total = bases[p.n];
    const uint32_t cs = p.chunk_shift;
    const uint64_t U = uint64_t(1) << cs;
    for (uint64_t w = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < total; w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t j = item_of(bases, p.n, w);
        const uint64_t i = p.lookups[3 * j], b = p.lookups[3 * j + 1], e = p.lookups[3 * j + 2];
        const uint64_t nb = p.nbits[i];
        tb.stream(p, i);
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.payload, p.pay_off[i], nb, bit0);
        BitCursor bc;
        uint32_t ctx, used = 0;
        bool bad = false;
        if (INDEXED) {
            const uint64_t ni = p.sym_off[i + 1] - p.sym_off[i];
            const uint64_t c = (b >> cs) + (w - bases[j]);                 // chunk of stream i
            const uint64_t g = (p.sym_off[i] >> cs) + i + c;                // its entry in the batch index
            const uint64_t nchunks = (ni + U - 1) >> cs;
            const uint64_t ustart = c << cs;
            const uint64_t first = b > ustart ? b : ustart;
            const uint64_t last = e < ustart + U ? e : ustart + U;
            const uint64_t ent = p.index[g];
            const uint64_t s = ent & Tables::POS;
            bool corrupt = s > nb || (c > 0 && s < (p.index[g - 1] & Tables::POS));
            // an item that ends on a chunk boundary must use exactly the bits up to the next entry (nbits after the last symbol)
            const bool exact = last == ustart + U || last == ni;
            const uint64_t next = last == ni ? nb : (c + 1 < nchunks ? (p.index[g + 1] & Tables::POS) : nb);
            if (exact) corrupt |= next < s || next > nb;
            if (corrupt) { item_fail(p.status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
            bc.init(src, bit0 + s);
            ctx = Tables::entry_ctx(ent);
            decode_share(tb, p, src, bc, ctx, uint32_t(first - ustart), uint32_t(last - first), j, first - b, used, bad);
            if (bad || s + used > nb || (exact && used != next - s)) item_fail(p.status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
        } else {
            // one lane walks the stream from bit 0 in context prev0, which the call gave the model's width (nb <= walk_max_bits
            // < 2^32: the count kernel refused longer streams)
            bc.init(src, bit0);
            ctx = p.prev0;
            uint64_t t = 0;
            for (; t < b && !bad && used < nb; ++t) tb.next(p, src, bc, ctx, used, bad);
            mhb::ByteOut bo;
            bo.init(p.out, p.out_at[j]);
            if (t == b)
                for (; t < e && !bad && used < nb; ++t) bo.put(tb.next(p, src, bc, ctx, used, bad));
            bo.flush();
            if (bad || used > nb) item_fail(p.status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
            else if (t < e) item_fail(p.status, status, j, MH_ERR_ARG, BATCH_STATUS_ARG);          // the stream ends before `end`
            else if (p.sym_off && e == p.sym_off[i + 1] - p.sym_off[i] && used != nb)          // src/coding.cpp:124,158
                item_fail(p.status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
        }
    }
}

// ------------------------------------------------------------------------------------------------ launches

// status block cleared, counts, scan: the item bases in the workspace
template <typename Params>
hipError_t count_and_scan(const Params &p, void *d_ws, hipStream_t st, unsigned long long *&bases, int *&status) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const RangeLayout L = range_layout(p.n);
    status = reinterpret_cast<int *>(ws);
    int *stop = status + 1;                                                     // (stays 0: the scan runs unconditionally)
    bases = reinterpret_cast<unsigned long long *>(ws + L.off_bases);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess || p.n == 0) return e;
    hipLaunchKernelGGL(count_kernel<Params>, dim3(uint32_t((p.n + 1 + 255) / 256)), dim3(256), 0, st, p, bases, status);
    return mhb::scan_exclusive(bases, p.n + 1, sums, stop, st);
}

template <typename Format>
hipError_t launch_range(const RangeParams &p, void *d_ws, hipStream_t st) {
    using Tables = typename Format::Tables;
    size_t lds;
    hipError_t e = tables_room<Tables>(p, {reinterpret_cast<const void *>(range_kernel<Format>)}, lds);
    if (e != hipSuccess) return e;
    unsigned long long *bases;
    int *status;
    e = count_and_scan(p, d_ws, st, bases, status);
    if (e != hipSuccess || p.n == 0) return e;
    // the item total is on the device: the grid covers the most items the ranges can have (every range touches at most
    // n_units units), capped at what the device holds as grid_for does; surplus workgroups find no item
    const uint64_t nu = p.n_units ? p.n_units : 1, many = uint64_t(1) << 40;
    const uint64_t items = p.n > many / nu ? many : p.n * nu;
    hipLaunchKernelGGL(range_kernel<Format>, dim3(mhb::grid_for(items, Tables::BOUND, Tables::PER_CU)), dim3(Tables::BOUND), lds, st, p, bases,
                       status);
    return hipGetLastError();
}

template <typename Tables>
hipError_t launch_lookup(const LookupParams &p, void *d_ws, hipStream_t st) {
    size_t lds;
    hipError_t e = tables_room<Tables>(p, {reinterpret_cast<const void *>(lookup_kernel<Tables, true>),
                                           reinterpret_cast<const void *>(lookup_kernel<Tables, false>)}, lds);
    if (e != hipSuccess) return e;
    unsigned long long *bases;
    int *status;
    e = count_and_scan(p, d_ws, st, bases, status);
    if (e != hipSuccess || p.n == 0) return e;
    const int threads = Tables::LDS && p.n >= uint64_t(mhk::cu_count()) * SPREAD ? Tables::BOUND : 256;
    // the item total is on the device: with an index a lookup may touch any number of chunks, so the grid covers the device
    // (grid_for's cap) and surplus lanes find no item; without one there is exactly one item per lookup at most
    if (p.index)
        hipLaunchKernelGGL((lookup_kernel<Tables, true>), dim3(mhb::grid_for(uint64_t(1) << 40, uint64_t(threads), Tables::PER_CU)), dim3(threads),
                           lds, st, p, bases, status);
    else
        hipLaunchKernelGGL((lookup_kernel<Tables, false>), dim3(mhb::grid_for(p.n, uint64_t(threads), Tables::PER_CU)), dim3(threads), lds, st, p,
                           bases, status);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ranges(const RangeParams &p, Model model, void *d_ws, hipStream_t st) {
    switch (model) {
    case Model::Shared: return launch_range<Format01>(p, d_ws, st);
    case Model::Shared2: return launch_range<Format2>(p, d_ws, st);
    default: return hipErrorInvalidValue;                       // (a single stream has no model set)
    }
}

hipError_t launch_lookups(const LookupParams &p, Model model, void *d_ws, hipStream_t st) {
    switch (model) {
    case Model::Shared: return launch_lookup<SharedTables>(p, d_ws, st);
    case Model::Set: return launch_lookup<SetTables>(p, d_ws, st);
    case Model::Shared2: return launch_lookup<Shared2Tables>(p, d_ws, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mhq
