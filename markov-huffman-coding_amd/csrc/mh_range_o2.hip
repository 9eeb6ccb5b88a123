// mh_range_o2.hip — random access into order-2 streams (include/mh.h, "RANDOM ACCESS INTO ORDER-2 STREAMS"; extension,
// parity unpinned): byte ranges of one indexed stream, and lookups (stream, begin, end) into a batch under one shared order-2
// model.  A work unit is a chunk of the chunk index, or a piece of MH_FINE_SYMBOLS symbols when the fine index is given
// (single stream); without a batch index it is the whole stream, walked by one lane from bit 0.  An item is one
// (range or lookup, unit) pair.
//   range2_count_kernel    one thread per range or lookup: checks it and writes the number of units it touches (0: empty or
//                          refused)
//   batch_scan_*           exclusive scan of the counts: item bases, entry n = the item total
//   range2_decode_kernel   one lane per item on a grid-stride loop up to the total (read on the device): the lane starts at
//                          the unit's entry in its 16-bit context (or at the nearest earlier usable piece of the same chunk,
//                          or at the chunk's entry), decodes the symbols in front of the range without storing them, then
//                          stores its share through ByteOut
//   batch2_lookup_kernel   the same over pay_off / nbits / sym_off / index slices, or one lane per lookup walking an
//                          index-free stream from bit 0 in context (prev0, prev0)
// The decode tables are the model's order-2 tables in L2 as batch2_dec_idx_kernel reads them (65 536 contexts: no LDS copy);
// a lane is a chain of dependent gathers, so the unit size sets the latency.  The scan, the bit source of a window and
// ByteOut are mh_batch_dev.hpp's, used as they are.
#include "mh_range_o2.h"
#include "mh_batch_dev.hpp"
#include "mh_decode_dev.hpp"
#include "mh_dev.hpp"
#include "../../include/mh.h"

namespace mhr {

using mhb::BATCH_STATUS_ARG;
using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;
using mhk::IDX2_POS;

namespace {

constexpr int R2_THREADS = 256;                     // no tables in LDS: small workgroups, many waves per CU for the L2 gathers
constexpr uint32_t FINE2_NONE = 0xFFFFu;            // an order-2 fine entry whose distance does not fit 16 bits

__device__ __forceinline__ void item_fail(int32_t *item_status, int *status, uint64_t j, int mh_code, int dev_code) {
    atomicCAS(&item_status[j], MH_OK, mh_code);
    mhb::fail(status, dev_code);
}

// the model's order-2 tables as batch2_dec_idx_kernel reads them: general form, every level gathered from L2
__device__ __forceinline__ DecTables tables2(const mhb::DecBatchParams &t) { return DecTables{t.sec, t.tree, t.P, 0u, 0u}; }

// one symbol in 16-bit context ctx, which then advances (a pair without a code is a null entry: bad)
__device__ __forceinline__ uint32_t next2(const mhb::DecBatchParams &t, const DecTables &tabs, const BitSrc &src, BitCursor &bc,
                                          uint32_t &ctx, uint32_t &used, bool &bad) {
    const uint32_t sym = mhk::decode_one(t.prim, t.sec_base, tabs, src, bc, ctx, used, bad);
    ctx = ((ctx << 8) | sym) & 0xFFFFu;
    return sym;
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

// lookup j into a batch: the checks of the order-0/1 batch lookups (batch_range_count_kernel)
__device__ __forceinline__ int check_item(const mhq::BatchRangeParams &p, uint64_t j, uint64_t &cnt) {
    const uint64_t i = p.lookups[3 * j], b = p.lookups[3 * j + 1], e = p.lookups[3 * j + 2];
    cnt = 0;
    if (i >= p.n || b > e) return MH_ERR_ARG;
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

__device__ __forceinline__ uint64_t items_of(const RangeParams &p) { return p.n; }
__device__ __forceinline__ uint64_t items_of(const mhq::BatchRangeParams &p) { return p.m; }
__device__ __forceinline__ int32_t *status_of(const RangeParams &p) { return p.range_status; }
__device__ __forceinline__ int32_t *status_of(const mhq::BatchRangeParams &p) { return p.lookup_status; }

template <typename Params>
__global__ void range2_count_kernel(Params p, unsigned long long *bases, int *status) {
    const uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t n = items_of(p);
    if (j > n) return;
    if (j == n) { bases[j] = 0; return; }
    uint64_t cnt;
    const int st = check_item(p, j, cnt);
    status_of(p)[j] = st;
    bases[j] = cnt;
    if (st != MH_OK) mhb::fail(status, st == MH_ERR_ARG ? BATCH_STATUS_ARG : mhk::MHK_STATUS_CAPACITY);
}

// the item of w: the largest j with bases[j] <= w (items without units share their successor's base)
__device__ __forceinline__ uint64_t item_of(const unsigned long long *bases, uint64_t n, uint64_t w) {
    uint64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (bases[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------ one stream

__global__ __launch_bounds__(R2_THREADS) void range2_decode_kernel(RangeParams p, const unsigned long long *bases, int *status) {
    const DecTables tabs = tables2(p.tab);
    const uint64_t total = bases[p.n];
    const uint32_t us = p.unit_shift, cs = p.chunk_shift;
    const uint64_t U = uint64_t(1) << us, C = uint64_t(1) << cs;
    const uint64_t nchunks = (p.n_symbols + C - 1) >> cs;
    // the window as a bit source: reads stay inside the aligned dwords that hold its bytes
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
        // the unit's chunk and its span [cpos, chi]
        const uint64_t c = ustart >> cs;
        const uint64_t ce = p.index[c], cpos = ce & IDX2_POS;
        const uint64_t cnext = c + 1 < nchunks ? (p.index[c + 1] & IDX2_POS) : p.nbits;
        const uint64_t chi = cnext < p.nbits ? cnext : p.nbits;
        bool corrupt = cpos > p.nbits || (c > 0 && cpos < (p.index[c - 1] & IDX2_POS));
        // start: the unit's own fine entry, the nearest earlier usable piece of the chunk, or the chunk's entry
        uint64_t s = cpos, s_sym = c << cs;
        uint32_t ctx = uint32_t(ce >> 48);
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
        if (exact) corrupt |= next < s || next > p.nbits;
        if (corrupt) { item_fail(p.range_status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        const uint64_t lim = exact ? next : s;
        if (s < win_lo || lim > win_hi) { item_fail(p.range_status, status, j, MH_ERR_ARG, BATCH_STATUS_ARG); continue; }
        BitCursor bc;
        bc.init(src, bit0 + (s - win_lo));
        uint32_t used = 0;
        bool bad = false;
        const uint32_t skip = uint32_t(first - s_sym), store = uint32_t(last - first);
        for (uint32_t t = 0; t < skip && !bad; ++t) next2(p.tab, tabs, src, bc, ctx, used, bad);
        mhb::ByteOut bo;
        bo.init(p.out, p.out_at[j] + (first - b));
        for (uint32_t t = 0; t < store && !bad; ++t) bo.put(next2(p.tab, tabs, src, bc, ctx, used, bad));
        bo.flush();
        if (bad || s + used > p.nbits || (exact && used != next - s)) item_fail(p.range_status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
        else if (s + used > win_hi) item_fail(p.range_status, status, j, MH_ERR_ARG, BATCH_STATUS_ARG);   // read past the window
    }
}

// ------------------------------------------------------------------------------------------------ batch lookups

template <bool INDEXED>
__global__ __launch_bounds__(R2_THREADS) void batch2_lookup_kernel(mhq::BatchRangeParams p, const unsigned long long *bases, int *status) {
    const DecTables tabs = tables2(p.tab);
    const uint64_t total = bases[p.m];
    const uint32_t cs = p.chunk_shift;
    const uint64_t U = uint64_t(1) << cs;
    for (uint64_t w = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < total; w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t j = item_of(bases, p.m, w);
        const uint64_t i = p.lookups[3 * j], b = p.lookups[3 * j + 1], e = p.lookups[3 * j + 2];
        const uint64_t nb = p.nbits[i];
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.payload, p.pay_off[i], nb, bit0);
        BitCursor bc;
        uint32_t used = 0;
        bool bad = false;
        mhb::ByteOut bo;
        if (INDEXED) {
            const uint64_t ni = p.sym_off[i + 1] - p.sym_off[i];
            const uint64_t c = (b >> cs) + (w - bases[j]);                 // chunk of stream i
            const uint64_t g = (p.sym_off[i] >> cs) + i + c;                // its entry in the batch index
            const uint64_t nchunks = (ni + U - 1) >> cs;
            const uint64_t ustart = c << cs;
            const uint64_t first = b > ustart ? b : ustart;
            const uint64_t last = e < ustart + U ? e : ustart + U;
            const uint64_t ent = p.index[g];
            const uint64_t s = ent & IDX2_POS;
            bool corrupt = s > nb || (c > 0 && s < (p.index[g - 1] & IDX2_POS));
            const bool exact = last == ustart + U || last == ni;
            const uint64_t next = last == ni ? nb : (c + 1 < nchunks ? (p.index[g + 1] & IDX2_POS) : nb);
            if (exact) corrupt |= next < s || next > nb;
            if (corrupt) { item_fail(p.lookup_status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
            bc.init(src, bit0 + s);
            uint32_t ctx = uint32_t(ent >> 48);
            const uint32_t skip = uint32_t(first - ustart), store = uint32_t(last - first);
            for (uint32_t t = 0; t < skip && !bad; ++t) next2(p.tab, tabs, src, bc, ctx, used, bad);
            bo.init(p.out, p.out_at[j] + (first - b));
            for (uint32_t t = 0; t < store && !bad; ++t) bo.put(next2(p.tab, tabs, src, bc, ctx, used, bad));
            bo.flush();
            if (bad || s + used > nb || (exact && used != next - s)) item_fail(p.lookup_status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
        } else {
            // one lane walks the stream from bit 0 in context (prev0, prev0) (nb <= walk_max_bits: the count kernel refused
            // longer streams)
            bc.init(src, bit0);
            uint32_t ctx = p.prev0;
            uint64_t t = 0;
            for (; t < b && !bad && used < nb; ++t) next2(p.tab, tabs, src, bc, ctx, used, bad);
            bo.init(p.out, p.out_at[j]);
            if (t == b)
                for (; t < e && !bad && used < nb; ++t) bo.put(next2(p.tab, tabs, src, bc, ctx, used, bad));
            bo.flush();
            if (bad || used > nb) item_fail(p.lookup_status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
            else if (t < e) item_fail(p.lookup_status, status, j, MH_ERR_ARG, BATCH_STATUS_ARG);          // the stream ends before `end`
            else if (p.sym_off && e == p.sym_off[i + 1] - p.sym_off[i] && used != nb)                     // src/coding.cpp:124,158
                item_fail(p.lookup_status, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
        }
    }
}

// status block cleared, counts, scan: the item bases in the workspace (mh_range.h's layout)
template <typename Params>
hipError_t count_and_scan(const Params &p, uint64_t n, void *d_ws, hipStream_t st, unsigned long long *&bases, int *&status) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const RangeLayout L = range_layout(n);
    status = reinterpret_cast<int *>(ws);
    int *stop = status + 1;                                                     // (stays 0: the scan runs unconditionally)
    bases = reinterpret_cast<unsigned long long *>(ws + L.off_bases);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(range2_count_kernel<Params>, dim3(uint32_t((n + 1 + 255) / 256)), dim3(256), 0, st, p, bases, status);
    return mhb::scan_exclusive(bases, n + 1, sums, stop, st);
}

}  // namespace

hipError_t launch_decode_ranges_o2(const RangeParams &p, void *d_ws, hipStream_t st) {
    unsigned long long *bases;
    int *status;
    hipError_t e = count_and_scan(p, p.n, d_ws, st, bases, status);
    if (e != hipSuccess || p.n == 0) return e;
    // the item total is on the device: the grid covers the most items the ranges can have, capped at what the device holds
    // as grid_for does; surplus workgroups find no item
    const uint64_t nu = p.n_units ? p.n_units : 1, many = uint64_t(1) << 40;
    const uint64_t items = p.n > many / nu ? many : p.n * nu;
    hipLaunchKernelGGL(range2_decode_kernel, dim3(mhb::grid_for(items, R2_THREADS, 8)), dim3(R2_THREADS), 0, st, p, bases, status);
    return hipGetLastError();
}

hipError_t launch_batch_ranges_o2(const mhq::BatchRangeParams &p, void *d_ws, hipStream_t st) {
    unsigned long long *bases;
    int *status;
    hipError_t e = count_and_scan(p, p.m, d_ws, st, bases, status);
    if (e != hipSuccess || p.m == 0) return e;
    // with an index a lookup may touch any number of chunks (the grid covers the device); without one, one item per lookup
    if (p.index)
        hipLaunchKernelGGL(batch2_lookup_kernel<true>, dim3(mhb::grid_for(uint64_t(1) << 40, R2_THREADS, 8)), dim3(R2_THREADS), 0, st, p,
                           bases, status);
    else
        hipLaunchKernelGGL(batch2_lookup_kernel<false>, dim3(mhb::grid_for(p.m, R2_THREADS, 8)), dim3(R2_THREADS), 0, st, p, bases, status);
    return hipGetLastError();
}

}  // namespace mhr
