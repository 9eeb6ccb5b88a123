// mh_range.hip — byte ranges of one indexed order-0/1 stream (include/mh.h, "RANDOM ACCESS: BYTE RANGES OF AN INDEXED STREAM").
// A work unit is a chunk of the chunk index, or a piece of MH_FINE_SYMBOLS symbols when the fine index is given.  An item is
// one (range, unit) pair: the symbols of the unit that lie in the range.
//   range_count_kernel    one thread per range: checks it and writes the number of units it touches (0: empty or refused)
//   batch_scan_*          exclusive scan of the counts: item bases, entry n = the item total
//   range_decode_kernel   one lane per item on a grid-stride loop up to the total (read on the device): the lane starts at the
//                         unit's index entry, decodes the symbols in front of the range without storing them, then stores its
//                         share of the range through ByteOut
// The table loader, the bit source of a window, ByteOut and the scan are the batch decoder's (mh_batch_dev.hpp), used as they are.
#include "mh_range.h"
#include "mh_batch_dev.hpp"
#include "mh_decode_dev.hpp"
#include "mh_dev.hpp"
#include "../../include/mh.h"

namespace mhr {

using mhb::B_THREADS;
using mhb::BATCH_STATUS_ARG;
using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;

namespace {

__device__ __forceinline__ void range_fail(const RangeParams &p, int *status, uint64_t j, int mh_code, int dev_code) {
    atomicCAS(&p.range_status[j], MH_OK, mh_code);
    mhb::fail(status, dev_code);
}

// start state of unit u: payload bit offset from the stream start, and the context byte in front of it.  With a fine index
// the entry holds the low 24 bits of the offset; its chunk's entry supplies the rest (a chunk spans fewer than 2^24 bits).
__device__ __forceinline__ uint64_t unit_pos(const RangeParams &p, uint64_t u, uint32_t &ctx) {
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

__global__ void range_count_kernel(RangeParams p, unsigned long long *bases, int *status) {
    const uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j > p.n) return;
    if (j == p.n) { bases[j] = 0; return; }
    const uint64_t b = p.ranges[2 * j], e = p.ranges[2 * j + 1];
    int st = MH_OK;
    uint64_t cnt = 0;
    if (b > e || e > p.n_symbols) st = MH_ERR_ARG;
    else if (b < e) {
        const uint64_t at = p.out_at[j];
        if (at > p.out_cap || e - b > p.out_cap - at) st = MH_ERR_CAPACITY;
        else cnt = ((e - 1) >> p.unit_shift) - (b >> p.unit_shift) + 1;
    }
    p.range_status[j] = st;
    bases[j] = cnt;
    if (st != MH_OK) mhb::fail(status, st == MH_ERR_ARG ? BATCH_STATUS_ARG : mhk::MHK_STATUS_CAPACITY);
}

__global__ __launch_bounds__(B_THREADS) void range_decode_kernel(RangeParams p, const unsigned long long *bases, int *status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint16_t *lut; const uint32_t *sub_base;
    const DecTables tabs = mhb::load_tables(p.tab, smem, lut, sub_base);
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
        // the range of item w: the largest j with bases[j] <= w (ranges without items share their successor's base)
        uint64_t lo = 0, hi = p.n - 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (bases[mid] <= w) lo = mid; else hi = mid - 1;
        }
        const uint64_t j = lo;
        const uint64_t b = p.ranges[2 * j], e = p.ranges[2 * j + 1];
        const uint64_t u = (b >> us) + (w - bases[j]);
        const uint64_t ustart = u << us;
        const uint64_t first = b > ustart ? b : ustart;
        const uint64_t last = e < ustart + U ? e : ustart + U;
        uint32_t ctx, pctx;
        const uint64_t s = unit_pos(p, u, ctx);
        bool corrupt = s > p.nbits || (u > 0 && s < unit_pos(p, u - 1, pctx));
        // an item that ends on a unit boundary must use exactly the bits up to the next entry (nbits after the last symbol)
        const bool exact = last == ustart + U || last == p.n_symbols;
        const uint64_t next = last == p.n_symbols ? p.nbits : (u + 1 < p.n_units ? unit_pos(p, u + 1, pctx) : p.nbits);
        if (exact) corrupt |= next < s || next > p.nbits;
        if (corrupt) { range_fail(p, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        const uint64_t lim = (next >= s && next <= p.nbits) ? next : s;
        if (s < win_lo || lim > win_hi) { range_fail(p, status, j, MH_ERR_ARG, BATCH_STATUS_ARG); continue; }
        BitCursor bc;
        bc.init(src, bit0 + (s - win_lo));
        uint32_t prev = ctx, used = 0;
        bool bad = false;
        const uint32_t skip = uint32_t(first - ustart), store = uint32_t(last - first);
        for (uint32_t t = 0; t < skip && !bad; ++t) prev = mhk::decode_one(lut, sub_base, tabs, src, bc, prev, used, bad);
        mhb::ByteOut bo;
        bo.init(p.out, p.out_at[j] + (first - b));
        for (uint32_t t = 0; t < store && !bad; ++t) {
            prev = mhk::decode_one(lut, sub_base, tabs, src, bc, prev, used, bad);
            bo.put(prev);
        }
        bo.flush();
        if (bad || s + used > p.nbits || (exact && used != next - s)) range_fail(p, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
    }
}

}  // namespace

hipError_t launch_decode_ranges(const RangeParams &p, void *d_ws, hipStream_t st) {
    const int lds_max = 163840;
    hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(range_decode_kernel), lds_max);
    if (attr != hipSuccess) return attr;
    const size_t lds = mhb::tables_lds(p.tab);
    if (lds > size_t(lds_max)) return hipErrorInvalidValue;
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const RangeLayout L = range_layout(p.n);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;            // (stop stays 0: the scan runs unconditionally)
    auto *bases = reinterpret_cast<unsigned long long *>(ws + L.off_bases);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess || p.n == 0) return e;
    hipLaunchKernelGGL(range_count_kernel, dim3(uint32_t((p.n + 1 + 255) / 256)), dim3(256), 0, st, p, bases, status);
    if ((e = mhb::scan_exclusive(bases, p.n + 1, sums, stop, st)) != hipSuccess) return e;
    // the item total is on the device: the grid covers the most items the ranges can have (every range touches at most
    // n_units units), capped at what the device holds as grid_for does; surplus workgroups find no item
    const uint64_t nu = p.n_units ? p.n_units : 1, many = uint64_t(1) << 40;
    const uint64_t items = p.n > many / nu ? many : p.n * nu;
    hipLaunchKernelGGL(range_decode_kernel, dim3(mhb::grid_for(items, B_THREADS, 1)), dim3(B_THREADS), lds, st, p, bases, status);
    return hipGetLastError();
}

}  // namespace mhr
