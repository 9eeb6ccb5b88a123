// mh_batch_range.hip — lookups (stream, begin, end) into a batch of order-0/1 streams (include/mh.h, "RANDOM ACCESS INTO
// BATCHES"), under one shared model or one model per stream.  With a chunk index the work unit is a chunk of the stream's
// slice; without one it is the whole stream, walked by one lane from bit 0.  An item is one (lookup, unit) pair.
//   batch_range_count_kernel    one thread per lookup: checks it and the offsets of its stream, writes its status and the
//                               number of units it touches (0: empty or refused)
//   batch_scan_*                exclusive scan of the counts: item bases, entry m = the item total
//   batch_range_decode_kernel   one lane per item on a grid-stride loop up to the total (read on the device): the lane starts
//                               at the unit's index entry (or at bit 0 in context prev0), decodes the symbols in front of the
//                               lookup without storing them, then stores its share through ByteOut
// Only the offsets of the streams a lookup names are read, so the cost does not depend on the batch's stream count.  The
// shared model's tables go to LDS (mh_range.hip's loader); a set's tables stay in L2 (mh_each.hip's decode_sym).
#include "mh_batch_range.h"
#include "mh_batch_dev.hpp"
#include "mh_decode_dev.hpp"
#include "mh_dev.hpp"
#include "mh_each_dev.hpp"
#include "../../include/mh.h"

namespace mhq {

using mhb::BATCH_STATUS_ARG;
using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;

namespace {

// The LDS tables take up to 160 KiB: one workgroup per CU.  Below SPREAD lookups per CU the shared-model decoder runs 256-lane
// workgroups instead, so that its lanes spread over four times as many CUs (measured on an MI355X: 3-23 % faster at 1 K-16 K
// lookups, the same above).
constexpr int SHARED_THREADS = 1024;
constexpr uint64_t SPREAD = 256;
constexpr int SET_THREADS = 256;         // no LDS: eight workgroups per CU, as mh_each.hip's decoders

__device__ __forceinline__ void lookup_fail(const BatchRangeParams &p, int *status, uint64_t j, int mh_code, int dev_code) {
    atomicCAS(&p.lookup_status[j], MH_OK, mh_code);
    mhb::fail(status, dev_code);
}

// the shared model: LDS tables, one context table per byte (order 0: the same table 256 times)
struct SharedTables {
    const uint16_t *lut;
    const uint32_t *sub_base;
    DecTables tabs;
    __device__ __forceinline__ void init(const BatchRangeParams &p, unsigned char *smem) { tabs = mhb::load_tables(p.tab, smem, lut, sub_base); }
    __device__ __forceinline__ void stream(const BatchRangeParams &, uint64_t) {}
    __device__ __forceinline__ uint32_t next(const BatchRangeParams &, const BitSrc &src, BitCursor &bc, uint32_t prev, uint32_t &used, bool &bad) const {
        return mhk::decode_one(lut, sub_base, tabs, src, bc, prev, used, bad);
    }
};

// the set's model of stream i: its context -> slot row and its order, tables in L2
struct SetTables {
    const uint32_t *row;
    bool o1;
    __device__ __forceinline__ void init(const BatchRangeParams &, unsigned char *) {}
    __device__ __forceinline__ void stream(const BatchRangeParams &p, uint64_t i) { row = p.set.ctx_slot + i * 256u; o1 = p.set.type[i] != 0; }
    __device__ __forceinline__ uint32_t next(const BatchRangeParams &p, const BitSrc &src, BitCursor &bc, uint32_t prev, uint32_t &used, bool &bad) const {
        return mhe::decode_sym(p.set, row, o1 ? prev : 0u, src, bc, used, bad);
    }
};

__global__ void batch_range_count_kernel(BatchRangeParams p, unsigned long long *bases, int *status) {
    const uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j > p.m) return;
    if (j == p.m) { bases[j] = 0; return; }
    const uint64_t i = p.lookups[3 * j], b = p.lookups[3 * j + 1], e = p.lookups[3 * j + 2];
    int st = MH_OK;
    uint64_t cnt = 0;
    if (i >= p.n || b > e) st = MH_ERR_ARG;
    else {
        const uint64_t p0 = p.pay_off[i], p1 = p.pay_off[i + 1], nb = p.nbits[i];
        if (p1 < p0 || nb > (p1 - p0) * 8u) st = MH_ERR_ARG;
        if (st == MH_OK && p.sym_off) {
            const uint64_t s0 = p.sym_off[i], s1 = p.sym_off[i + 1];
            if (s1 < s0 || e > s1 - s0) st = MH_ERR_ARG;
        }
        if (e > nb && !p.sym_off) st = MH_ERR_ARG;            // every code has at least one bit: n_i <= nbits_i
        if (st == MH_OK && b < e) {
            const uint64_t at = p.out_at[j];
            if (at > p.out_cap || e - b > p.out_cap - at) st = MH_ERR_CAPACITY;
            else if (p.index) cnt = ((e - 1) >> p.chunk_shift) - (b >> p.chunk_shift) + 1;
            else if (nb > p.walk_max_bits) st = MH_ERR_ARG;
            else cnt = 1;
        }
    }
    p.lookup_status[j] = st;
    bases[j] = cnt;
    if (st != MH_OK) mhb::fail(status, st == MH_ERR_ARG ? BATCH_STATUS_ARG : mhk::MHK_STATUS_CAPACITY);
}

template <typename Tables, bool INDEXED>
__global__ __launch_bounds__(1024) void batch_range_decode_kernel(BatchRangeParams p, const unsigned long long *bases, int *status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Tables tb;
    tb.init(p, smem);
    const uint64_t total = bases[p.m];
    const uint32_t cs = p.chunk_shift;
    const uint64_t U = uint64_t(1) << cs;
    for (uint64_t w = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < total; w += uint64_t(gridDim.x) * blockDim.x) {
        // the lookup of item w: the largest j with bases[j] <= w (lookups without items share their successor's base)
        uint64_t lo = 0, hi = p.m - 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (bases[mid] <= w) lo = mid; else hi = mid - 1;
        }
        const uint64_t j = lo;
        const uint64_t i = p.lookups[3 * j], b = p.lookups[3 * j + 1], e = p.lookups[3 * j + 2];
        const uint64_t nb = p.nbits[i];
        tb.stream(p, i);
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.payload, p.pay_off[i], nb, bit0);
        BitCursor bc;
        uint32_t prev, used = 0;
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
            const uint64_t s = ent & MH_INDEX_BIT_MASK;
            bool corrupt = s > nb || (c > 0 && s < (p.index[g - 1] & MH_INDEX_BIT_MASK));
            // an item that ends on a chunk boundary must use exactly the bits up to the next entry (nbits after the last symbol)
            const bool exact = last == ustart + U || last == ni;
            const uint64_t next = last == ni ? nb : (c + 1 < nchunks ? (p.index[g + 1] & MH_INDEX_BIT_MASK) : nb);
            if (exact) corrupt |= next < s || next > nb;
            if (corrupt) { lookup_fail(p, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
            bc.init(src, bit0 + s);
            prev = uint32_t(ent >> 56);
            const uint32_t skip = uint32_t(first - ustart), store = uint32_t(last - first);
            for (uint32_t t = 0; t < skip && !bad; ++t) prev = tb.next(p, src, bc, prev, used, bad);
            bo.init(p.out, p.out_at[j] + (first - b));
            for (uint32_t t = 0; t < store && !bad; ++t) {
                prev = tb.next(p, src, bc, prev, used, bad);
                bo.put(prev);
            }
            bo.flush();
            if (bad || s + used > nb || (exact && used != next - s)) lookup_fail(p, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
        } else {
            // one lane walks the stream from bit 0 (nb <= walk_max_bits < 2^32: the count kernel refused longer streams)
            bc.init(src, bit0);
            prev = p.prev0;
            uint64_t t = 0;
            for (; t < b && !bad && used < nb; ++t) prev = tb.next(p, src, bc, prev, used, bad);
            bo.init(p.out, p.out_at[j]);
            if (t == b)
                for (; t < e && !bad && used < nb; ++t) {
                    prev = tb.next(p, src, bc, prev, used, bad);
                    bo.put(prev);
                }
            bo.flush();
            if (bad || used > nb) lookup_fail(p, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
            else if (t < e) lookup_fail(p, status, j, MH_ERR_ARG, BATCH_STATUS_ARG);          // the stream ends before `end`
            else if (p.sym_off && e == p.sym_off[i + 1] - p.sym_off[i] && used != nb)      // src/coding.cpp:124,158
                lookup_fail(p, status, j, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
        }
    }
}

template <typename Tables, bool INDEXED>
hipError_t launch_decode(const BatchRangeParams &p, int threads, int per_cu, size_t lds, const unsigned long long *bases, int *status,
                         hipStream_t st) {
    // the item total is on the device: with an index a lookup may touch any number of chunks, so the grid covers the device
    // (grid_for's cap) and surplus lanes find no item; without one there is exactly one item per lookup at most
    const uint64_t many = uint64_t(1) << 40;
    const uint64_t items = INDEXED ? many : p.m;
    hipLaunchKernelGGL((batch_range_decode_kernel<Tables, INDEXED>), dim3(mhb::grid_for(items, uint64_t(threads), per_cu)), dim3(threads), lds,
                       st, p, bases, status);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_batch_ranges(const BatchRangeParams &p, bool shared, void *d_ws, hipStream_t st) {
    const int lds_max = 163840;
    size_t lds = 0;
    if (shared) {
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(batch_range_decode_kernel<SharedTables, true>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(batch_range_decode_kernel<SharedTables, false>), lds_max);
        if (attr != hipSuccess) return attr;
        lds = mhb::tables_lds(p.tab);
        if (lds > size_t(lds_max)) return hipErrorInvalidValue;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const mhr::RangeLayout L = mhr::range_layout(p.m);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;            // (stop stays 0: the scan runs unconditionally)
    auto *bases = reinterpret_cast<unsigned long long *>(ws + L.off_bases);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess || p.m == 0) return e;
    hipLaunchKernelGGL(batch_range_count_kernel, dim3(uint32_t((p.m + 1 + 255) / 256)), dim3(256), 0, st, p, bases, status);
    if ((e = mhb::scan_exclusive(bases, p.m + 1, sums, stop, st)) != hipSuccess) return e;
    if (shared) {
        const int threads = p.m < uint64_t(mhk::cu_count()) * SPREAD ? 256 : SHARED_THREADS;
        return p.index ? launch_decode<SharedTables, true>(p, threads, 1, lds, bases, status, st)
                       : launch_decode<SharedTables, false>(p, threads, 1, lds, bases, status, st);
    }
    return p.index ? launch_decode<SetTables, true>(p, SET_THREADS, 8, 0, bases, status, st)
                   : launch_decode<SetTables, false>(p, SET_THREADS, 8, 0, bases, status, st);
}

}  // namespace mhq
