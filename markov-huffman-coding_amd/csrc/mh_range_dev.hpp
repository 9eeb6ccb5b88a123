// mh_range_dev.hpp — what a kernel file needs to decode from an arbitrary place of a batch, one lane per item: the symbol
// decoders of a lane (one policy per model kind), the item search and the LDS room of a policy's kernels.  Written for the
// random-access kernels (mh_range.hip) and used as they are by the span tokens (mh_token.hip); kernel files only.
//   Tables   the symbol decoder of a lane, one policy per model (mhb::Model).  SharedTables: the order-0/1 tables in LDS as
//            load_tables lays them out, one workgroup per CU.  SetTables: stream i's slots in L2 (mh_each.hip's decode_sym).
//            Shared2Tables: the model's order-2 tables in L2 as dec_idx_kernel<Shared2> reads them (65 536 contexts: no LDS
//            copy; a lane is a chain of dependent gathers, so the unit size sets the latency).  Set and Shared2: workgroups of
//            256 lanes, eight per CU.  A policy also names the format of an index entry (POS, entry_ctx) and the bound its
//            kernels compile under.
// The bit source of a stream (mhb::stream_src) and the scan are mh_batch_dev.hpp's, which this header includes.
#pragma once

#include "mh_range.h"
#include "mh_batch_dev.hpp"
#include "mh_decode_dev.hpp"
#include "mh_dev.hpp"
#include "mh_each_dev.hpp"
#include "../../include/mh.h"

namespace mhq {

using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;

constexpr int LDS_MAX = 163840;
// The LDS tables take up to 160 KiB: one workgroup per CU.  Below SPREAD lookups per CU the shared-model lookups run 256-lane
// workgroups instead, so that their lanes spread over four times as many CUs (measured on an MI355X: 3-23 % faster at 1 K-16 K
// lookups, the same above).
constexpr uint64_t SPREAD = 256;

// ------------------------------------------------------------------------------------------------ the symbol decoders
// next() decodes one symbol in the lane's context ctx and advances ctx.  P: RangeParams or LookupParams (both carry tab).
//   BOUND, PER_CU   the launch bound the kernels compile under and the workgroups a CU holds
//   POS, entry_ctx  the bit offset and the context of an index entry

// an order-0/1 index entry, and a model that is the same for every stream
struct Entry01 {
    static constexpr uint64_t POS = MH_INDEX_BIT_MASK;
    static __device__ __forceinline__ uint32_t entry_ctx(uint64_t e) { return uint32_t(e >> 56); }
    __device__ __forceinline__ void stream(const LookupParams &, uint64_t) {}
};

// the shared model: LDS tables, one context table per byte (order 0: the same table 256 times)
struct SharedTables : Entry01 {
    static constexpr int BOUND = mhb::B_THREADS, PER_CU = 1;
    static constexpr bool LDS = true;
    const uint16_t *lut;
    const uint32_t *sub_base;
    DecTables tabs;
    template <typename P> __device__ __forceinline__ void init(const P &p, unsigned char *smem) { tabs = mhb::load_tables(p.tab, smem, lut, sub_base); }
    template <typename P>
    __device__ __forceinline__ uint32_t next(const P &, const BitSrc &src, BitCursor &bc, uint32_t &ctx, uint32_t &used, bool &bad) const {
        return ctx = mhk::decode_one(lut, sub_base, tabs, src, bc, ctx, used, bad);
    }
};

// the set's model of stream i: its context -> slot row and its order, tables in L2.  (Compiled under the shared model's bound
// and launched with 256 lanes.)
struct SetTables : Entry01 {
    static constexpr int BOUND = 1024, PER_CU = 8;
    static constexpr bool LDS = false;
    const uint32_t *row;
    bool o1;
    __device__ __forceinline__ void init(const LookupParams &, unsigned char *) {}
    __device__ __forceinline__ void stream(const LookupParams &p, uint64_t i) { row = p.set.ctx_slot + i * 256u; o1 = p.set.type[i] != 0; }
    __device__ __forceinline__ uint32_t next(const LookupParams &p, const BitSrc &src, BitCursor &bc, uint32_t &ctx, uint32_t &used, bool &bad) const {
        return ctx = mhe::decode_sym(p.set, row, o1 ? ctx : 0u, src, bc, used, bad);
    }
};

// the shared order-2 model: general form, every level gathered from L2; ctx holds the last two symbols (a pair without a
// code is a null entry: bad)
struct Shared2Tables {
    static constexpr int BOUND = 256, PER_CU = 8;
    static constexpr bool LDS = false;
    static constexpr uint64_t POS = mhk::IDX2_POS;
    static __device__ __forceinline__ uint32_t entry_ctx(uint64_t e) { return uint32_t(e >> 48); }
    DecTables tabs;
    template <typename P> __device__ __forceinline__ void init(const P &p, unsigned char *) { tabs = DecTables{p.tab.sec, p.tab.tree, p.tab.P, 0u, 0u}; }
    __device__ __forceinline__ void stream(const LookupParams &, uint64_t) {}
    template <typename P>
    __device__ __forceinline__ uint32_t next(const P &p, const BitSrc &src, BitCursor &bc, uint32_t &ctx, uint32_t &used, bool &bad) const {
        const uint32_t sym = mhk::decode_one(p.tab.prim, p.tab.sec_base, tabs, src, bc, ctx, used, bad);
        ctx = ((ctx << 8) | sym) & 0xFFFFu;
        return sym;
    }
};

// the item of w: the largest j with bases[j] <= w (items without units share their successor's base)
__device__ __forceinline__ uint64_t item_of(const unsigned long long *bases, uint64_t n, uint64_t w) {
    uint64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (bases[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the dynamic LDS of a policy's kernels: the shared model's tables, which every kernel in fns must be allowed to take
template <typename Tables, typename P, size_t N>
hipError_t tables_room(const P &p, const void *const (&fns)[N], size_t &lds) {
    lds = 0;
    if (!Tables::LDS) return hipSuccess;
    for (const void *fn : fns) {
        const hipError_t attr = mhk::allow_lds(fn, LDS_MAX);
        if (attr != hipSuccess) return attr;
    }
    lds = mhb::tables_lds(p.tab);
    return lds > size_t(LDS_MAX) ? hipErrorInvalidValue : hipSuccess;
}

}  // namespace mhq
