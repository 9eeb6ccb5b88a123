// mh_symdec_dev.hpp — the symbol decoder of a lane, one policy per model kind, for the kernel families over compressed
// batches: the decoders (mh_batch.hip), which store the symbol, and those that take it from a register instead: the search
// (mh_find.hip) and the digests (mh_crc.hip).  next() decodes one symbol in the lane's context ctx and rolls ctx on: the
// kernels feed the symbol to their consumer and never touch the context.  A stream starts in b.prev0 (order 2: both bytes).
//   NT, PER_CU   the workgroup shape of every family under this model kind
//   O2           the format of the batch's index entries (mhb::chunk_of)
// P is the family's parameter struct: p.b (mhb::DecBatchParams: the batch and, under a shared model, its decode tables) and
// p.set (mhe::SetDev: the models under a set).  Like mh_batch_dev.hpp, everything is in an unnamed namespace.
#pragma once

#include "mh_batch_dev.hpp"
#include "mh_each_dev.hpp"

namespace mhb {
namespace {

using mhk::BitCursor;

template <Model K> struct Dec;
// the shared model's two-level tables in LDS; one workgroup of 16 waves per CU beside them
template <> struct Dec<Model::Shared> {
    static constexpr int NT = B_THREADS, PER_CU = 1;
    static constexpr bool O2 = false;
    const uint16_t *lut;
    const uint32_t *sub_base;
    DecTables tabs;
    template <typename P>
    __device__ __forceinline__ Dec(const P &p, unsigned char *smem) : tabs(load_tables(p.b, smem, lut, sub_base)) {}
    template <typename P> __device__ __forceinline__ void stream(const P &, uint64_t) {}
    template <typename P>
    __device__ __forceinline__ uint32_t next(const P &, const BitSrc &src, BitCursor &bc, uint32_t &ctx, uint32_t &used, bool &bad) const {
        return ctx = mhk::decode_one(lut, sub_base, tabs, src, bc, ctx, used, bad);
    }
};
// stream i's slots in L2: no tables in LDS, so small workgroups and many waves per CU for the gathers
template <> struct Dec<Model::Set> {
    static constexpr int NT = 256, PER_CU = 8;
    static constexpr bool O2 = false;
    const uint32_t *row;
    bool o1;
    template <typename P> __device__ __forceinline__ Dec(const P &, unsigned char *) : row(nullptr), o1(false) {}
    template <typename P> __device__ __forceinline__ void stream(const P &p, uint64_t i) { row = p.set.ctx_slot + i * 256u; o1 = p.set.type[i] != 0; }
    template <typename P>
    __device__ __forceinline__ uint32_t next(const P &p, const BitSrc &src, BitCursor &bc, uint32_t &ctx, uint32_t &used, bool &bad) const {
        return ctx = mhe::decode_sym(p.set, row, o1 ? ctx : 0u, src, bc, used, bad);
    }
};
// the shared model's order-2 tables as decode2_kernel reads them: general form, every level gathered from L2
// (the same shape as under a set); ctx holds the last two symbols
template <> struct Dec<Model::Shared2> {
    static constexpr int NT = 256, PER_CU = 8;
    static constexpr bool O2 = true;
    const uint16_t *prim;
    const uint32_t *sec_base;
    DecTables tabs;
    template <typename P>
    __device__ __forceinline__ Dec(const P &p, unsigned char *) : prim(p.b.prim), sec_base(p.b.sec_base), tabs{p.b.sec, p.b.tree, p.b.P, 0u, 0u} {}
    template <typename P> __device__ __forceinline__ void stream(const P &, uint64_t) {}
    template <typename P>
    __device__ __forceinline__ uint32_t next(const P &, const BitSrc &src, BitCursor &bc, uint32_t &ctx, uint32_t &used, bool &bad) const {
        const uint32_t sym = mhk::decode_one(prim, sec_base, tabs, src, bc, ctx, used, bad);
        ctx = ((ctx << 8) | sym) & 0xFFFFu;
        return sym;
    }
};

}  // namespace
}  // namespace mhb
