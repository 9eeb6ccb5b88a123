// mh_each_dev.hpp — device code shared by the kernels that decode under a model set (include/mh.h, "BATCHES OF STREAMS, ONE
// MODEL EACH"): the batch kernel families through mhb::Dec<Model::Set> (mh_symdec_dev.hpp) and the lookups into batches
// (mh_range.hip).  The tables stay in global memory (L2): a set's slots are far too many for LDS.  Unnamed namespace: each
// kernel file gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_decode_dev.hpp"
#include "mh_dev.hpp"
#include "mh_each.h"

namespace mhe {
namespace {

using mhk::BitCursor;
using mhk::BitSrc;

// one symbol of stream i after prev: the 8-bit first level, then the walk tree for longer codes (<= 64 bits)
__device__ __forceinline__ uint32_t decode_sym(const SetDev &s, const uint32_t *row, uint32_t ctx, const BitSrc &src, BitCursor &bc,
                                               uint32_t &used, bool &bad) {
    const uint32_t slot = row[ctx];
    if (slot == NO_SLOT) { bad = true; return 0; }            // a context the model has no code for
    bc.refill(src);
    const uint32_t e = s.prim[size_t(slot) * 256u + uint32_t(bc.window() >> 56)];
    if (e & mh::DEC16_LEAF) {
        const uint32_t len = (e >> 8) & 31u;
        bad |= (len == 0);
        bc.drop(len); used += len;
        return e & 255u;
    }
    bc.drop(8);
    const uint32_t *tr = s.tree + size_t(slot) * 256u;
    uint32_t node = e & 255u, nb = 8;
    for (int guard = 0; guard < 56; ++guard) {
        bc.refill(src);
        const uint32_t bit = uint32_t(bc.window() >> 63);
        bc.drop(1); ++nb;
        const uint32_t pair = tr[node];
        const uint32_t c = bit ? (pair >> 16) : (pair & 0xFFFFu);
        if (c & mh::TREE_LEAF) { used += nb; return c & 255u; }
        node = c & 255u;
    }
    bad = true;
    used += nb;
    return 0;
}

}  // namespace
}  // namespace mhe
