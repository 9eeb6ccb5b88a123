// mh_batch_o2.h — launch interface between the order-2 batch calls of the C ABI (mh_api_batch_o2.cpp) and their kernels
// (mh_batch_o2.hip): many independent streams under one shared order-2 model, each starting in context (prev0, prev0)
// (include/mh.h, "BATCHES OF ORDER-2 STREAMS").  Layouts, work units and workspaces are those of the order-0/1 batch
// (mh_batch.h); only the encoder's tables differ.  The decoder is mhb::launch_decode under Model::Shared2.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"

namespace mhb {

// EncBatchParams with prev0 = the 16-bit start context prev0 << 8 | prev0, len8 / code64 indexed ctx << 8 | sym (1 << 24
// entries); enc16 and len_slot are unused
struct EncBatchO2Params : EncBatchParams {
    const uint64_t *enc64;          // len << 56 | code per (ctx, sym), len 255: longer than 56 bits (nullptr: len8 / code64 only)
    const uint8_t *o2img;           // the live contexts' LDS image (mh_encode.hip, o2hot_lookup16), or nullptr when the model has none
    uint32_t o2img_bytes;
};

// The order-2 histogram of the concatenation counted the first two symbols of each stream in contexts that reach into the
// streams in front of it: one thread per stream moves them to the stream's own contexts (prev0 << 8 | prev0, then
// prev0 << 8 | first byte).  Offsets are checked as in launch_hist_fixup (MH_ERR_ARG through d_status).
hipError_t launch_hist2_fixup(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total, uint32_t prev0,
                              unsigned long long *d_counts, int *d_status, hipStream_t st);
// workspace: enc_layout of mh_batch.h; index entries carry the context in bits 48..63
hipError_t launch_encode_batch_o2(const EncBatchO2Params &p, void *d_ws, hipStream_t st);

}  // namespace mhb
