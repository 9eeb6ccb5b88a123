// mh_batch_range.h — launch interface between the batch-range calls of the C ABI (mh_api_batch_range.cpp) and their kernels
// (mh_batch_range.hip): lookups (stream, begin, end) into a batch of order-0/1 streams, under one shared model or one model
// per stream (include/mh.h, "RANDOM ACCESS INTO BATCHES").  The batch layout is mh_batch.h's; the workspace is
// mh_range.h's (status block, item bases, scan block sums), sized by the number of lookups.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"
#include "mh_each.h"
#include "mh_range.h"

namespace mhq {

struct BatchRangeParams {
    const uint8_t *payload;         // packed payloads, 16-byte aligned
    const uint64_t *pay_off;        // n + 1 byte offsets (only the touched streams' entries are read)
    const uint64_t *nbits;          // n
    uint64_t n;
    uint32_t prev0;
    const uint64_t *sym_off;        // n + 1 symbol offsets (the encode's in_off); required with an index, optional without
    const uint64_t *index;          // batch chunk index (mh_batch_index_base slices), nullptr: index-free
    uint32_t chunk_shift;
    uint64_t walk_max_bits;         // index-free: lookups into longer streams are refused (MH_ERR_ARG)
    const uint64_t *lookups;        // 3 per lookup: stream, begin, end
    uint64_t m;
    uint8_t *out;
    const uint64_t *out_at;
    uint64_t out_cap;
    int *lookup_status;
    mhb::DecBatchParams tab;        // shared model: its decode tables (only the table fields are used)
    mhe::SetDev set;                // model set: one model per stream
};

// shared: the model in p.tab (LDS tables); otherwise the set in p.set (L2 tables)
hipError_t launch_batch_ranges(const BatchRangeParams &p, bool shared, void *d_ws, hipStream_t st);

// the call-level checks every device lookup call shares (mh_api_batch_range.cpp); fills everything of p but the tables.
// MH_OK, MH_ERR_ARG or MH_ERR_CAPACITY (workspace).
int prepare_lookups(const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams, uint8_t prev0,
                    const uint64_t *d_sym_off, const uint64_t *d_index, uint32_t chunk_symbols, const uint64_t *d_lookups, size_t n_lookups,
                    uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap, int32_t *d_lookup_status, void *d_ws, size_t ws_bytes,
                    BatchRangeParams &p);

}  // namespace mhq
