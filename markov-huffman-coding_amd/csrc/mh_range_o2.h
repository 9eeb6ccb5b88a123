// mh_range_o2.h — launch interface between the order-2 random-access calls of the C ABI (mh_api_range_o2.cpp) and their
// kernels (mh_range_o2.hip): ranges [begin, end) of ONE indexed order-2 stream, and lookups (stream, begin, end) into a batch
// of order-2 streams (include/mh.h, "RANDOM ACCESS INTO ORDER-2 STREAMS").  Parameters and workspace are those of the
// order-0/1 range calls (mh_range.h, mh_batch_range.h); only their meaning differs:
//   - index entries are ctx16 << 48 | bit offset (mhk::IDX2_POS masks the offset);
//   - the fine index (single stream) is ctx16 << 16 | bits from the chunk's entry to the piece, 0xFFFF = does not fit;
//   - tab holds the model's order-2 tables (prim / sec / sec_base / tree of 65 536 contexts, read in the general form from
//     L2, as decode2_kernel reads them); sec_lds, direct and H are unused;
//   - prev0 (batch) is the 16-bit start context prev0 << 8 | prev0.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch_range.h"
#include "mh_range.h"

namespace mhr {

hipError_t launch_decode_ranges_o2(const RangeParams &p, void *d_ws, hipStream_t st);
hipError_t launch_batch_ranges_o2(const mhq::BatchRangeParams &p, void *d_ws, hipStream_t st);

}  // namespace mhr
