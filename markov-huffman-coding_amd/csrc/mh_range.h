// mh_range.h — launch interface between the byte-range calls of the C ABI (mh_api_range.cpp) and their kernels
// (mh_range.hip): ranges [begin, end) of ONE indexed order-0/1 stream (include/mh.h, "RANDOM ACCESS: BYTE RANGES OF AN
// INDEXED STREAM").  The decode tables and the lane helpers are the batch decoder's (mh_batch.h, mh_batch_dev.hpp), used
// read-only.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"

namespace mhr {

// workspace: status block (int32 status at 0) | item bases (u64, n_ranges + 1, scanned in place) | scan block sums
struct RangeLayout {
    size_t off_bases, off_sums, total;
};
inline RangeLayout range_layout(uint64_t n_ranges) {
    RangeLayout l;
    l.off_bases = 64;
    l.off_sums = l.off_bases + size_t(n_ranges + 1) * 8;
    l.total = (l.off_sums + size_t(mhb::scan_blocks(n_ranges + 1) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

struct RangeParams {
    const uint8_t *payload;         // stream byte win_base sits here (any alignment)
    uint64_t win_base, win_bytes;   // the window: stream bytes [win_base, win_base + win_bytes)
    uint64_t nbits, n_symbols;
    const uint64_t *index;          // chunk index of the whole stream (bit offsets from the stream start)
    uint32_t chunk_shift;
    const uint32_t *fine;           // fine index or nullptr
    uint32_t unit_shift;            // chunk_shift, or MH_T_SUB_SHIFT with a fine index
    uint64_t n_units;               // ceil(n_symbols / unit)
    const uint64_t *ranges;         // 2 per range: begin, end
    uint64_t n;
    uint8_t *out;
    const uint64_t *out_at;
    uint64_t out_cap;
    int *range_status;
    mhb::DecBatchParams tab;        // the model's decode tables (only its table fields are used)
};

hipError_t launch_decode_ranges(const RangeParams &p, void *d_ws, hipStream_t st);

}  // namespace mhr
