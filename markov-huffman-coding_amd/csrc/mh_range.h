// mh_range.h — launch interface between the random-access calls of the C ABI (mh_api_range.cpp, mh_api_batch_range.cpp) and
// their kernels (mh_range.hip), for every order and model kind (include/mh.h, "RANDOM ACCESS: BYTE RANGES OF AN INDEXED
// STREAM", "RANDOM ACCESS INTO BATCHES", "RANDOM ACCESS INTO ORDER-2 STREAMS"):
//   ranges    [begin, end) of ONE indexed stream, under an order-0/1 or an order-2 model (RangeParams, launch_ranges)
//   lookups   (stream, begin, end) into a batch, under one shared order-0/1 model, one model per stream or one shared order-2
//             model (LookupParams, launch_lookups)
// The model kind is mhb::Model (mh_batch.h), as for the search and the re-coder.  Under Shared2 the parameters keep their
// fields and change their meaning:
//   - index entries are ctx16 << 48 | bit offset (mhk::IDX2_POS masks the offset);
//   - the fine index (ranges) is ctx16 << 16 | bits from the chunk's entry to the piece, 0xFFFF = does not fit;
//   - tab holds the model's order-2 tables (prim / sec / sec_base / tree of 65 536 contexts, read in the general form from
//     L2, as decode2_kernel reads them); sec_lds, direct and H are unused;
//   - prev0 (lookups) is the 16-bit start context prev0 << 8 | prev0.
// The decode tables, the batch layout and the lane helpers are the batch decoder's (mh_batch.h, mh_batch_dev.hpp), used
// read-only.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"
#include "mh_each.h"

namespace mhq {

// workspace of every call: status block (int32 status at 0) | item bases (u64, n + 1, scanned in place) | scan block sums
struct RangeLayout {
    size_t off_bases, off_sums, total;
};
inline RangeLayout range_layout(uint64_t n) {
    RangeLayout l;
    l.off_bases = 64;
    l.off_sums = l.off_bases + size_t(n + 1) * 8;
    l.total = (l.off_sums + size_t(mhb::scan_blocks(n + 1) + 1) * 8 + 255) & ~size_t(255);
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
    uint64_t n;                     // ranges
    uint8_t *out;
    const uint64_t *out_at;
    uint64_t out_cap;
    int *status;                    // n, one per range
    mhb::DecBatchParams tab;        // the model's decode tables (only its table fields are used)
};

struct LookupParams {
    const uint8_t *payload;         // packed payloads, 16-byte aligned
    const uint64_t *pay_off;        // n_streams + 1 byte offsets (only the touched streams' entries are read)
    const uint64_t *nbits;          // n_streams
    uint64_t n_streams;
    uint32_t prev0;
    const uint64_t *sym_off;        // n_streams + 1 symbol offsets (the encode's in_off); required with an index, optional without
    const uint64_t *index;          // batch chunk index (mh_batch_index_base slices), nullptr: index-free
    uint32_t chunk_shift;
    uint64_t walk_max_bits;         // index-free: lookups into longer streams are refused (MH_ERR_ARG)
    const uint64_t *lookups;        // 3 per lookup: stream, begin, end
    uint64_t n;                     // lookups
    uint8_t *out;
    const uint64_t *out_at;
    uint64_t out_cap;
    int *status;                    // n, one per lookup
    mhb::DecBatchParams tab;        // Shared, Shared2: the model's decode tables (only the table fields are used)
    mhe::SetDev set;                // Set: one model per stream
};

// model: Shared (LDS tables, units from unit_pos) or Shared2 (L2 tables, order-2 index format)
hipError_t launch_ranges(const RangeParams &p, mhb::Model model, void *d_ws, hipStream_t st);
// model: Shared (p.tab, LDS tables), Set (p.set, L2 tables) or Shared2 (p.tab, L2 tables)
hipError_t launch_lookups(const LookupParams &p, mhb::Model model, void *d_ws, hipStream_t st);

// the call-level checks every device lookup call shares (mh_api_batch_range.cpp); fills everything of p but the tables.
// MH_OK, MH_ERR_ARG or MH_ERR_CAPACITY (workspace).
int prepare_lookups(const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams, uint32_t prev0,
                    const uint64_t *d_sym_off, const uint64_t *d_index, uint32_t chunk_symbols, const uint64_t *d_lookups, size_t n_lookups,
                    uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap, int32_t *d_lookup_status, void *d_ws, size_t ws_bytes,
                    LookupParams &p);

}  // namespace mhq
