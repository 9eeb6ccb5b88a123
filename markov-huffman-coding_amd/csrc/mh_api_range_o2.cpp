// mh_api_range_o2.cpp — random access into order-2 streams (include/mh.h, "RANDOM ACCESS INTO ORDER-2 STREAMS"; extension,
// parity unpinned): byte ranges of one indexed stream and lookups into a batch under one shared order-2 model, decoded on the
// device (kernels: mh_range_o2.hip).  The host forms are the order-0/1 ones (mh_api_range.cpp, mh_api_batch_range.cpp) over
// these device calls.
#include "mh_api_internal.hpp"
#include "mh_batch_range.h"
#include "mh_range.h"
#include "mh_range_o2.h"

using namespace mhapi;

extern "C" {

size_t mh_dev_decode_ranges_o2_workspace(size_t n_ranges) { return mhr::range_layout(n_ranges).total; }

int mh_dev_decode_ranges_o2(const mh_model *m, const uint8_t *d_payload, uint64_t payload_byte_base, uint64_t payload_bytes, uint64_t nbits,
                            const uint64_t *d_index, uint32_t chunk_symbols, uint64_t n_symbols, const uint32_t *d_fine,
                            const uint64_t *d_ranges, size_t n_ranges, uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                            int32_t *d_range_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order2(m) || (!d_payload && payload_bytes) || (!d_index && n_symbols) || !d_ws) return MH_ERR_ARG;
    if (n_ranges && (!d_ranges || !d_out_at || !d_range_status)) return MH_ERR_ARG;
    if ((!d_out && out_cap) || !aligned16(d_out) || !aligned16(d_ws)) return MH_ERR_ARG;
    const int shift = chunk_shift_of(chunk_symbols);
    if (shift < 0 || n_symbols > nbits) return MH_ERR_ARG;
    // the order-2 fine index exists for chunks of up to 1024 symbols (its entries are 16-bit distances from the chunk's entry)
    if (d_fine && (shift > 10 || (reinterpret_cast<uintptr_t>(d_fine) & 3u))) return MH_ERR_ARG;
    if (payload_byte_base > (nbits + 7) / 8 || payload_bytes > (nbits + 7) / 8 - payload_byte_base) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_decode_ranges_o2_workspace(n_ranges)) return MH_ERR_CAPACITY;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    mhr::RangeParams p{};
    p.payload = d_payload; p.win_base = payload_byte_base; p.win_bytes = payload_bytes;
    p.nbits = nbits; p.n_symbols = n_symbols;
    p.index = d_index; p.chunk_shift = uint32_t(shift);
    p.fine = d_fine;
    p.unit_shift = d_fine ? uint32_t(MH_T_SUB_SHIFT) : uint32_t(shift);
    p.n_units = (n_symbols + (uint64_t(1) << p.unit_shift) - 1) >> p.unit_shift;
    p.ranges = d_ranges; p.n = n_ranges;
    p.out = d_out; p.out_at = d_out_at; p.out_cap = out_cap;
    p.range_status = d_range_status;
    fill_dec_tables(m, p.tab);
    HIP_TRY(mhr::launch_decode_ranges_o2(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int mh_decode_ranges_o2(const mh_model *m, const uint8_t *payload, uint64_t nbits, const uint64_t *index, uint32_t chunk_symbols,
                        uint64_t n_symbols, const uint64_t *ranges, size_t n_ranges, uint8_t *out, size_t out_cap, uint64_t *out_off,
                        int32_t *range_status) {
    return decode_ranges_host(m, true, payload, nbits, index, chunk_symbols, n_symbols, ranges, n_ranges, out, out_cap, out_off,
                              range_status);
}

size_t mh_dev_decode_batch_o2_ranges_workspace(size_t n_lookups) { return mhr::range_layout(n_lookups).total; }

int mh_dev_decode_batch_o2_ranges(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                                  size_t n_streams, uint8_t prev0, const uint64_t *d_sym_off, const uint64_t *d_index, uint32_t chunk_symbols,
                                  const uint64_t *d_lookups, size_t n_lookups, uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                                  int32_t *d_lookup_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order2(m)) return MH_ERR_ARG;
    mhq::BatchRangeParams p{};
    const int rc = mhq::prepare_lookups(d_payload, d_pay_off, d_nbits, n_streams, prev0, d_sym_off, d_index, chunk_symbols, d_lookups,
                                        n_lookups, d_out, d_out_at, out_cap, d_lookup_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    p.prev0 = ctx_of_prev0(m, prev0);
    fill_dec_tables(m, p.tab);
    HIP_TRY(mhr::launch_batch_ranges_o2(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int mh_decode_batch_o2_ranges(const mh_model *m, const uint8_t *payload, uint64_t payload_bytes, const uint64_t *pay_off, const uint64_t *nbits,
                              size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                              const uint64_t *lookups, size_t n_lookups, uint8_t *out, size_t out_cap, uint64_t *out_off, int32_t *lookup_status) {
    return decode_batch_ranges_host(m, true, payload, payload_bytes, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols,
                                    lookups, n_lookups, out, out_cap, out_off, lookup_status);
}

}  // extern "C"
