// mh_api_batch_o2.cpp — the order-2 batch calls of the C ABI (include/mh.h, "BATCHES OF ORDER-2 STREAMS"): many small
// streams under one shared order-2 model in a few launches (kernels: mh_batch_o2.hip), and their host-buffer forms (the
// bodies of mh_encode_batch / mh_decode_batch over the order-2 device calls).  mh_dev_decode_batch_o2 is the second entry of
// mh_dev_decode_batch's body (mh_api_batch.cpp).  Extension, parity unpinned.
#include "mh_api_internal.hpp"
#include "mh_batch_o2.h"

using namespace mhapi;

extern "C" {

size_t mh_dev_histogram_o2_batch_workspace(size_t total) {
    const size_t h = mh_dev_histogram_o2_workspace(total);
    return h > 256 ? h : 256;
}

int mh_dev_histogram_o2_batch(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint8_t prev0,
                              uint64_t *d_counts, void *d_ws, size_t ws_bytes, void *stream) {
    if ((!d_data && total) || !d_in_off || !d_counts || !d_ws || !aligned16(d_data)) return MH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_ws) & 255u) return MH_ERR_ARG;
    if (ws_bytes < 256) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const uint16_t ctx0 = uint16_t(uint32_t(prev0) << 8 | prev0);
    // clears the status word, then checks that the 1 << 24 counts add up to total (the fix-up below moves, never adds)
    const int rc = mh_dev_histogram_o2_ws(d_data, total, ctx0, d_counts, d_ws, ws_bytes, stream);
    if (rc != MH_OK) return rc;
    HIP_TRY(mhb::launch_hist2_fixup(d_data, d_in_off, n_streams, total, prev0, reinterpret_cast<unsigned long long *>(d_counts),
                                    static_cast<int *>(d_ws), static_cast<hipStream_t>(stream)));
    return MH_OK;
}

size_t mh_dev_encode_batch_o2_workspace(size_t n_streams, size_t total) { return mhb::enc_layout(n_streams, total).total; }

int mh_dev_encode_batch_o2(const mh_model *m, const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint8_t prev0,
                           uint8_t *d_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_nbits, uint64_t *d_index, uint32_t chunk_symbols,
                           void *d_ws, size_t ws_bytes, void *stream) {
    if (!order2(m) || (!d_data && total) || !d_in_off || !d_out_off || (!d_nbits && n_streams) || (!d_payload && cap) || !d_ws) return MH_ERR_ARG;
    if (!aligned16(d_payload) || !aligned16(d_ws)) return MH_ERR_ARG;
    const int shift = d_index ? chunk_shift_of(chunk_symbols) : 0;
    if (shift < 0) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_encode_batch_o2_workspace(n_streams, total)) return MH_ERR_CAPACITY;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_len8 || !have_device()) return MH_ERR_NO_DEVICE;
    mhb::EncBatchO2Params p{};
    p.data = d_data; p.in_off = d_in_off; p.n = n_streams; p.total = total; p.prev0 = ctx_of_prev0(m, prev0);
    p.chunk_shift = uint32_t(shift);
    p.index = reinterpret_cast<unsigned long long *>(d_index);
    p.out = d_payload; p.cap = cap;
    p.out_off = reinterpret_cast<unsigned long long *>(d_out_off);
    p.nbits = reinterpret_cast<unsigned long long *>(d_nbits);
    p.len8 = m->d_len8; p.code64 = m->d_code64; p.enc64 = m->d_enc64; p.max_len = m->max_len;
    if (m->o2_enc_ok) { p.o2img = m->d_o2img; p.o2img_bytes = m->o2img_bytes; }    // (the single-stream encoder's rule: mh_api.cpp)
    HIP_TRY(mhb::launch_encode_batch_o2(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

/* ------------------------------------------------------- host-buffer calls */

int mh_encode_batch_o2(const mh_model *m, const uint8_t *data, const uint64_t *in_off, size_t n_streams, uint8_t prev0,
                       uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *nbits, uint64_t *index, uint32_t chunk_symbols) {
    if (!order2(m)) return MH_ERR_ARG;
    return encode_batch_host(m, data, in_off, n_streams, prev0, out_payload, cap, out_off, nbits, index, chunk_symbols, mh_dev_encode_batch_o2);
}

int mh_decode_batch_o2(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams,
                       uint8_t prev0, uint8_t *out, size_t out_cap, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                       int32_t *stream_status) {
    if (!order2(m)) return MH_ERR_ARG;
    return decode_batch_host(m, payload, pay_off, nbits, n_streams, prev0, out, out_cap, sym_off, index, chunk_symbols, stream_status,
                             mh_dev_decode_batch_o2);
}

}  // extern "C"
