// mh_api_crc.cpp — the digest calls of the C ABI (include/mh.h, "DIGESTS OF BATCHES"): the device calls under one shared
// model of order 0/1 or 2 or under a model set, the digest of uncompressed batches (kernels: mh_crc.hip), the host-buffer
// forms and the host-side combine.
#include "mh_api_reader.hpp"
#include "mh_crc.h"

using namespace mhapi;

namespace {

constexpr mhc::CrcTables kTables = mhc::make_tables();

// the batch part of the parameters behind the shared checks (mh_api_reader.hpp), and the digests' own outputs
int prepare(const CodedBatch &a, uint32_t ctx0, uint32_t *d_crc, uint64_t *d_len, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
            mhc::CrcParams &p) {
    if (!d_crc && a.n) return MH_ERR_ARG;
    const mhc::CrcLayout L = mhc::crc_layout(a.n);
    const int rc = dev_batch_params(a, SymOff::UnderIndex, ctx0, d_ws, ws_bytes, L.total, L.off_status, d_stream_status, p.b);
    if (rc != MH_OK) return rc;
    p.crc = d_crc;
    p.len = reinterpret_cast<unsigned long long *>(d_len);
    return MH_OK;
}

// mh_dev_crc_batch and mh_dev_crc_batch_o2 behind their order checks: one shared model, its tables as the model's batch
// decoder takes them
int crc_shared(const mh_model *m, mhc::Model model, const CodedBatch &a, uint32_t *d_crc, uint64_t *d_len, int32_t *d_stream_status, void *d_ws,
               size_t ws_bytes, void *stream) {
    mhc::CrcParams p{};
    const int rc = prepare(a, ctx_of_prev0(m, a.prev0), d_crc, d_len, d_stream_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    fill_dec_tables(m, p.b);
    HIP_TRY(mhc::launch_crc(p, model, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

// The host form of either order: an index-free batch with a stream over the walk cap is indexed first and digested as an
// indexed batch; a stream the indexing fails has no symbols, so crc 0 and len 0.  Then the batch is uploaded, the device call
// of the model's order runs once and the results come back.
int crc_host(const mh_model *m, CodedBatch a, uint32_t *crc, uint64_t *len, int32_t *stream_status) {
    if (!crc && a.n) return MH_ERR_ARG;
    int rc = host_batch_args(a, a.index != nullptr);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    std::vector<uint64_t> own_so, own_idx;
    std::vector<int32_t> idx_st;
    if (over_walk_cap(a)) {
        own_so.assign(a.n + 1, 0);
        if ((rc = index_first(m, a, false, own_so.data(), own_idx, idx_st)) != MH_OK) return rc;
    }
    const hipStream_t st = nullptr;
    const size_t n = a.n, wsb = mh_dev_crc_batch_workspace(n, a.sym_total, a.index ? a.chunk_symbols : 0);
    DevBatch db;
    DevBuf d_crc, d_len, d_st, d_ws;
    HIP_TRY(d_crc.alloc(n * 4));
    HIP_TRY(d_len.alloc(n * 8));
    HIP_TRY(d_st.alloc(n * 4));
    HIP_TRY(d_ws.alloc(wsb));
    if ((rc = db.upload(a, st)) != MH_OK) return rc;
    rc = crc_shared(m, order2(m) ? mhc::Model::Shared2 : mhc::Model::Shared, db.d, d_crc.as<uint32_t>(), d_len.as<uint64_t>(), d_st.as<int32_t>(),
                    d_ws.p, wsb, st);
    if (rc != MH_OK) return rc;
    const int dev_rc = mh_dev_status(d_ws.p, st);
    std::vector<int32_t> sst(n);
    if (n) {
        HIP_TRY(hipMemcpy(sst.data(), d_st.p, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(crc, d_crc.p, n * 4, hipMemcpyDeviceToHost));
        if (len) HIP_TRY(hipMemcpy(len, d_len.p, n * 8, hipMemcpyDeviceToHost));
    }
    const int first = first_failure(sst, idx_st, dev_rc);
    if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
    return first;
}

}  // namespace

extern "C" {

size_t mh_dev_crc_batch_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    (void)sym_total; (void)chunk_symbols;                          // nothing is kept per chunk
    return mhc::crc_layout(n_streams).total;
}

int mh_dev_crc_batch(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                     uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                     uint32_t chunk_symbols, uint32_t *d_crc, uint64_t *d_len, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order01(m)) return MH_ERR_ARG;
    return crc_shared(m, mhc::Model::Shared, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                      d_crc, d_len, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_crc_batch_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                        uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                        uint32_t chunk_symbols, uint32_t *d_crc, uint64_t *d_len, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
                        void *stream) {
    if (!order2(m)) return MH_ERR_ARG;
    return crc_shared(m, mhc::Model::Shared2, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                      d_crc, d_len, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_crc_each(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                    uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                    uint32_t chunk_symbols, uint32_t *d_crc, uint64_t *d_len, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!s || n_streams != s->d.n) return MH_ERR_ARG;
    mhc::CrcParams p{};
    const int rc = prepare({d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols}, prev0, d_crc,
                           d_len, d_stream_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    p.set = s->d;
    HIP_TRY(mhc::launch_crc(p, mhc::Model::Set, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int mh_crc_batch(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, uint8_t prev0,
                 const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint32_t *crc, uint64_t *len, int32_t *stream_status) {
    if (!order01(m)) return MH_ERR_ARG;
    return crc_host(m, {payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols}, crc, len, stream_status);
}

int mh_crc_batch_o2(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, uint8_t prev0,
                    const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint32_t *crc, uint64_t *len, int32_t *stream_status) {
    if (!order2(m)) return MH_ERR_ARG;
    return crc_host(m, {payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols}, crc, len, stream_status);
}

size_t mh_dev_crc_raw_batch_workspace(size_t n_streams, size_t total) {
    (void)n_streams; (void)total;                                  // the status block and the tables
    return mhc::crc_layout(0).total;
}

int mh_dev_crc_raw_batch(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint32_t *d_crc, void *d_ws,
                         size_t ws_bytes, void *stream) {
    if ((!d_data && total) || !d_in_off || (!d_crc && n_streams) || !d_ws || !aligned16(d_ws)) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_crc_raw_batch_workspace(n_streams, total)) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    HIP_TRY(mhc::launch_crc_raw(d_data, d_in_off, n_streams, total, d_crc, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

uint32_t mh_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return mhc::gf_mul(crc_a, mhc::pow8_of(kTables.pow8, len_b)) ^ crc_b;
}

}  // extern "C"
