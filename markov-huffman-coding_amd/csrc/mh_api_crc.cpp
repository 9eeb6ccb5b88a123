// mh_api_crc.cpp — the digest calls of the C ABI (include/mh.h, "DIGESTS OF BATCHES"): the device calls under one shared
// model of order 0/1 or 2 or under a model set, the digest of uncompressed batches (kernels: mh_crc.hip), the host-buffer
// forms and the host-side combine.
#include "mh_api_internal.hpp"
#include "mh_batch.h"
#include "mh_crc.h"

using namespace mhapi;

namespace {

constexpr mhc::CrcTables kTables = mhc::make_tables();

// the checks all device calls share, in the order of mh_dev_find_batch, and the batch part of the parameters
int prepare(const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint32_t ctx0,
            const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, uint32_t *d_crc, uint64_t *d_len,
            int32_t *d_stream_status, void *d_ws, size_t ws_bytes, mhc::CrcParams &p) {
    if ((!d_payload && pay_total) || !d_pay_off || (!d_nbits && n_streams) || (!d_crc && n_streams) || !d_ws) return MH_ERR_ARG;
    if (!aligned16(d_payload) || !aligned16(d_ws)) return MH_ERR_ARG;
    int shift = 0;
    if (d_index && ((shift = chunk_shift_of(chunk_symbols)) < 0 || !d_sym_off)) return MH_ERR_ARG;
    const mhc::CrcLayout L = mhc::crc_layout(n_streams);
    if (ws_bytes < L.total) return MH_ERR_CAPACITY;
    p.b.payload = d_payload; p.b.pay_off = d_pay_off; p.b.nbits = d_nbits; p.b.n = n_streams; p.b.pay_total = pay_total; p.b.prev0 = ctx0;
    p.b.sym_off = d_index ? reinterpret_cast<unsigned long long *>(const_cast<uint64_t *>(d_sym_off)) : nullptr;   // (read only)
    p.b.sym_total = d_index ? sym_total : 0;
    p.b.index = d_index; p.b.chunk_shift = uint32_t(shift);
    p.b.walk_max_bits = MH_BATCH_WALK_MAX_BITS;
    p.b.stream_status = d_stream_status ? d_stream_status : reinterpret_cast<int *>(static_cast<unsigned char *>(d_ws) + L.off_status);
    p.crc = d_crc;
    p.len = reinterpret_cast<unsigned long long *>(d_len);
    return MH_OK;
}

// mh_dev_crc_batch and mh_dev_crc_batch_o2 behind their order checks: one shared model, its tables as the model's batch
// decoder takes them
int crc_shared(const mh_model *m, mhc::Model model, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
               uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
               uint32_t *d_crc, uint64_t *d_len, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    mhc::CrcParams p{};
    const int rc = prepare(d_payload, d_pay_off, d_nbits, n_streams, pay_total, ctx_of_prev0(m, prev0), d_sym_off, sym_total, d_index, chunk_symbols,
                           d_crc, d_len, d_stream_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    fill_dec_tables(m, p.b);
    HIP_TRY(mhc::launch_crc(p, model, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

// the argument checks of the two host forms, in the order of mh_find_batch
int host_args(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, const uint64_t *sym_off,
              const uint64_t *index, uint32_t chunk_symbols, const uint32_t *crc) {
    if (!pay_off || (!nbits && n_streams) || (!crc && n_streams)) return MH_ERR_ARG;
    if (index && (chunk_shift_of(chunk_symbols) < 0 || !sym_off)) return MH_ERR_ARG;
    if (!offsets_ok(pay_off, n_streams)) return MH_ERR_ARG;
    if (!payload && pay_off[n_streams]) return MH_ERR_ARG;
    for (size_t i = 0; i < n_streams; ++i)
        if (nbits[i] > (pay_off[i + 1] - pay_off[i]) * 8) return MH_ERR_ARG;
    if (index && !offsets_ok(sym_off, n_streams)) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    return MH_OK;
}

// The host form of either order: an index-free batch with a stream over the walk cap is indexed first (mh_index_batch /
// mh_index_batch_o2 never refuse a valid stream) and digested as an indexed batch; a stream the indexing fails keeps that
// error and has no symbols, so crc 0 and len 0.  Then the batch is uploaded, the device call of the model's order runs once
// and the results come back.
int crc_host(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, uint8_t prev0,
             const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint32_t *crc, uint64_t *len, int32_t *stream_status) {
    int rc = host_args(m, payload, pay_off, nbits, n_streams, sym_off, index, chunk_symbols, crc);
    if (rc != MH_OK) return rc;
    const bool o2 = order2(m);
    std::vector<uint64_t> own_so, own_idx;
    std::vector<int32_t> idx_st;
    bool over = false;
    if (!index)
        for (size_t i = 0; i < n_streams && !over; ++i) over = nbits[i] > MH_BATCH_WALK_MAX_BITS;
    if (over) {
        const uint64_t minl = uint64_t(m->min_len > 0 ? m->min_len : 1);
        uint64_t bound = 0;
        for (size_t i = 0; i < n_streams; ++i) bound += nbits[i] / minl;
        chunk_symbols = MH_CHUNK_DEFAULT;
        own_so.assign(n_streams + 1, 0);
        own_idx.assign(size_t(mh_batch_index_capacity(bound, n_streams, chunk_symbols)), 0);
        idx_st.assign(n_streams, MH_OK);
        rc = (o2 ? mh_index_batch_o2 : mh_index_batch)(m, payload, pay_off, nbits, n_streams, prev0, chunk_symbols, own_so.data(), own_idx.data(),
                                                       own_idx.size(), idx_st.data());
        if (rc == MH_ERR_HIP || rc == MH_ERR_NO_DEVICE || rc == MH_ERR_NOMEM || rc == MH_ERR_CAPACITY) return rc;
        sym_off = own_so.data();
        index = own_idx.data();
    }
    const hipStream_t st = nullptr;
    const uint64_t pay_total = pay_off[n_streams];
    const uint64_t sym_total = index ? sym_off[n_streams] : 0;
    const size_t nidx = index ? size_t(mh_batch_index_capacity(sym_total, n_streams, chunk_symbols)) : 0;
    const size_t wsb = mh_dev_crc_batch_workspace(n_streams, sym_total, index ? chunk_symbols : 0);
    DevBuf d_pl, d_po, d_nb, d_so, d_idx, d_crc, d_len, d_st, d_ws;
    HIP_TRY(d_pl.alloc(size_t(pay_total) + 64));
    HIP_TRY(d_po.alloc((n_streams + 1) * 8));
    HIP_TRY(d_nb.alloc(n_streams * 8));
    HIP_TRY(d_so.alloc((n_streams + 1) * 8));
    HIP_TRY(d_idx.alloc(nidx * 8));
    HIP_TRY(d_crc.alloc(n_streams * 4));
    HIP_TRY(d_len.alloc(n_streams * 8));
    HIP_TRY(d_st.alloc(n_streams * 4));
    HIP_TRY(d_ws.alloc(wsb));
    if (pay_total) HIP_TRY(stage_h2d(d_pl.p, payload, size_t(pay_total), st));
    HIP_TRY(hipMemcpy(d_po.p, pay_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
    if (n_streams) HIP_TRY(hipMemcpy(d_nb.p, nbits, n_streams * 8, hipMemcpyHostToDevice));
    if (index) {
        HIP_TRY(hipMemcpy(d_so.p, sym_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
        if (nidx) HIP_TRY(hipMemcpy(d_idx.p, index, nidx * 8, hipMemcpyHostToDevice));
    }
    rc = (o2 ? mh_dev_crc_batch_o2 : mh_dev_crc_batch)(m, d_pl.as<uint8_t>(), d_po.as<uint64_t>(), d_nb.as<uint64_t>(), n_streams, pay_total, prev0,
                                                       index ? d_so.as<uint64_t>() : nullptr, sym_total, index ? d_idx.as<uint64_t>() : nullptr,
                                                       chunk_symbols, d_crc.as<uint32_t>(), d_len.as<uint64_t>(), d_st.as<int32_t>(), d_ws.p, wsb, st);
    if (rc != MH_OK) return rc;
    const int dev_rc = mh_dev_status(d_ws.p, st);
    std::vector<int32_t> sst(n_streams);
    if (n_streams) {
        HIP_TRY(hipMemcpy(sst.data(), d_st.p, n_streams * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(crc, d_crc.p, n_streams * 4, hipMemcpyDeviceToHost));
        if (len) HIP_TRY(hipMemcpy(len, d_len.p, n_streams * 8, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < idx_st.size(); ++i)
        if (idx_st[i] != MH_OK) sst[i] = idx_st[i];
    // the call's result: the first failed stream's error, else the device's
    int first = MH_OK;
    for (size_t i = 0; i < n_streams && first == MH_OK; ++i) first = sst[i];
    if (first == MH_OK && dev_rc != MH_OK && dev_rc != MH_ERR_ARG) first = dev_rc;
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
    return crc_shared(m, mhc::Model::Shared, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols,
                      d_crc, d_len, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_crc_batch_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                        uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                        uint32_t chunk_symbols, uint32_t *d_crc, uint64_t *d_len, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
                        void *stream) {
    if (!order2(m)) return MH_ERR_ARG;
    return crc_shared(m, mhc::Model::Shared2, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index,
                      chunk_symbols, d_crc, d_len, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_crc_each(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                    uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                    uint32_t chunk_symbols, uint32_t *d_crc, uint64_t *d_len, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!s || n_streams != s->d.n) return MH_ERR_ARG;
    mhc::CrcParams p{};
    const int rc = prepare(d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols, d_crc, d_len,
                           d_stream_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    p.set = s->d;
    HIP_TRY(mhc::launch_crc(p, mhc::Model::Set, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int mh_crc_batch(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, uint8_t prev0,
                 const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint32_t *crc, uint64_t *len, int32_t *stream_status) {
    if (!order01(m)) return MH_ERR_ARG;
    return crc_host(m, payload, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols, crc, len, stream_status);
}

int mh_crc_batch_o2(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, uint8_t prev0,
                    const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint32_t *crc, uint64_t *len, int32_t *stream_status) {
    if (!order2(m)) return MH_ERR_ARG;
    return crc_host(m, payload, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols, crc, len, stream_status);
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
