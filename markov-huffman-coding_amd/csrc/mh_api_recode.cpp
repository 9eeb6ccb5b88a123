// mh_api_recode.cpp — the re-coding calls of the C ABI (include/mh.h, "RE-CODING BATCHES"): the training histogram of a
// compressed batch and the batch coded again under another model, under one shared source model or a model set (kernels:
// mh_recode.hip), and the host-buffer form.
#include "mh_api_internal.hpp"
#include "mh_batch.h"
#include "mh_recode.h"

using namespace mhapi;

namespace {

// the source batch, checked in the order of mh_dev_decode_batch; sym_off is written by an index-free re-code
int source(const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
           const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, const void *d_ws, mhr::Src &s) {
    if ((!d_payload && pay_total) || !d_pay_off || (!d_nbits && n_streams) || !d_ws) return MH_ERR_ARG;
    if (!aligned16(d_payload) || !aligned16(d_ws)) return MH_ERR_ARG;
    int shift = 0;
    if (d_index && ((shift = chunk_shift_of(chunk_symbols)) < 0 || !d_sym_off)) return MH_ERR_ARG;
    s.b.payload = d_payload; s.b.pay_off = d_pay_off; s.b.nbits = d_nbits; s.b.n = n_streams; s.b.pay_total = pay_total; s.b.prev0 = prev0;
    s.b.sym_off = reinterpret_cast<unsigned long long *>(const_cast<uint64_t *>(d_sym_off));
    s.b.sym_total = sym_total;
    s.b.index = d_index; s.b.chunk_shift = uint32_t(shift);
    s.b.walk_max_bits = MH_BATCH_WALK_MAX_BITS;
    return MH_OK;
}

int shared_tables(const mh_model *m, mhr::Src &s) {
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    fill_dec_tables(m, s.b);
    return MH_OK;
}

int histogram_coded(const mh_model *m, const mh_model_set *set, int order, const uint8_t *d_payload, const uint64_t *d_pay_off,
                    const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                    const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_counts, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
                    void *stream) {
    if (set ? n_streams != set->d.n : !order01(m)) return MH_ERR_ARG;
    if ((order != 0 && order != 1) || !d_counts) return MH_ERR_ARG;
    mhr::HistParams p{};
    const int rc = source(d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols, d_ws, p.s);
    if (rc != MH_OK) return rc;
    const mhr::HistLayout L = mhr::hist_layout(n_streams);
    if (ws_bytes < L.total) return MH_ERR_CAPACITY;
    p.s.b.stream_status = d_stream_status ? d_stream_status : reinterpret_cast<int *>(static_cast<unsigned char *>(d_ws) + L.off_status);
    p.order = uint32_t(order);
    p.counts = reinterpret_cast<unsigned long long *>(d_counts);
    if (set) {
        if (!have_device()) return MH_ERR_NO_DEVICE;
        p.s.set = set->d;
    } else {
        const int t = shared_tables(m, p.s);
        if (t != MH_OK) return t;
    }
    HIP_TRY(mhr::launch_histogram_coded(p, !set, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int recode(const mh_model *m, const mh_model_set *set, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
           const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total,
           const uint64_t *d_index, uint32_t chunk_symbols, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits,
           uint64_t *d_out_index, uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (set ? n_streams != set->d.n : !order01(m)) return MH_ERR_ARG;
    if (!order01(dst) || !d_out_off || (!d_out_nbits && n_streams)) return MH_ERR_ARG;
    if (!d_index && !d_sym_off) return MH_ERR_ARG;                    // index-free: the decoded lengths are an output
    mhr::RecodeParams p{};
    const int rc = source(d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols, d_ws, p.s);
    if (rc != MH_OK) return rc;
    if (!aligned16(d_out_payload)) return MH_ERR_ARG;
    int oshift = int(p.s.b.chunk_shift);
    if (!d_index && d_out_index && (oshift = chunk_shift_of(chunk_symbols)) < 0) return MH_ERR_ARG;
    const uint64_t W = d_index ? mhb::work_items(n_streams, sym_total, chunk_symbols) : 0;
    const mhr::RecodeLayout L = mhr::recode_layout(n_streams, W);
    if (ws_bytes < L.total) return MH_ERR_CAPACITY;
    p.s.b.stream_status = d_stream_status ? d_stream_status : reinterpret_cast<int *>(static_cast<unsigned char *>(d_ws) + L.off_status);
    p.out = d_out_payload; p.cap = d_out_payload ? cap : 0;
    p.out_off = reinterpret_cast<unsigned long long *>(d_out_off);
    p.out_nbits = reinterpret_cast<unsigned long long *>(d_out_nbits);
    p.out_index = reinterpret_cast<unsigned long long *>(d_out_index);
    p.dropped = reinterpret_cast<unsigned long long *>(d_dropped);
    p.out_chunk_shift = uint32_t(oshift);
    if (dst->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (set) {
        if (!have_device()) return MH_ERR_NO_DEVICE;
        p.s.set = set->d;
    } else {
        const int t = shared_tables(m, p.s);
        if (t != MH_OK) return t;
    }
    if (!dst->d_len8 || !dst->d_code64) return MH_ERR_NO_DEVICE;
    p.dst.len8 = dst->d_len8;
    p.dst.code64 = reinterpret_cast<const unsigned long long *>(dst->d_code64);
    p.dst.ctx_mask = dst->type ? 0xFFu : 0u;
    HIP_TRY(mhr::launch_recode(p, !set, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

}  // namespace

extern "C" {

size_t mh_dev_histogram_coded_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    (void)sym_total; (void)chunk_symbols;                             // the counting keeps nothing per chunk
    return mhr::hist_layout(n_streams).total;
}

int mh_dev_histogram_coded_batch(const mh_model *src, int order, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                                 size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                                 const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_counts, int32_t *d_stream_status, void *d_ws,
                                 size_t ws_bytes, void *stream) {
    if (!src) return MH_ERR_ARG;
    return histogram_coded(src, nullptr, order, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index,
                           chunk_symbols, d_counts, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_histogram_coded_each(const mh_model_set *src, int order, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                                size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                                const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_counts, int32_t *d_stream_status, void *d_ws,
                                size_t ws_bytes, void *stream) {
    if (!src) return MH_ERR_ARG;
    return histogram_coded(nullptr, src, order, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index,
                           chunk_symbols, d_counts, d_stream_status, d_ws, ws_bytes, stream);
}

size_t mh_dev_recode_batch_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    const uint64_t W = chunk_shift_of(chunk_symbols) >= 0 ? mhb::work_items(n_streams, sym_total, chunk_symbols) : 0;
    return mhr::recode_layout(n_streams, W).total;
}

int mh_dev_recode_batch(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                        size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                        uint32_t chunk_symbols, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits,
                        uint64_t *d_out_index, uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!src) return MH_ERR_ARG;
    return recode(src, nullptr, dst, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols,
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_recode_each(const mh_model_set *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                       size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                       uint32_t chunk_symbols, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits,
                       uint64_t *d_out_index, uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!src) return MH_ERR_ARG;
    return recode(nullptr, src, dst, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols,
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_recode_batch(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                    size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint8_t *out_payload,
                    size_t cap, uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_index, uint64_t *dropped, int32_t *stream_status) {
    if (!order01(src) || !order01(dst) || !pay_off || (!nbits && n_streams) || !out_off || (!out_nbits && n_streams) || !sym_off)
        return MH_ERR_ARG;
    if ((index || out_index) && chunk_shift_of(chunk_symbols) < 0) return MH_ERR_ARG;
    if (!offsets_ok(pay_off, n_streams)) return MH_ERR_ARG;
    const uint64_t pay_total = pay_off[n_streams];
    if (!payload && pay_total) return MH_ERR_ARG;
    for (size_t i = 0; i < n_streams; ++i)
        if (nbits[i] > (pay_off[i + 1] - pay_off[i]) * 8) return MH_ERR_ARG;
    if (index && !offsets_ok(sym_off, n_streams)) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (src->max_len > mh::MAX_CODE_BITS || dst->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    // index-free with a stream over the walk cap: index the batch first (mh_index_batch never refuses a valid stream), then
    // re-code it as an indexed batch; a stream the indexing fails keeps that error and has no symbols, so no payload
    const uint64_t minl = uint64_t(src->min_len > 0 ? src->min_len : 1);
    uint64_t bound = 0;
    for (size_t i = 0; i < n_streams; ++i) bound += nbits[i] / minl;
    std::vector<uint64_t> own_idx;
    std::vector<int32_t> idx_st;
    bool over = false;
    if (!index)
        for (size_t i = 0; i < n_streams && !over; ++i) over = nbits[i] > MH_BATCH_WALK_MAX_BITS;
    if (over) {
        if (!out_index) chunk_symbols = MH_CHUNK_DEFAULT;
        own_idx.assign(size_t(mh_batch_index_capacity(bound, n_streams, chunk_symbols)), 0);
        idx_st.assign(n_streams, MH_OK);
        const int rc = mh_index_batch(src, payload, pay_off, nbits, n_streams, prev0, chunk_symbols, sym_off, own_idx.data(), own_idx.size(),
                                      idx_st.data());
        if (rc == MH_ERR_HIP || rc == MH_ERR_NO_DEVICE || rc == MH_ERR_NOMEM || rc == MH_ERR_CAPACITY) return rc;
        index = own_idx.data();
    }
    const hipStream_t st = nullptr;
    const uint64_t sym_total = index ? sym_off[n_streams] : bound;    // index-free: what the destination index is sized for
    const size_t nidx = index ? size_t(mh_batch_index_capacity(sym_total, n_streams, chunk_symbols)) : 0;
    const size_t noidx = out_index ? size_t(mh_batch_index_capacity(sym_total, n_streams, chunk_symbols)) : 0;
    const size_t wsb = mh_dev_recode_batch_workspace(n_streams, sym_total, index ? chunk_symbols : 0);
    const size_t dcap = out_payload ? cap : 0;
    DevBuf d_pl, d_po, d_nb, d_so, d_idx, d_out, d_oo, d_onb, d_oidx, d_drop, d_st, d_ws;
    HIP_TRY(d_pl.alloc(size_t(pay_total) + 64));
    HIP_TRY(d_po.alloc((n_streams + 1) * 8));
    HIP_TRY(d_nb.alloc(n_streams * 8));
    HIP_TRY(d_so.alloc((n_streams + 1) * 8));
    HIP_TRY(d_idx.alloc(nidx * 8));
    HIP_TRY(d_out.alloc(dcap));
    HIP_TRY(d_oo.alloc((n_streams + 1) * 8));
    HIP_TRY(d_onb.alloc(n_streams * 8));
    HIP_TRY(d_oidx.alloc(noidx * 8));
    HIP_TRY(d_drop.alloc(n_streams * 8));
    HIP_TRY(d_st.alloc(n_streams * 4));
    HIP_TRY(d_ws.alloc(wsb));
    if (pay_total) HIP_TRY(stage_h2d(d_pl.p, payload, size_t(pay_total), st));
    HIP_TRY(hipMemcpy(d_po.p, pay_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
    if (n_streams) HIP_TRY(hipMemcpy(d_nb.p, nbits, n_streams * 8, hipMemcpyHostToDevice));
    if (index) {
        HIP_TRY(hipMemcpy(d_so.p, sym_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
        if (nidx) HIP_TRY(hipMemcpy(d_idx.p, index, nidx * 8, hipMemcpyHostToDevice));
    }
    if (noidx) HIP_TRY(hipMemcpy(d_oidx.p, out_index, noidx * 8, hipMemcpyHostToDevice));   // gap entries stay what the caller had
    int rc = mh_dev_recode_batch(src, dst, d_pl.as<uint8_t>(), d_po.as<uint64_t>(), d_nb.as<uint64_t>(), n_streams, pay_total, prev0,
                                 d_so.as<uint64_t>(), sym_total, index ? d_idx.as<uint64_t>() : nullptr, chunk_symbols,
                                 out_payload ? d_out.as<uint8_t>() : nullptr, dcap, d_oo.as<uint64_t>(), d_onb.as<uint64_t>(),
                                 out_index ? d_oidx.as<uint64_t>() : nullptr, d_drop.as<uint64_t>(), d_st.as<int32_t>(), d_ws.p, wsb, st);
    if (rc != MH_OK) return rc;
    const int dev_rc = mh_dev_status(d_ws.p, st);
    std::vector<int32_t> sst(n_streams);
    if (n_streams) HIP_TRY(hipMemcpy(sst.data(), d_st.p, n_streams * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_off, d_oo.p, (n_streams + 1) * 8, hipMemcpyDeviceToHost));
    if (n_streams) HIP_TRY(hipMemcpy(out_nbits, d_onb.p, n_streams * 8, hipMemcpyDeviceToHost));
    if (n_streams && dropped) HIP_TRY(hipMemcpy(dropped, d_drop.p, n_streams * 8, hipMemcpyDeviceToHost));
    if (!index) HIP_TRY(hipMemcpy(sym_off, d_so.p, (n_streams + 1) * 8, hipMemcpyDeviceToHost));
    if (out_payload && out_off[n_streams] && out_off[n_streams] <= dcap && dev_rc != MH_ERR_CAPACITY)
        HIP_TRY(stage_d2h(out_payload, d_out.p, size_t(out_off[n_streams]), st));
    if (noidx && dev_rc != MH_ERR_CAPACITY) HIP_TRY(hipMemcpy(out_index, d_oidx.p, noidx * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < idx_st.size(); ++i)
        if (idx_st[i] != MH_OK) sst[i] = idx_st[i];
    int first = MH_OK;
    for (size_t i = 0; i < n_streams && first == MH_OK; ++i) first = sst[i];
    if (first == MH_OK && dev_rc != MH_OK && dev_rc != MH_ERR_ARG) first = dev_rc;      // MH_ERR_CAPACITY: the payload does not fit
    if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
    return first;
}

}  // extern "C"
