// mh_api_batch.cpp — the batch calls of the C ABI (include/mh.h, "BATCHES OF INDEPENDENT STREAMS"): many small order-0/1
// streams under one shared model in a few launches (kernels: mh_batch.hip), and their host-buffer forms.  The device decode
// call of the order-2 batches (mh_api_batch_o2.cpp has the rest of that family) is the second entry of the one here.
#include "mh_api_reader.hpp"
#include "mh_each.h"

using namespace mhapi;

namespace {

// mh_dev_decode_batch (o2 = false: an order-0/1 model) and mh_dev_decode_batch_o2 (an order-2 model)
int dev_decode_batch(const mh_model *m, bool o2, const CodedBatch &a, uint8_t *d_out, uint64_t out_cap, int32_t *d_stream_status, void *d_ws,
                     size_t ws_bytes, void *stream) {
    if (!(o2 ? order2(m) : order01(m)) || !a.sym_off || (!d_out && out_cap) || !aligned16(d_out)) return MH_ERR_ARG;
    const mhb::DecLayout L = mhb::dec_layout(a.n);
    mhb::DecodeParams p{};
    mhb::DecBatchParams &b = p.b;
    const int rc = dev_batch_params(a, SymOff::Through, ctx_of_prev0(m, a.prev0), d_ws, ws_bytes, L.total, L.off_status, d_stream_status, b);
    if (rc != MH_OK) return rc;
    if (a.index && a.sym_total > out_cap) return MH_ERR_CAPACITY;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    b.out = d_out; b.out_cap = out_cap;
    fill_dec_tables(m, b);
    HIP_TRY(mhb::launch_decode(p, o2 ? mhb::Model::Shared2 : mhb::Model::Shared, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

}  // namespace

extern "C" {

uint64_t mh_batch_index_base(uint64_t in_off, uint64_t stream, uint32_t chunk_symbols) {
    return chunk_symbols ? in_off / chunk_symbols + stream : 0;
}

uint64_t mh_batch_index_capacity(uint64_t total, uint64_t n_streams, uint32_t chunk_symbols) {
    return chunk_symbols ? total / chunk_symbols + n_streams + 1 : 0;
}

size_t mh_dev_histogram_batch_workspace(size_t total) {
    const size_t h = mh_dev_histogram_workspace(total);
    return h > 256 ? h : 256;
}

static int histogram_batch(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint8_t prev0,
                           uint64_t *d_counts, void *d_ws, size_t ws_bytes, void *stream, int order) {
    if ((!d_data && total) || !d_in_off || !d_counts || !d_ws || !aligned16(d_data) || !aligned16(d_ws)) return MH_ERR_ARG;
    if (ws_bytes < 256) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    if (order) {
        rc = mh_dev_histogram_o1(d_data, total, prev0, d_counts, d_ws, ws_bytes, stream);   // clears the status word, checks the sum
    } else {
        HIP_TRY(hipMemsetAsync(d_ws, 0, 64, st));
        rc = mh_dev_histogram_o0(d_data, total, d_counts, nullptr, 0, stream);
    }
    if (rc != MH_OK) return rc;
    HIP_TRY(mhb::launch_hist_fixup(d_data, d_in_off, n_streams, total, prev0, reinterpret_cast<unsigned long long *>(d_counts), order,
                                   static_cast<int *>(d_ws), st));
    return MH_OK;
}

int mh_dev_histogram_o1_batch(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint8_t prev0,
                              uint64_t *d_counts, void *d_ws, size_t ws_bytes, void *stream) {
    return histogram_batch(d_data, d_in_off, n_streams, total, prev0, d_counts, d_ws, ws_bytes, stream, 1);
}

int mh_dev_histogram_o0_batch(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint64_t *d_counts,
                              void *d_ws, size_t ws_bytes, void *stream) {
    return histogram_batch(d_data, d_in_off, n_streams, total, MH_PREV0, d_counts, d_ws, ws_bytes, stream, 0);
}

size_t mh_encode_batch_bound(const mh_model *m, size_t total, size_t n_streams) {
    size_t maxlen = m ? size_t(m->max_len) : 64;
    if (maxlen < 1) maxlen = 1;
    return (total * maxlen + 7) / 8 + n_streams + 16;            // + one partial byte per stream
}

size_t mh_dev_encode_batch_workspace(size_t n_streams, size_t total) { return mhb::enc_layout(n_streams, total).total; }

int mh_dev_encode_batch(const mh_model *m, const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint8_t prev0,
                        uint8_t *d_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_nbits, uint64_t *d_index, uint32_t chunk_symbols,
                        void *d_ws, size_t ws_bytes, void *stream) {
    if (!order01(m) || (!d_data && total) || !d_in_off || !d_out_off || (!d_nbits && n_streams) || (!d_payload && cap) || !d_ws) return MH_ERR_ARG;
    if (!aligned16(d_payload) || !aligned16(d_ws)) return MH_ERR_ARG;
    const int shift = d_index ? chunk_shift_of(chunk_symbols) : 0;
    if (shift < 0) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_encode_batch_workspace(n_streams, total)) return MH_ERR_CAPACITY;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_enc16 || !have_device()) return MH_ERR_NO_DEVICE;
    mhb::EncBatchParams p{};
    p.data = d_data; p.in_off = d_in_off; p.n = n_streams; p.total = total; p.prev0 = prev0;
    p.chunk_shift = uint32_t(shift);
    p.index = reinterpret_cast<unsigned long long *>(d_index);
    p.out = d_payload; p.cap = cap;
    p.out_off = reinterpret_cast<unsigned long long *>(d_out_off);
    p.nbits = reinterpret_cast<unsigned long long *>(d_nbits);
    p.enc16 = m->d_enc16; p.len_slot = m->d_len_slot; p.len8 = m->d_len8; p.code64 = m->d_code64; p.max_len = m->max_len;
    HIP_TRY(mhb::launch_encode_batch(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

size_t mh_dev_decode_batch_workspace(size_t n_streams) { return mhb::dec_layout(n_streams).total; }

size_t mh_dev_decode_batch_o2_workspace(size_t n_streams) { return mhb::dec_layout(n_streams).total; }

int mh_dev_decode_batch(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                        uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap, uint64_t *d_sym_off, uint64_t sym_total,
                        const uint64_t *d_index, uint32_t chunk_symbols, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    return dev_decode_batch(m, false, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols}, d_out,
                            out_cap, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_decode_batch_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                           uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap, uint64_t *d_sym_off, uint64_t sym_total,
                           const uint64_t *d_index, uint32_t chunk_symbols, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    return dev_decode_batch(m, true, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols}, d_out,
                            out_cap, d_stream_status, d_ws, ws_bytes, stream);
}

}  // extern "C"

/* ------------------------------------------------------- host-buffer calls */

// The host-buffer bodies, shared with the order-2 batch calls (mh_api_batch_o2.cpp): `dev` is the device call of the family,
// the caller has checked the model's order.
int mhapi::encode_batch_host(const mh_model *m, const uint8_t *data, const uint64_t *in_off, size_t n_streams, uint8_t prev0,
                             uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *nbits, uint64_t *index, uint32_t chunk_symbols,
                             DevEncodeBatchFn dev) {
    if (!m || !in_off || !out_off || (!nbits && n_streams) || (!out_payload && cap)) return MH_ERR_ARG;
    if (index && chunk_shift_of(chunk_symbols) < 0) return MH_ERR_ARG;
    if (!offsets_ok(in_off, n_streams)) return MH_ERR_ARG;
    const size_t total = size_t(in_off[n_streams]);
    if (!data && total) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    const hipStream_t st = nullptr;
    const size_t bound = mh_encode_batch_bound(m, total, n_streams);
    const size_t dcap = cap < bound ? cap : bound;
    const size_t nidx = index ? size_t(mh_batch_index_capacity(total, n_streams, chunk_symbols)) : 0;
    const size_t wsb = mh_dev_encode_batch_workspace(n_streams, total);
    DevBuf d_data, d_in, d_out, d_oo, d_nb, d_idx, d_ws;
    HIP_TRY(d_data.alloc(total));
    HIP_TRY(d_in.alloc((n_streams + 1) * 8));
    HIP_TRY(d_out.alloc(dcap));
    HIP_TRY(d_oo.alloc((n_streams + 1) * 8));
    HIP_TRY(d_nb.alloc(n_streams * 8));
    HIP_TRY(d_idx.alloc(nidx * 8));
    HIP_TRY(d_ws.alloc(wsb));
    if (total) HIP_TRY(stage_h2d(d_data.p, data, total, st));
    HIP_TRY(hipMemcpy(d_in.p, in_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
    if (nidx) HIP_TRY(hipMemcpy(d_idx.p, index, nidx * 8, hipMemcpyHostToDevice));   // gap entries stay what the caller had
    int rc = dev(m, d_data.as<uint8_t>(), d_in.as<uint64_t>(), n_streams, total, prev0, d_out.as<uint8_t>(), dcap,
                 d_oo.as<uint64_t>(), d_nb.as<uint64_t>(), index ? d_idx.as<uint64_t>() : nullptr, chunk_symbols, d_ws.p, wsb, st);
    if (rc == MH_OK) rc = mh_dev_status(d_ws.p, st);
    if (rc != MH_OK) return rc;
    HIP_TRY(hipMemcpy(out_off, d_oo.p, (n_streams + 1) * 8, hipMemcpyDeviceToHost));
    if (n_streams) HIP_TRY(hipMemcpy(nbits, d_nb.p, n_streams * 8, hipMemcpyDeviceToHost));
    if (out_off[n_streams]) HIP_TRY(stage_d2h(out_payload, d_out.p, size_t(out_off[n_streams]), st));
    if (nidx) HIP_TRY(hipMemcpy(index, d_idx.p, nidx * 8, hipMemcpyDeviceToHost));
    return MH_OK;
}

int mhapi::decode_batch_host(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams,
                             uint8_t prev0, uint8_t *out, size_t out_cap, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                             int32_t *stream_status, DevDecodeBatchFn dev) {
    if (!m || !sym_off || (!out && out_cap)) return MH_ERR_ARG;
    CodedBatch a{payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols};
    int rc = host_batch_args(a, index != nullptr);
    if (rc != MH_OK) return rc;
    if (a.sym_total > out_cap) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    const hipStream_t st = nullptr;
    // index-free: the output is at most nbits / (shortest code) bytes per stream; streams over the walk cap go through mh_decode
    std::vector<size_t> long_streams;
    uint64_t dcap = a.sym_total;
    if (!index) {
        const uint64_t minl = uint64_t(m->min_len > 0 ? m->min_len : 1);
        uint64_t bound = 0;
        for (size_t i = 0; i < n_streams; ++i) {
            if (nbits[i] > MH_BATCH_WALK_MAX_BITS) long_streams.push_back(i);
            else bound += nbits[i] / minl;
        }
        dcap = std::min<uint64_t>(out_cap, bound);
    }
    const size_t wsb = mh_dev_decode_batch_workspace(n_streams);
    DevBatch db;
    DevBuf d_out, d_st, d_ws;
    HIP_TRY(d_out.alloc(size_t(dcap)));
    HIP_TRY(d_st.alloc(n_streams * 4));
    HIP_TRY(d_ws.alloc(wsb));
    if ((rc = db.upload(a, st)) != MH_OK) return rc;
    rc = dev(m, db.d.payload, db.d.pay_off, db.d.nbits, n_streams, a.pay_total, prev0, d_out.as<uint8_t>(), dcap, db.so.as<uint64_t>(), a.sym_total,
             db.d.index, chunk_symbols, d_st.as<int32_t>(), d_ws.p, wsb, st);
    if (rc != MH_OK) return rc;
    const int dev_rc = mh_dev_status(d_ws.p, st);
    std::vector<int32_t> sst(n_streams);
    if (n_streams) HIP_TRY(hipMemcpy(sst.data(), d_st.p, n_streams * 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> dso(n_streams + 1);
    HIP_TRY(hipMemcpy(dso.data(), db.so.p, (n_streams + 1) * 8, hipMemcpyDeviceToHost));
    // the streams the device walk refused (over MH_BATCH_WALK_MAX_BITS) decode one by one; their bytes go in between
    std::vector<std::vector<uint8_t>> extra(long_streams.size());
    for (size_t k = 0; k < long_streams.size(); ++k) {
        const size_t i = long_streams[k];
        size_t nb = 0;
        const int r = mh_decode_to(m, payload + pay_off[i], nbits[i], prev0, grow_vec, &extra[k], &nb, nullptr, 0, 0);
        extra[k].resize(nb);
        sst[i] = r;
    }
    const int first = first_failure(sst, {}, dev_rc);
    if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
    if (!long_streams.empty()) return splice_alone(dso, d_out.p, long_streams, extra, out, out_cap, sym_off, first, st);
    std::copy(dso.begin(), dso.end(), sym_off);
    if (dso[n_streams] && dso[n_streams] <= out_cap) HIP_TRY(stage_d2h(out, d_out.p, size_t(dso[n_streams]), st));   // (a failed stream's bytes are undefined, its neighbours' are not)
    return first;
}

extern "C" {

int mh_encode_batch(const mh_model *m, const uint8_t *data, const uint64_t *in_off, size_t n_streams, uint8_t prev0,
                    uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *nbits, uint64_t *index, uint32_t chunk_symbols) {
    if (!order01(m)) return MH_ERR_ARG;
    return encode_batch_host(m, data, in_off, n_streams, prev0, out_payload, cap, out_off, nbits, index, chunk_symbols, mh_dev_encode_batch);
}

int mh_decode_batch(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, uint8_t prev0,
                    uint8_t *out, size_t out_cap, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, int32_t *stream_status) {
    if (!order01(m)) return MH_ERR_ARG;
    return decode_batch_host(m, payload, pay_off, nbits, n_streams, prev0, out, out_cap, sym_off, index, chunk_symbols, stream_status,
                             mh_dev_decode_batch);
}

}  // extern "C"
