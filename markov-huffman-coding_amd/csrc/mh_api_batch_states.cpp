// mh_api_batch_states.cpp — the segment-state calls of the C ABI (include/mh.h, "SEGMENT STATES OF INDEX-FREE BATCHES" and
// "SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES"): states, then index or emit, for a batch of index-free streams under one
// shared model of order 0/1, a model set or one shared order-2 model (kernels: mh_batch_states.hip), and the host forms
// that build a whole batch's index.
#include "mh_api_reader.hpp"
#include "mh_batch_states.h"

using namespace mhapi;

namespace {

// the arguments every device call takes; the model's part is filled by the callers
int common(mhs::StParams &p, int kind, const void *model, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
           size_t n, uint64_t pay_total, uint8_t prev0, void *d_ws, size_t ws_bytes) {
    if (!dev_batch_ptrs_ok(d_payload, pay_total, d_pay_off, d_nbits, n, d_ws)) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_batch_states_workspace(n, pay_total)) return MH_ERR_CAPACITY;
    p = mhs::StParams{};
    p.payload = d_payload; p.pay_off = d_pay_off; p.nbits = d_nbits; p.n = n; p.pay_total = pay_total;
    p.segs = mhs::segs_of(pay_total, n);
    p.prev0 = prev0;
    const bool o2 = kind == mhs::KIND_SHARED2;
    p.state0 = o2 ? (uint64_t(prev0) << 8 | prev0) << 48 : uint64_t(prev0) << 56;
    p.pos_mask = o2 ? MH_INDEX2_BIT_MASK : MH_INDEX_BIT_MASK;
    p.walk_max_bits = MH_BATCH_WALK_MAX_BITS;
    p.kind = kind;
    const unsigned long long tag[mhs::TAG_WORDS] = {
        mhs::TAG_MAGIC | unsigned(kind), n, pay_total, prev0, reinterpret_cast<uintptr_t>(d_payload),
        reinterpret_cast<uintptr_t>(d_pay_off), reinterpret_cast<uintptr_t>(d_nbits), reinterpret_cast<uintptr_t>(model)};
    std::copy(tag, tag + mhs::TAG_WORDS, p.tag);
    return MH_OK;
}

int shared_model(mhs::StParams &p, const mh_model *m) {
    if (!order01(m)) return MH_ERR_ARG;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    fill_dec_tables(m, p.tabs);
    p.lds = mhb::tables_lds(p.tabs);
    if (p.lds > 163840) return MH_ERR_ARG;
    return MH_OK;
}

int shared2_model(mhs::StParams &p, const mh_model *m) {
    if (!order2(m)) return MH_ERR_ARG;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !m->d_o2rep || !have_device()) return MH_ERR_NO_DEVICE;
    fill_dec_tables(m, p.tabs);
    p.rep = m->d_rep();
    p.live = m->d_live();
    return MH_OK;
}

int set_model(mhs::StParams &p, const mh_model_set *s, size_t n) {
    if (!s || n != s->d.n) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    p.set = s->d;
    return MH_OK;
}

int index_args(mhs::StParams &p, uint64_t *d_index, uint64_t index_cap, uint32_t chunk_symbols, int32_t *d_stream_status) {
    const int shift = chunk_shift_of(chunk_symbols);
    if (!d_index || shift < 0) return MH_ERR_ARG;
    p.index = reinterpret_cast<unsigned long long *>(d_index);
    p.index_cap = index_cap;
    p.chunk_shift = uint32_t(shift);
    p.caller_status = d_stream_status;
    return MH_OK;
}

int emit_args(mhs::StParams &p, uint8_t *d_out, uint64_t out_cap, int32_t *d_stream_status) {
    if ((!d_out && out_cap) || !aligned16(d_out)) return MH_ERR_ARG;
    p.out = d_out;
    p.out_cap = out_cap;
    p.caller_status = d_stream_status;
    return MH_OK;
}

// host forms: states and index on the device for the whole batch; a stream the device refuses (its fallback walk would
// exceed MH_BATCH_WALK_MAX_BITS) is indexed on its own by mh_dev_build_index under model_of(i)
template <class States, class Index, class ModelOf>
int index_host(const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n, uint8_t prev0, uint32_t chunk, uint64_t *sym_off,
               uint64_t *index, uint64_t index_cap, int32_t *stream_status, States states, Index dev_index, ModelOf model_of) {
    const hipStream_t st = nullptr;
    const uint64_t pay_total = pay_off[n];
    const size_t wsb = mh_dev_batch_states_workspace(n, pay_total);
    DevBatch db;                                      // (index-free: its so is where the states call writes the lengths)
    DevBuf d_st, d_ws, d_idx;
    HIP_TRY(d_st.alloc(n * 4));
    HIP_TRY(d_ws.alloc(wsb));
    int rc = db.upload({payload, pay_off, nbits, n, pay_total, prev0, nullptr, 0, nullptr, chunk}, st);
    if (rc != MH_OK) return rc;
    rc = states(db.d.payload, db.d.pay_off, db.d.nbits, pay_total, db.so.as<uint64_t>(), d_st.as<int32_t>(), d_ws.p, wsb);
    if (rc != MH_OK) return rc;
    std::vector<uint64_t> dso(n + 1);
    HIP_TRY(hipMemcpy(dso.data(), db.so.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t dcap = mh_batch_index_capacity(dso[n], n, chunk);
    HIP_TRY(d_idx.alloc(size_t(dcap) * 8));
    rc = dev_index(db.d.payload, db.d.pay_off, db.d.nbits, pay_total, d_idx.as<uint64_t>(), dcap, d_st.as<int32_t>(), d_ws.p, wsb);
    if (rc != MH_OK) return rc;
    (void)mh_dev_status(d_ws.p, st);                  // (per-stream statuses below carry every error)
    std::vector<int32_t> sst(n);
    if (n) HIP_TRY(hipMemcpy(sst.data(), d_st.p, n * 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> didx(static_cast<size_t>(dcap));
    if (dcap) HIP_TRY(hipMemcpy(didx.data(), d_idx.p, size_t(dcap) * 8, hipMemcpyDeviceToHost));
    // the refused streams, one by one (every nbits was checked against its payload before: MH_ERR_ARG here is the refusal)
    std::vector<uint64_t> count(n);
    std::vector<std::vector<uint64_t>> own(n);
    for (size_t i = 0; i < n; ++i) {
        count[i] = dso[i + 1] - dso[i];
        if (sst[i] != MH_ERR_ARG) continue;
        mh_model *m = nullptr;
        bool owned = false;
        int r = model_of(i, m, owned);
        std::unique_ptr<mh_model, void (*)(mh_model *)> hold(owned ? m : nullptr, mh_model_free);
        const uint64_t nb = nbits[i], bytes = pay_off[i + 1] - pay_off[i];
        if (r == MH_OK) {
            const int minl = mh_model_min_code_len(m) > 0 ? mh_model_min_code_len(m) : 1;
            const uint64_t cap_i = nb / uint64_t(minl) / chunk + 2;
            const size_t wsi = mh_dev_build_index_workspace(nb);
            DevBuf s_pl, s_idx, s_n, s_ws;
            HIP_TRY(s_pl.alloc(size_t(bytes) + 64));
            HIP_TRY(s_idx.alloc(size_t(cap_i) * 8));
            HIP_TRY(s_n.alloc(8));
            HIP_TRY(s_ws.alloc(wsi));
            if (bytes) HIP_TRY(stage_h2d(s_pl.p, payload + pay_off[i], size_t(bytes), st));
            r = mh_dev_build_index(m, s_pl.as<uint8_t>(), nb, prev0, s_idx.as<uint64_t>(), cap_i, chunk, s_n.as<uint64_t>(), s_ws.p,
                                   wsi, st);
            if (r == MH_OK) r = mh_dev_status(s_ws.p, st);
            uint64_t ns = 0;
            if (r == MH_OK) HIP_TRY(hipMemcpy(&ns, s_n.p, 8, hipMemcpyDeviceToHost));
            if (r == MH_OK) {
                own[i].resize(size_t(mh_index_entries(ns, chunk)));
                if (!own[i].empty()) HIP_TRY(hipMemcpy(own[i].data(), s_idx.p, own[i].size() * 8, hipMemcpyDeviceToHost));
                count[i] = ns;
            }
        }
        sst[i] = r;
    }
    // the batch's own layout: slices move from the device's offsets (refused streams counted 0 there) to the true ones
    std::vector<uint64_t> so(n + 1, 0);
    for (size_t i = 0; i < n; ++i) so[i + 1] = so[i] + (sst[i] == MH_OK ? count[i] : 0);
    int first = MH_OK;
    for (size_t i = 0; i < n && first == MH_OK; ++i) first = sst[i];
    if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
    std::copy(so.begin(), so.end(), sym_off);
    if (index_cap < mh_batch_index_capacity(so[n], n, chunk)) return MH_ERR_CAPACITY;
    for (size_t i = 0; i < n; ++i) {
        if (sst[i] != MH_OK) continue;
        const uint64_t ne = mh_index_entries(count[i], chunk);
        const uint64_t *src = own[i].empty() ? didx.data() + mh_batch_index_base(dso[i], i, chunk) : own[i].data();
        if (ne) std::memcpy(index + mh_batch_index_base(so[i], i, chunk), src, size_t(ne) * 8);
    }
    return first;
}

// the three device calls of a shared model, order 0/1 (KIND_SHARED) or order 2 (KIND_SHARED2)
int model_of_kind(mhs::StParams &p, int kind, const mh_model *m) { return kind == mhs::KIND_SHARED2 ? shared2_model(p, m) : shared_model(p, m); }

int dev_states(int kind, const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
               uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    mhs::StParams p;
    if (!d_sym_off) return MH_ERR_ARG;
    int rc = common(p, kind, m, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_ws, ws_bytes);
    if (rc == MH_OK) rc = model_of_kind(p, kind, m);
    if (rc != MH_OK) return rc;
    p.sym_off = reinterpret_cast<unsigned long long *>(d_sym_off);
    p.caller_status = d_stream_status;
    HIP_TRY(mhs::launch_states(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int dev_index(int kind, const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
              uint64_t pay_total, uint8_t prev0, uint64_t *d_index, uint64_t index_cap, uint32_t chunk_symbols, int32_t *d_stream_status,
              void *d_ws, size_t ws_bytes, void *stream) {
    mhs::StParams p;
    int rc = common(p, kind, m, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_ws, ws_bytes);
    if (rc == MH_OK) rc = index_args(p, d_index, index_cap, chunk_symbols, d_stream_status);
    if (rc == MH_OK) rc = model_of_kind(p, kind, m);
    if (rc != MH_OK) return rc;
    HIP_TRY(mhs::launch_index(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int dev_emit(int kind, const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
             uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
             void *stream) {
    mhs::StParams p;
    int rc = common(p, kind, m, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_ws, ws_bytes);
    if (rc == MH_OK) rc = emit_args(p, d_out, out_cap, d_stream_status);
    if (rc == MH_OK) rc = model_of_kind(p, kind, m);
    if (rc != MH_OK) return rc;
    HIP_TRY(mhs::launch_emit(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}
}  // namespace

extern "C" {

size_t mh_dev_batch_states_workspace(size_t n_streams, uint64_t pay_total) { return mhs::layout(n_streams, pay_total).total; }

int mh_dev_batch_states(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                        uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
                        void *stream) {
    return dev_states(mhs::KIND_SHARED, m, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_each_states(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                       uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
                       void *stream) {
    mhs::StParams p;
    if (!d_sym_off) return MH_ERR_ARG;
    int rc = common(p, mhs::KIND_SET, s, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_ws, ws_bytes);
    if (rc == MH_OK) rc = set_model(p, s, n_streams);
    if (rc != MH_OK) return rc;
    p.sym_off = reinterpret_cast<unsigned long long *>(d_sym_off);
    p.caller_status = d_stream_status;
    HIP_TRY(mhs::launch_states(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int mh_dev_batch_index(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                       uint64_t pay_total, uint8_t prev0, uint64_t *d_index, uint64_t index_cap, uint32_t chunk_symbols,
                       int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    return dev_index(mhs::KIND_SHARED, m, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_index, index_cap, chunk_symbols, d_stream_status,
                     d_ws, ws_bytes, stream);
}

int mh_dev_each_index(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                      uint64_t pay_total, uint8_t prev0, uint64_t *d_index, uint64_t index_cap, uint32_t chunk_symbols,
                      int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    mhs::StParams p;
    int rc = common(p, mhs::KIND_SET, s, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_ws, ws_bytes);
    if (rc == MH_OK) rc = index_args(p, d_index, index_cap, chunk_symbols, d_stream_status);
    if (rc == MH_OK) rc = set_model(p, s, n_streams);
    if (rc != MH_OK) return rc;
    HIP_TRY(mhs::launch_index(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int mh_dev_batch_emit(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                      uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap, int32_t *d_stream_status, void *d_ws,
                      size_t ws_bytes, void *stream) {
    return dev_emit(mhs::KIND_SHARED, m, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_out, out_cap, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_each_emit(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                     uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap, int32_t *d_stream_status, void *d_ws,
                     size_t ws_bytes, void *stream) {
    mhs::StParams p;
    int rc = common(p, mhs::KIND_SET, s, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_ws, ws_bytes);
    if (rc == MH_OK) rc = emit_args(p, d_out, out_cap, d_stream_status);
    if (rc == MH_OK) rc = set_model(p, s, n_streams);
    if (rc != MH_OK) return rc;
    HIP_TRY(mhs::launch_emit(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

/* ------------------------------------------------------- order 2 */

size_t mh_dev_batch_states_o2_workspace(size_t n_streams, uint64_t pay_total) { return mh_dev_batch_states_workspace(n_streams, pay_total); }

int mh_dev_batch_states_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                           uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
                           void *stream) {
    return dev_states(mhs::KIND_SHARED2, m, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_batch_index_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                          uint64_t pay_total, uint8_t prev0, uint64_t *d_index, uint64_t index_cap, uint32_t chunk_symbols,
                          int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    return dev_index(mhs::KIND_SHARED2, m, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_index, index_cap, chunk_symbols, d_stream_status,
                     d_ws, ws_bytes, stream);
}

int mh_dev_batch_emit_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                         uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap, int32_t *d_stream_status, void *d_ws,
                         size_t ws_bytes, void *stream) {
    return dev_emit(mhs::KIND_SHARED2, m, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_out, out_cap, d_stream_status, d_ws, ws_bytes, stream);
}

// what the states call left in the header: the repair launches that rewrote a record, the streams the one-lane walk walked
int mh_dev_batch_states_stats(const void *d_ws, void *stream, uint32_t *repair_passes_run, uint64_t *streams_walked) {
    if (!d_ws || !repair_passes_run || !streams_walked) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char hdr[mhs::HDR_BYTES];
    HIP_TRY(hipMemcpyAsync(hdr, d_ws, sizeof hdr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int words[mhs::HDR_BYTES / 4];
    unsigned long long tag0;
    std::memcpy(words, hdr, sizeof hdr);
    std::memcpy(&tag0, hdr + mhs::HDR_TAG, 8);
    const unsigned long long kind = tag0 & 0xFFFFFFFFull;
    if ((tag0 & ~0xFFFFFFFFull) != mhs::TAG_MAGIC || kind < mhs::KIND_SHARED || kind > mhs::KIND_SHARED2) return MH_ERR_ARG;   // no states in d_ws
    uint32_t passes = 0;
    for (int pass = 1; pass <= mhs::REPAIR_PASSES; ++pass) passes += words[mhs::HDR_CHANGED + pass] != 0;
    *repair_passes_run = passes;
    *streams_walked = uint64_t(uint32_t(words[mhs::HDR_WALKED]));
    return MH_OK;
}

/* ------------------------------------------------------- host-buffer calls */

static int host_args(const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n, uint32_t chunk, const uint64_t *sym_off,
                     const uint64_t *index) {
    if (!sym_off || !index) return MH_ERR_ARG;         // both are outputs: the batch itself is index-free
    CodedBatch a{payload, pay_off, nbits, n, 0, 0, nullptr, 0, nullptr, chunk};
    return host_batch_args(a, true);
}

int mh_index_batch(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, uint8_t prev0,
                   uint32_t chunk_symbols, uint64_t *sym_off, uint64_t *index, uint64_t index_cap, int32_t *stream_status) {
    if (!order01(m)) return MH_ERR_ARG;
    int rc = host_args(payload, pay_off, nbits, n_streams, chunk_symbols, sym_off, index);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    auto states = [&](const uint8_t *pl, const uint64_t *po, const uint64_t *nb, uint64_t pt, uint64_t *so, int32_t *st, void *ws, size_t wsb) {
        return mh_dev_batch_states(m, pl, po, nb, n_streams, pt, prev0, so, st, ws, wsb, nullptr);
    };
    auto dev_index = [&](const uint8_t *pl, const uint64_t *po, const uint64_t *nb, uint64_t pt, uint64_t *idx, uint64_t cap, int32_t *st, void *ws,
                         size_t wsb) {
        return mh_dev_batch_index(m, pl, po, nb, n_streams, pt, prev0, idx, cap, chunk_symbols, st, ws, wsb, nullptr);
    };
    auto model_of = [&](size_t, mh_model *&out, bool &owned) { out = const_cast<mh_model *>(m); owned = false; return MH_OK; };
    return index_host(payload, pay_off, nbits, n_streams, prev0, chunk_symbols, sym_off, index, index_cap, stream_status, states, dev_index, model_of);
}

int mh_index_batch_o2(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, uint8_t prev0,
                      uint32_t chunk_symbols, uint64_t *sym_off, uint64_t *index, uint64_t index_cap, int32_t *stream_status) {
    if (!order2(m)) return MH_ERR_ARG;
    int rc = host_args(payload, pay_off, nbits, n_streams, chunk_symbols, sym_off, index);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    auto states = [&](const uint8_t *pl, const uint64_t *po, const uint64_t *nb, uint64_t pt, uint64_t *so, int32_t *st, void *ws, size_t wsb) {
        return mh_dev_batch_states_o2(m, pl, po, nb, n_streams, pt, prev0, so, st, ws, wsb, nullptr);
    };
    auto dev_index = [&](const uint8_t *pl, const uint64_t *po, const uint64_t *nb, uint64_t pt, uint64_t *idx, uint64_t cap, int32_t *st, void *ws,
                         size_t wsb) {
        return mh_dev_batch_index_o2(m, pl, po, nb, n_streams, pt, prev0, idx, cap, chunk_symbols, st, ws, wsb, nullptr);
    };
    auto model_of = [&](size_t, mh_model *&out, bool &owned) { out = const_cast<mh_model *>(m); owned = false; return MH_OK; };
    return index_host(payload, pay_off, nbits, n_streams, prev0, chunk_symbols, sym_off, index, index_cap, stream_status, states, dev_index, model_of);
}

int mh_index_each(const uint8_t *tables, const uint64_t *tab_off, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                  size_t n_streams, uint8_t prev0, uint32_t chunk_symbols, uint64_t *sym_off, uint64_t *index, uint64_t index_cap,
                  int32_t *stream_status) {
    if (!tab_off || !offsets_ok(tab_off, n_streams) || (!tables && tab_off[n_streams])) return MH_ERR_ARG;
    int rc = host_args(payload, pay_off, nbits, n_streams, chunk_symbols, sym_off, index);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    mh_model_set *s = nullptr;
    if ((rc = mh_model_set_from_tables(tables, tab_off, n_streams, &s)) != MH_OK) return rc;
    std::unique_ptr<mh_model_set, void (*)(mh_model_set *)> hold(s, mh_model_set_free);
    auto states = [&](const uint8_t *pl, const uint64_t *po, const uint64_t *nb, uint64_t pt, uint64_t *so, int32_t *st, void *ws, size_t wsb) {
        return mh_dev_each_states(s, pl, po, nb, n_streams, pt, prev0, so, st, ws, wsb, nullptr);
    };
    auto dev_index = [&](const uint8_t *pl, const uint64_t *po, const uint64_t *nb, uint64_t pt, uint64_t *idx, uint64_t cap, int32_t *st, void *ws,
                         size_t wsb) {
        return mh_dev_each_index(s, pl, po, nb, n_streams, pt, prev0, idx, cap, chunk_symbols, st, ws, wsb, nullptr);
    };
    auto model_of = [&](size_t i, mh_model *&out, bool &owned) {
        owned = true;
        const size_t len = size_t(tab_off[i + 1] - tab_off[i]);
        return len ? mh_model_from_table_bits(tables + tab_off[i], len, &out) : MH_ERR_CORRUPT;
    };
    return index_host(payload, pay_off, nbits, n_streams, prev0, chunk_symbols, sym_off, index, index_cap, stream_status, states, dev_index, model_of);
}

}  // extern "C"
