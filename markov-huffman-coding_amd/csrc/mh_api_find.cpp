// mh_api_find.cpp — the search calls of the C ABI (include/mh.h, "SEARCH IN BATCHES"): the pattern set (a host object: the
// Shift-And automaton of mh_find.h), the device calls under one shared model or a model set (kernels: mh_find.hip) and the
// host-buffer form.
#include "mh_api_internal.hpp"
#include "mh_batch.h"
#include "mh_find.h"

using namespace mhapi;

namespace {

bool order01(const mh_model *m) { return m && (m->type == 0 || m->type == 1); }

bool offsets_ok(const uint64_t *off, size_t n) {
    if (off[0] != 0) return false;
    for (size_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

// the checks both device calls share, in the order of mh_dev_decode_batch, and the batch part of the parameters
int prepare(const mh_pattern_set *ps, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
            uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
            uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap, int32_t *d_stream_status, void *d_ws,
            size_t ws_bytes, mhf::FindParams &p) {
    if (!ps || (!d_payload && pay_total) || !d_pay_off || (!d_nbits && n_streams) || !d_hit_off || !d_ws) return MH_ERR_ARG;
    if (!aligned16(d_payload) || !aligned16(d_ws)) return MH_ERR_ARG;
    int shift = 0;
    if (d_index && ((shift = chunk_shift_of(chunk_symbols)) < 0 || !d_sym_off)) return MH_ERR_ARG;
    const uint64_t W = d_index ? mhf::work_items(n_streams, sym_total, chunk_symbols) : 0;
    const mhf::FindLayout L = mhf::find_layout(n_streams, W);
    if (ws_bytes < L.total) return MH_ERR_CAPACITY;
    p.b.payload = d_payload; p.b.pay_off = d_pay_off; p.b.nbits = d_nbits; p.b.n = n_streams; p.b.pay_total = pay_total; p.b.prev0 = prev0;
    p.b.sym_off = d_index ? reinterpret_cast<unsigned long long *>(const_cast<uint64_t *>(d_sym_off)) : nullptr;   // (read only)
    p.b.sym_total = d_index ? sym_total : 0;
    p.b.index = d_index; p.b.chunk_shift = uint32_t(shift);
    p.b.walk_max_bits = MH_BATCH_WALK_MAX_BITS;
    p.b.stream_status = d_stream_status ? d_stream_status : reinterpret_cast<int *>(static_cast<unsigned char *>(d_ws) + L.off_status);
    p.first = ps->first; p.last = ps->last; p.max_len = ps->max_len;
    p.hit_off = reinterpret_cast<unsigned long long *>(d_hit_off);
    p.hits = reinterpret_cast<unsigned long long *>(d_hits);
    p.hit_pattern = d_hits ? d_hit_pattern : nullptr;
    p.hit_cap = d_hits ? hit_cap : 0;
    return MH_OK;
}

int run(const mhf::FindParams &p, const mh_pattern_set *ps, bool shared, void *d_ws, void *stream) {
    mhf::Automaton a;
    std::memcpy(a.mask, ps->mask, sizeof a.mask);
    HIP_TRY(mhf::launch_find(p, a, shared, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

}  // namespace

extern "C" {

int mh_pattern_set_create(const uint8_t *bytes, const uint32_t *pat_off, size_t n_patterns, uint32_t flags, mh_pattern_set **out) {
    if (out) *out = nullptr;
    if (!bytes || !pat_off || !out || n_patterns == 0 || n_patterns > MH_FIND_MAX_POSITIONS || (flags & ~MH_FIND_FOLD_ASCII)) return MH_ERR_ARG;
    if (pat_off[0] != 0) return MH_ERR_ARG;
    for (size_t j = 0; j < n_patterns; ++j)
        if (pat_off[j + 1] <= pat_off[j] || pat_off[j + 1] > MH_FIND_MAX_POSITIONS) return MH_ERR_ARG;   // empty, decreasing, over the budget
    mh_pattern_set *ps = new (std::nothrow) mh_pattern_set;
    if (!ps) return MH_ERR_NOMEM;
    std::memset(ps->mask, 0, sizeof ps->mask);
    ps->n = uint32_t(n_patterns);
    ps->flags = flags;
    for (size_t j = 0; j < n_patterns; ++j) {
        const uint32_t a = pat_off[j], b = pat_off[j + 1];
        ps->first |= 1ull << a;
        ps->last |= 1ull << (b - 1);
        if (b - a > ps->max_len) ps->max_len = b - a;
        for (uint32_t k = a; k < b; ++k) {
            const uint8_t c = bytes[k];
            ps->mask[c] |= 1ull << k;
            if (flags & MH_FIND_FOLD_ASCII) {
                if (c >= 'A' && c <= 'Z') ps->mask[c + 32] |= 1ull << k;
                if (c >= 'a' && c <= 'z') ps->mask[c - 32] |= 1ull << k;
            }
        }
    }
    *out = ps;
    return MH_OK;
}

size_t mh_pattern_set_size(const mh_pattern_set *ps) { return ps ? ps->n : 0; }
int mh_pattern_set_max_len(const mh_pattern_set *ps) { return ps ? int(ps->max_len) : 0; }
void mh_pattern_set_free(mh_pattern_set *ps) { delete ps; }

size_t mh_dev_find_batch_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    const uint64_t W = chunk_shift_of(chunk_symbols) >= 0 ? mhf::work_items(n_streams, sym_total, chunk_symbols) : 0;
    return mhf::find_layout(n_streams, W).total;
}

int mh_dev_find_batch(const mh_model *m, const mh_pattern_set *ps, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                      size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                      uint32_t chunk_symbols, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                      int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order01(m)) return MH_ERR_ARG;
    mhf::FindParams p{};
    const int rc = prepare(ps, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols, d_hit_off,
                           d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    p.b.prim = m->d_prim; p.b.sec = m->d_sec; p.b.sec_base = m->d_sec_base; p.b.tree = m->d_tree;
    p.b.P = uint32_t(m->dec_bits); p.b.nsec = m->nsec; p.b.sec_lds = m->dec_lds ? 1u : 0u;
    p.b.direct = m->dec_direct ? 1u : 0u; p.b.H = uint32_t(m->dec_h);
    return run(p, ps, true, d_ws, stream);
}

int mh_dev_find_each(const mh_model_set *s, const mh_pattern_set *ps, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                     size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                     uint32_t chunk_symbols, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                     int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!s || n_streams != s->d.n) return MH_ERR_ARG;
    mhf::FindParams p{};
    const int rc = prepare(ps, d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols, d_hit_off,
                           d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    p.set = s->d;
    return run(p, ps, false, d_ws, stream);
}

int mh_find_batch(const mh_model *m, const mh_pattern_set *ps, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                  size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint64_t *hit_off,
                  uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap, int32_t *stream_status) {
    if (!order01(m) || !ps || !pay_off || (!nbits && n_streams) || !hit_off) return MH_ERR_ARG;
    if (index && (chunk_shift_of(chunk_symbols) < 0 || !sym_off)) return MH_ERR_ARG;
    if (!offsets_ok(pay_off, n_streams)) return MH_ERR_ARG;
    const uint64_t pay_total = pay_off[n_streams];
    if (!payload && pay_total) return MH_ERR_ARG;
    for (size_t i = 0; i < n_streams; ++i)
        if (nbits[i] > (pay_off[i + 1] - pay_off[i]) * 8) return MH_ERR_ARG;
    if (index && !offsets_ok(sym_off, n_streams)) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    // index-free with a stream over the walk cap: index the batch first (mh_index_batch never refuses a valid stream), then
    // search it as an indexed batch; a stream the indexing fails keeps that error and has no symbols, so no hits
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
        const int rc = mh_index_batch(m, payload, pay_off, nbits, n_streams, prev0, chunk_symbols, own_so.data(), own_idx.data(), own_idx.size(),
                                      idx_st.data());
        if (rc == MH_ERR_HIP || rc == MH_ERR_NO_DEVICE || rc == MH_ERR_NOMEM || rc == MH_ERR_CAPACITY) return rc;
        sym_off = own_so.data();
        index = own_idx.data();
    }
    const hipStream_t st = nullptr;
    const uint64_t sym_total = index ? sym_off[n_streams] : 0;
    const size_t nidx = index ? size_t(mh_batch_index_capacity(sym_total, n_streams, chunk_symbols)) : 0;
    const size_t wsb = mh_dev_find_batch_workspace(n_streams, sym_total, index ? chunk_symbols : 0);
    const uint64_t cap = hits ? hit_cap : 0;
    DevBuf d_pl, d_po, d_nb, d_so, d_idx, d_ho, d_hits, d_pat, d_st, d_ws;
    HIP_TRY(d_pl.alloc(size_t(pay_total) + 64));
    HIP_TRY(d_po.alloc((n_streams + 1) * 8));
    HIP_TRY(d_nb.alloc(n_streams * 8));
    HIP_TRY(d_so.alloc((n_streams + 1) * 8));
    HIP_TRY(d_idx.alloc(nidx * 8));
    HIP_TRY(d_ho.alloc((n_streams + 1) * 8));
    HIP_TRY(d_hits.alloc(size_t(cap) * 24));
    HIP_TRY(d_pat.alloc(size_t(cap) * 4));
    HIP_TRY(d_st.alloc(n_streams * 4));
    HIP_TRY(d_ws.alloc(wsb));
    if (pay_total) HIP_TRY(stage_h2d(d_pl.p, payload, size_t(pay_total), st));
    HIP_TRY(hipMemcpy(d_po.p, pay_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
    if (n_streams) HIP_TRY(hipMemcpy(d_nb.p, nbits, n_streams * 8, hipMemcpyHostToDevice));
    if (index) {
        HIP_TRY(hipMemcpy(d_so.p, sym_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
        if (nidx) HIP_TRY(hipMemcpy(d_idx.p, index, nidx * 8, hipMemcpyHostToDevice));
    }
    int rc = mh_dev_find_batch(m, ps, d_pl.as<uint8_t>(), d_po.as<uint64_t>(), d_nb.as<uint64_t>(), n_streams, pay_total, prev0,
                               index ? d_so.as<uint64_t>() : nullptr, sym_total, index ? d_idx.as<uint64_t>() : nullptr, chunk_symbols,
                               d_ho.as<uint64_t>(), hits ? d_hits.as<uint64_t>() : nullptr, hit_pattern ? d_pat.as<uint32_t>() : nullptr, cap,
                               d_st.as<int32_t>(), d_ws.p, wsb, st);
    if (rc != MH_OK) return rc;
    const int dev_rc = mh_dev_status(d_ws.p, st);
    std::vector<int32_t> sst(n_streams);
    if (n_streams) HIP_TRY(hipMemcpy(sst.data(), d_st.p, n_streams * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hit_off, d_ho.p, (n_streams + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t nrec = std::min<uint64_t>(hit_off[n_streams], cap);
    if (nrec) {
        HIP_TRY(hipMemcpy(hits, d_hits.p, size_t(nrec) * 24, hipMemcpyDeviceToHost));
        if (hit_pattern) HIP_TRY(hipMemcpy(hit_pattern, d_pat.p, size_t(nrec) * 4, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < idx_st.size(); ++i)
        if (idx_st[i] != MH_OK) sst[i] = idx_st[i];
    int first = MH_OK;
    for (size_t i = 0; i < n_streams && first == MH_OK; ++i) first = sst[i];
    if (first == MH_OK && dev_rc != MH_OK && dev_rc != MH_ERR_ARG) first = dev_rc;      // MH_ERR_CAPACITY: the hits do not fit
    if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
    return first;
}

}  // extern "C"
