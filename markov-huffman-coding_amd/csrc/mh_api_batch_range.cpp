// mh_api_batch_range.cpp — lookups (stream, begin, end) into a batch of streams (include/mh.h, "RANDOM ACCESS INTO BATCHES"
// and "RANDOM ACCESS INTO ORDER-2 STREAMS"): the device calls under one shared model of any order or under a model set
// (kernels: mh_range.hip), and the host-buffer forms that upload only the streams the lookups touch.
#include "mh_api_reader.hpp"
#include "mh_range.h"

#include <memory>
#include <unordered_map>

using namespace mhapi;

namespace {

thread_local uint64_t t_batch_range_upload = 0;   // payload bytes the calling thread's last host form uploaded

// ------------------------------------------------------------------------------------------------ host forms

// What the host forms decode with: one shared model, or the table files of one model per stream.
struct Models {
    const mh_model *m = nullptr;                                  // shared model
    bool o2 = false;                                              // ... of order 2 (mh_decode_batch_o2_ranges)
    const uint8_t *tables = nullptr;                              // per-stream tables (m == nullptr)
    uint64_t tables_bytes = 0;
    const uint64_t *tab_off = nullptr;
};

struct Batch {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const uint64_t *pay_off, *nbits;
    size_t n;
    uint8_t prev0;
    const uint64_t *sym_off, *index;
    uint32_t chunk;
};

// A stream too large to batch: through the single-stream calls (indexed: mh_decode_ranges or mh_decode_ranges_o2 on its
// slice, which uploads only the touched chunks; index-free: mh_decode of the whole stream).  js: its decodable lookups.
int decode_direct(const Models &md, const Batch &B, size_t i, const std::vector<size_t> &js, const uint64_t *lookups, uint8_t *out,
                  const uint64_t *out_off, std::vector<int32_t> &rst) {
    mh_model *own = nullptr;
    const mh_model *m = md.m;
    if (!m) {
        const uint64_t t0 = md.tab_off[i], t1 = md.tab_off[i + 1];
        const int rc = t1 > t0 ? mh_model_from_table_bits(md.tables + t0, size_t(t1 - t0), &own) : MH_ERR_CORRUPT;
        if (rc != MH_OK) { for (size_t j : js) rst[j] = rc; return MH_OK; }
        m = own;
    }
    std::unique_ptr<mh_model, void (*)(mh_model *)> hold(own, mh_model_free);
    const uint8_t *pl = B.payload + B.pay_off[i];
    const uint64_t nb = B.nbits[i];
    if (B.index) {
        const uint64_t ni = B.sym_off[i + 1] - B.sym_off[i];
        const uint64_t *idx = B.index + mh_batch_index_base(B.sym_off[i], i, B.chunk);
        std::vector<uint64_t> rg(js.size() * 2), oo(js.size() + 1);
        std::vector<int32_t> st(js.size());
        uint64_t cap = 0;
        for (size_t k = 0; k < js.size(); ++k) {
            rg[2 * k] = lookups[3 * js[k] + 1]; rg[2 * k + 1] = lookups[3 * js[k] + 2];
            cap += rg[2 * k + 1] - rg[2 * k];
        }
        std::vector<uint8_t> tmp(static_cast<size_t>(cap) + 1);
        const int rc = decode_ranges_host(m, md.o2, pl, nb, idx, B.chunk, ni, rg.data(), js.size(), tmp.data(), size_t(cap), oo.data(), st.data());
        t_batch_range_upload += mh_last_range_upload_bytes();
        bool any = false;
        for (size_t k = 0; k < js.size(); ++k) any |= st[k] == rc;
        if (rc != MH_OK && !any) {
            if (rc == MH_ERR_HIP || rc == MH_ERR_NO_DEVICE) return rc;
            for (size_t j : js) rst[j] = rc;                        // the stream's own arguments (nbits, index) are bad
            return MH_OK;
        }
        for (size_t k = 0; k < js.size(); ++k) {
            rst[js[k]] = st[k];
            if (st[k] == MH_OK) std::memcpy(out + out_off[js[k]], tmp.data() + oo[k], size_t(oo[k + 1] - oo[k]));
        }
        return MH_OK;
    }
    std::vector<uint8_t> dec;
    size_t got = 0;
    const int rc = mh_decode_to(m, pl, nb, B.prev0, grow_vec, &dec, &got, nullptr, 0, 0);
    t_batch_range_upload += (nb + 7) / 8;
    if (rc == MH_ERR_HIP || rc == MH_ERR_NO_DEVICE) return rc;
    for (size_t j : js) {
        const uint64_t b = lookups[3 * j + 1], e = lookups[3 * j + 2];
        if (rc != MH_OK) rst[j] = rc;
        else if (B.sym_off && got != B.sym_off[i + 1] - B.sym_off[i]) rst[j] = MH_ERR_CORRUPT;
        else if (e > got) rst[j] = MH_ERR_ARG;                  // the stream ends before `end`
        else std::memcpy(out + out_off[j], dec.data() + b, size_t(e - b));
    }
    return MH_OK;
}

// streams g[0..) through one device call: their payloads compacted, their index slices re-based to the compacted sym_off,
// the lookups renumbered.  jl: the decodable lookups of these streams, as (lookup, position of its stream in g).
int decode_group(const Models &md, const Batch &B, const std::vector<size_t> &g, const std::vector<std::pair<size_t, size_t>> &jl,
                 const uint64_t *lookups, uint8_t *out, const uint64_t *out_off, std::vector<int32_t> &rst) {
    const size_t n = g.size(), m = jl.size();
    std::vector<uint64_t> poff(n + 1, 0), nb(n), so(n + 1, 0);
    for (size_t k = 0; k < n; ++k) {
        poff[k + 1] = poff[k] + (B.pay_off[g[k] + 1] - B.pay_off[g[k]]);
        nb[k] = B.nbits[g[k]];
        if (B.sym_off) so[k + 1] = so[k] + (B.sym_off[g[k] + 1] - B.sym_off[g[k]]);
    }
    std::vector<uint64_t> lk(m * 3), at(m);
    uint64_t ocap = 0;
    for (size_t q = 0; q < m; ++q) {
        const size_t j = jl[q].first;
        lk[3 * q] = jl[q].second; lk[3 * q + 1] = lookups[3 * j + 1]; lk[3 * q + 2] = lookups[3 * j + 2];
        at[q] = ocap;
        ocap += lk[3 * q + 2] - lk[3 * q + 1];
    }
    std::vector<uint64_t> idx;
    if (B.index) {
        idx.assign(size_t(mh_batch_index_capacity(so[n], n, B.chunk)), 0);
        for (size_t k = 0; k < n; ++k) {
            const uint64_t cnt = (so[k + 1] - so[k] + B.chunk - 1) / B.chunk;
            const uint64_t to = mh_batch_index_base(so[k], k, B.chunk), from = mh_batch_index_base(B.sym_off[g[k]], g[k], B.chunk);
            if (cnt) std::memcpy(idx.data() + to, B.index + from, size_t(cnt) * 8);
        }
    }
    mh_model_set *s = nullptr;
    if (!md.m) {
        std::vector<uint64_t> toff(n + 1, 0);
        for (size_t k = 0; k < n; ++k) toff[k + 1] = toff[k] + (md.tab_off[g[k] + 1] - md.tab_off[g[k]]);
        std::vector<uint8_t> tabs(static_cast<size_t>(toff[n]) + 1);
        for (size_t k = 0; k < n; ++k)
            if (toff[k + 1] > toff[k]) std::memcpy(tabs.data() + toff[k], md.tables + md.tab_off[g[k]], size_t(toff[k + 1] - toff[k]));
        const int rc = mh_model_set_from_tables(tabs.data(), toff.data(), n, &s);
        if (rc != MH_OK) return rc;
    }
    std::unique_ptr<mh_model_set, void (*)(mh_model_set *)> own(s, mh_model_set_free);
    const hipStream_t st = nullptr;
    const size_t wsb = mh_dev_decode_batch_ranges_workspace(m);
    DevBuf d_pl, d_meta, d_idx, d_lk, d_out, d_st, d_ws;
    HIP_TRY(d_pl.alloc(size_t(poff[n]) + 16));
    HIP_TRY(d_meta.alloc((3 * n + 2) * 8));                        // pay_off | nbits | sym_off
    HIP_TRY(d_idx.alloc(idx.size() * 8));
    HIP_TRY(d_lk.alloc(m * 32));                                   // lookups | out_at
    HIP_TRY(d_out.alloc(size_t(ocap)));
    HIP_TRY(d_st.alloc(m * 4));
    HIP_TRY(d_ws.alloc(wsb));
    {
        std::vector<uint8_t> pl(static_cast<size_t>(poff[n]));
        for (size_t k = 0; k < n; ++k)
            if (poff[k + 1] > poff[k]) std::memcpy(pl.data() + poff[k], B.payload + B.pay_off[g[k]], size_t(poff[k + 1] - poff[k]));
        if (poff[n]) HIP_TRY(stage_h2d(d_pl.p, pl.data(), pl.size(), st));
        HIP_TRY(hipStreamSynchronize(st));                           // (pl is a local staging copy)
    }
    t_batch_range_upload += poff[n];
    uint64_t *d_po = d_meta.as<uint64_t>(), *d_nb = d_po + n + 1, *d_so = d_nb + n;
    HIP_TRY(hipMemcpyAsync(d_po, poff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (n) HIP_TRY(hipMemcpyAsync(d_nb, nb.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_so, so.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (!idx.empty()) HIP_TRY(hipMemcpyAsync(d_idx.p, idx.data(), idx.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_lk.p, lk.data(), m * 24, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_lk.as<uint64_t>() + 3 * m, at.data(), m * 8, hipMemcpyHostToDevice, st));
    const uint64_t *dso = B.sym_off ? d_so : nullptr, *dix = B.index ? d_idx.as<uint64_t>() : nullptr;
    // the shared model's device call, or the set's: the same arguments behind the model
    auto dev = [&](auto call, auto *model) {
        return call(model, d_pl.as<uint8_t>(), d_po, d_nb, n, B.prev0, dso, dix, B.chunk, d_lk.as<uint64_t>(), m, d_out.as<uint8_t>(),
                    d_lk.as<uint64_t>() + 3 * m, ocap, d_st.as<int32_t>(), d_ws.p, wsb, st);
    };
    const int rc = !md.m ? dev(mh_dev_decode_each_ranges, s) : dev(md.o2 ? mh_dev_decode_batch_o2_ranges : mh_dev_decode_batch_ranges, md.m);
    if (rc != MH_OK) return rc;
    std::vector<int32_t> h_st(m);
    std::vector<uint8_t> h_out(static_cast<size_t>(ocap));
    HIP_TRY(hipMemcpyAsync(h_st.data(), d_st.p, m * 4, hipMemcpyDeviceToHost, st));
    if (ocap) HIP_TRY(stage_d2h(h_out.data(), d_out.p, size_t(ocap), st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t q = 0; q < m; ++q) {
        const size_t j = jl[q].first;
        rst[j] = h_st[q];
        if (h_st[q] == MH_OK) std::memcpy(out + out_off[j], h_out.data() + at[q], size_t(lk[3 * q + 2] - lk[3 * q + 1]));
    }
    return MH_OK;
}

int host_ranges(const Models &md, const Batch &B, const uint64_t *lookups, size_t n_lookups, uint8_t *out, size_t out_cap,
                uint64_t *out_off, int32_t *lookup_status) {
    // per-lookup checks on the host: the lookup, the offsets of its stream against the buffers' lengths, its table
    std::vector<int32_t> rst(n_lookups, MH_OK);
    std::unordered_map<uint64_t, int> tab_rc;                       // per-stream table verdict, on first touch
    for (size_t j = 0; j < n_lookups; ++j) {
        const uint64_t i = lookups[3 * j], b = lookups[3 * j + 1], e = lookups[3 * j + 2];
        if (i >= B.n || b > e) { rst[j] = MH_ERR_ARG; continue; }
        const uint64_t p0 = B.pay_off[i], p1 = B.pay_off[i + 1];
        bool bad = p1 < p0 || p1 > B.payload_bytes || B.nbits[i] > (p1 - p0) * 8;
        if (B.sym_off) bad |= B.sym_off[i + 1] < B.sym_off[i] || e > B.sym_off[i + 1] - B.sym_off[i];
        else bad |= e > B.nbits[i];                                  // every code has at least one bit: n_i <= nbits_i
        if (!md.m) bad |= md.tab_off[i + 1] < md.tab_off[i] || md.tab_off[i + 1] > md.tables_bytes;
        if (bad) { rst[j] = MH_ERR_ARG; continue; }
        if (!md.m && b < e) {
            auto t = tab_rc.find(i);
            if (t == tab_rc.end()) t = tab_rc.emplace(i, check_table(md.tables + md.tab_off[i], size_t(md.tab_off[i + 1] - md.tab_off[i]))).first;
            if (t->second != MH_OK) rst[j] = MH_ERR_BADTABLE;
        }
    }
    // outputs packed in lookup order; a refused lookup has length 0, one that does not fit keeps its length
    uint64_t pos = 0;
    for (size_t j = 0; j < n_lookups; ++j) {
        out_off[j] = pos;
        if (rst[j] != MH_OK) continue;
        const uint64_t len = lookups[3 * j + 2] - lookups[3 * j + 1];
        if (pos + len > out_cap) rst[j] = MH_ERR_CAPACITY;
        pos += len;
    }
    out_off[n_lookups] = pos;
    // the touched streams, in stream order, and their decodable lookups
    std::vector<std::pair<uint64_t, size_t>> work;                  // (stream, lookup)
    for (size_t j = 0; j < n_lookups; ++j)
        if (rst[j] == MH_OK && lookups[3 * j + 1] < lookups[3 * j + 2]) work.emplace_back(lookups[3 * j], j);
    if (!work.empty()) {
        if (!have_device()) return MH_ERR_NO_DEVICE;
        if (md.m && md.m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
        std::sort(work.begin(), work.end());
        std::vector<size_t> g, js;
        std::vector<std::pair<size_t, size_t>> jl;
        uint64_t acc = 0;
        for (size_t w = 0; w < work.size();) {
            const size_t i = size_t(work[w].first);
            js.clear();
            uint64_t outb = 0;
            for (; w < work.size() && work[w].first == i; ++w) {
                js.push_back(work[w].second);
                outb += lookups[3 * work[w].second + 2] - lookups[3 * work[w].second + 1];
            }
            const uint64_t pb = B.pay_off[i + 1] - B.pay_off[i];
            if (pb > MH_EACH_DIRECT_BYTES || (!B.index && B.nbits[i] > MH_BATCH_WALK_MAX_BITS)) {
                const int rc = decode_direct(md, B, i, js, lookups, out, out_off, rst);
                if (rc != MH_OK) return rc;
                continue;
            }
            // device footprint: payload, output, index slice, and a set's slots (at most one per 10 table bits, 256 per stream)
            uint64_t f = pb + outb + 64 + (B.index ? (B.sym_off[i + 1] - B.sym_off[i]) / B.chunk * 8 + 8 : 0);
            if (!md.m) f += mhe::STREAM_BYTES + std::min<uint64_t>((md.tab_off[i + 1] - md.tab_off[i]) * 8 / 20 + 1, 256) * mhe::SLOT_BYTES;
            if (!g.empty() && acc + f > MH_EACH_GROUP_BYTES) {
                const int rc = decode_group(md, B, g, jl, lookups, out, out_off, rst);
                if (rc != MH_OK) return rc;
                g.clear(); jl.clear(); acc = 0;
            }
            for (size_t j : js) jl.emplace_back(j, g.size());
            g.push_back(i);
            acc += f;
        }
        if (!g.empty()) {
            const int rc = decode_group(md, B, g, jl, lookups, out, out_off, rst);
            if (rc != MH_OK) return rc;
        }
    }
    int first = MH_OK;
    for (size_t j = 0; j < n_lookups && first == MH_OK; ++j) first = rst[j];
    if (lookup_status) std::copy(rst.begin(), rst.end(), lookup_status);
    return first;
}

// call-level checks of both host forms
int host_args(const Batch &B, const uint64_t *lookups, size_t n_lookups, uint8_t *out, size_t out_cap, const uint64_t *out_off) {
    if ((!B.payload && B.payload_bytes) || !B.pay_off || (!B.nbits && B.n) || (!lookups && n_lookups) || !out_off || (!out && out_cap))
        return MH_ERR_ARG;
    if (B.index && (!B.sym_off || chunk_shift_of(B.chunk) < 0)) return MH_ERR_ARG;
    return MH_OK;
}

}  // namespace

namespace mhq {

int prepare_lookups(const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams, uint32_t prev0,
                    const uint64_t *d_sym_off, const uint64_t *d_index, uint32_t chunk_symbols, const uint64_t *d_lookups, size_t n_lookups,
                    uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap, int32_t *d_lookup_status, void *d_ws, size_t ws_bytes,
                    LookupParams &p) {
    if (!d_pay_off || (n_streams && (!d_payload || !d_nbits)) || !d_ws) return MH_ERR_ARG;
    if (n_lookups && (!d_lookups || !d_out_at || !d_lookup_status)) return MH_ERR_ARG;
    if ((!d_out && out_cap) || !aligned16(d_payload) || !aligned16(d_out) || !aligned16(d_ws)) return MH_ERR_ARG;
    int shift;
    if (!index_args_ok(d_index, chunk_symbols, d_sym_off, shift)) return MH_ERR_ARG;
    if (ws_bytes < range_layout(n_lookups).total) return MH_ERR_CAPACITY;
    p.payload = d_payload; p.pay_off = d_pay_off; p.nbits = d_nbits; p.n_streams = n_streams; p.prev0 = prev0;
    p.sym_off = d_sym_off; p.index = d_index; p.chunk_shift = uint32_t(shift);
    p.walk_max_bits = MH_BATCH_WALK_MAX_BITS;
    p.lookups = d_lookups; p.n = n_lookups;
    p.out = d_out; p.out_at = d_out_at; p.out_cap = out_cap;
    p.status = d_lookup_status;
    return MH_OK;
}

}  // namespace mhq

namespace {

// mh_dev_decode_batch_ranges (o2 = false: an order-0/1 model) and mh_dev_decode_batch_o2_ranges (an order-2 model)
int dev_decode_batch_ranges(const mh_model *m, bool o2, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                            size_t n_streams, uint8_t prev0, const uint64_t *d_sym_off, const uint64_t *d_index, uint32_t chunk_symbols,
                            const uint64_t *d_lookups, size_t n_lookups, uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                            int32_t *d_lookup_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!(o2 ? order2(m) : order01(m))) return MH_ERR_ARG;
    mhq::LookupParams p{};
    const int rc = mhq::prepare_lookups(d_payload, d_pay_off, d_nbits, n_streams, ctx_of_prev0(m, prev0), d_sym_off, d_index, chunk_symbols,
                                        d_lookups, n_lookups, d_out, d_out_at, out_cap, d_lookup_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    fill_dec_tables(m, p.tab);
    HIP_TRY(mhq::launch_lookups(p, o2 ? mhb::Model::Shared2 : mhb::Model::Shared, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

}  // namespace

extern "C" {

uint64_t mh_last_batch_range_upload_bytes(void) { return t_batch_range_upload; }

size_t mh_dev_decode_batch_ranges_workspace(size_t n_lookups) { return mhq::range_layout(n_lookups).total; }
size_t mh_dev_decode_batch_o2_ranges_workspace(size_t n_lookups) { return mhq::range_layout(n_lookups).total; }

int mh_dev_decode_batch_ranges(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                               size_t n_streams, uint8_t prev0, const uint64_t *d_sym_off, const uint64_t *d_index, uint32_t chunk_symbols,
                               const uint64_t *d_lookups, size_t n_lookups, uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                               int32_t *d_lookup_status, void *d_ws, size_t ws_bytes, void *stream) {
    return dev_decode_batch_ranges(m, false, d_payload, d_pay_off, d_nbits, n_streams, prev0, d_sym_off, d_index, chunk_symbols, d_lookups,
                                   n_lookups, d_out, d_out_at, out_cap, d_lookup_status, d_ws, ws_bytes, stream);
}

int mh_dev_decode_batch_o2_ranges(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                                  size_t n_streams, uint8_t prev0, const uint64_t *d_sym_off, const uint64_t *d_index, uint32_t chunk_symbols,
                                  const uint64_t *d_lookups, size_t n_lookups, uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                                  int32_t *d_lookup_status, void *d_ws, size_t ws_bytes, void *stream) {
    return dev_decode_batch_ranges(m, true, d_payload, d_pay_off, d_nbits, n_streams, prev0, d_sym_off, d_index, chunk_symbols, d_lookups,
                                   n_lookups, d_out, d_out_at, out_cap, d_lookup_status, d_ws, ws_bytes, stream);
}

int mh_dev_decode_each_ranges(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                              size_t n_streams, uint8_t prev0, const uint64_t *d_sym_off, const uint64_t *d_index, uint32_t chunk_symbols,
                              const uint64_t *d_lookups, size_t n_lookups, uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                              int32_t *d_lookup_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!s || n_streams != s->d.n) return MH_ERR_ARG;
    mhq::LookupParams p{};
    const int rc = mhq::prepare_lookups(d_payload, d_pay_off, d_nbits, n_streams, prev0, d_sym_off, d_index, chunk_symbols, d_lookups,
                                        n_lookups, d_out, d_out_at, out_cap, d_lookup_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    p.set = s->d;
    HIP_TRY(mhq::launch_lookups(p, mhb::Model::Set, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int mh_decode_batch_ranges(const mh_model *m, const uint8_t *payload, uint64_t payload_bytes, const uint64_t *pay_off, const uint64_t *nbits,
                           size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                           const uint64_t *lookups, size_t n_lookups, uint8_t *out, size_t out_cap, uint64_t *out_off, int32_t *lookup_status) {
    return decode_batch_ranges_host(m, false, payload, payload_bytes, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols,
                                    lookups, n_lookups, out, out_cap, out_off, lookup_status);
}

int mh_decode_batch_o2_ranges(const mh_model *m, const uint8_t *payload, uint64_t payload_bytes, const uint64_t *pay_off, const uint64_t *nbits,
                              size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                              const uint64_t *lookups, size_t n_lookups, uint8_t *out, size_t out_cap, uint64_t *out_off, int32_t *lookup_status) {
    return decode_batch_ranges_host(m, true, payload, payload_bytes, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols,
                                    lookups, n_lookups, out, out_cap, out_off, lookup_status);
}

int mh_decompress_each_ranges(const uint8_t *tables, uint64_t tables_bytes, const uint64_t *tab_off, const uint8_t *payload,
                              uint64_t payload_bytes, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams, uint8_t prev0,
                              const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, const uint64_t *lookups,
                              size_t n_lookups, uint8_t *out, size_t out_cap, uint64_t *out_off, int32_t *lookup_status) {
    t_batch_range_upload = 0;
    const Batch B{payload, payload_bytes, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols};
    if (!tab_off || (!tables && tables_bytes)) return MH_ERR_ARG;
    const int rc = host_args(B, lookups, n_lookups, out, out_cap, out_off);
    if (rc != MH_OK) return rc;
    Models md;
    md.tables = tables; md.tables_bytes = tables_bytes; md.tab_off = tab_off;
    return host_ranges(md, B, lookups, n_lookups, out, out_cap, out_off, lookup_status);
}

}  // extern "C"

namespace mhapi {

int decode_batch_ranges_host(const mh_model *m, bool o2, const uint8_t *payload, uint64_t payload_bytes, const uint64_t *pay_off,
                             const uint64_t *nbits, size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index,
                             uint32_t chunk_symbols, const uint64_t *lookups, size_t n_lookups, uint8_t *out, size_t out_cap,
                             uint64_t *out_off, int32_t *lookup_status) {
    t_batch_range_upload = 0;
    const Batch B{payload, payload_bytes, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols};
    if (!(o2 ? order2(m) : order01(m))) return MH_ERR_ARG;
    const int rc = host_args(B, lookups, n_lookups, out, out_cap, out_off);
    if (rc != MH_OK) return rc;
    Models md;
    md.m = m;
    md.o2 = o2;
    return host_ranges(md, B, lookups, n_lookups, out, out_cap, out_off, lookup_status);
}

}  // namespace mhapi
