// mh_api_find.cpp — the search calls of the C ABI (include/mh.h, "SEARCH IN BATCHES", the search part of "ORDER 2 IN
// SEARCH AND RE-CODING" and "DICTIONARY SEARCH IN BATCHES"): the pattern set (a host object: the Shift-And automaton of
// mh_find.h), the device image of a dictionary (built in mh_dict_host.cpp), the device calls under one shared model of order
// 0/1 or 2 or under a model set (kernels: mh_find.hip) and the host-buffer forms.  Every call is written once over a Matcher.
#include "mh_api_reader.hpp"
#include "mh_find.h"

using namespace mhapi;

namespace {

// what a call searches for: a pattern set or a dictionary
struct Matcher {
    const mh_pattern_set *ps = nullptr;
    const mh_dict *dict = nullptr;
    explicit Matcher(const mh_pattern_set *s) : ps(s) {}
    explicit Matcher(const mh_dict *d) : dict(d) {}
    bool null() const { return !ps && !dict; }
};

// the batch part of the parameters behind the shared checks (mh_api_reader.hpp), and the search's own outputs
int prepare(const Matcher &mt, const CodedBatch &a, uint32_t ctx0, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
            int32_t *d_stream_status, void *d_ws, size_t ws_bytes, mhf::FindParams &p) {
    if (mt.null() || !d_hit_off) return MH_ERR_ARG;
    const mhf::FindLayout L = mhf::find_layout(a.n, work_items_of(a));
    const int rc = dev_batch_params(a, SymOff::UnderIndex, ctx0, d_ws, ws_bytes, L.total, L.off_status, d_stream_status, p.b);
    if (rc != MH_OK) return rc;
    if (mt.ps) { p.first = mt.ps->first; p.last = mt.ps->last; p.max_len = mt.ps->max_len; }
    p.hit_off = reinterpret_cast<unsigned long long *>(d_hit_off);
    p.hits = reinterpret_cast<unsigned long long *>(d_hits);
    p.hit_pattern = d_hits ? d_hit_pattern : nullptr;
    p.hit_cap = d_hits ? hit_cap : 0;
    return MH_OK;
}

int run(const mhf::FindParams &p, const Matcher &mt, mhf::Model model, void *d_ws, void *stream) {
    if (mt.dict) {
        if (!mt.dict->d_image) return MH_ERR_NO_DEVICE;
        HIP_TRY(mhf::launch_find_dict(p, mt.dict->dev, model, d_ws, static_cast<hipStream_t>(stream)));
        return MH_OK;
    }
    mhf::Automaton a;
    std::memcpy(a.mask, mt.ps->mask, sizeof a.mask);
    HIP_TRY(mhf::launch_find(p, a, model, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

// mh_dev_find_batch, mh_dev_find_batch_o2 and their dictionary forms behind their order checks: one shared model, its tables
// as the model's batch decoder takes them
int find_shared(const mh_model *m, mhf::Model model, const Matcher &mt, const CodedBatch &a, uint64_t *d_hit_off, uint64_t *d_hits,
                uint32_t *d_hit_pattern, uint64_t hit_cap, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    mhf::FindParams p{};
    const int rc = prepare(mt, a, ctx_of_prev0(m, a.prev0), d_hit_off, d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    fill_dec_tables(m, p.b);
    return run(p, mt, model, d_ws, stream);
}

// mh_dev_find_each and its dictionary form
int find_each(const mh_model_set *s, const Matcher &mt, const CodedBatch &a, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern,
              uint64_t hit_cap, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!s || a.n != s->d.n) return MH_ERR_ARG;
    mhf::FindParams p{};
    const int rc = prepare(mt, a, a.prev0, d_hit_off, d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, p);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    p.set = s->d;
    return run(p, mt, mhf::Model::Set, d_ws, stream);
}

// the argument checks of the two host forms, in the order of mh_decode_batch
int host_args(const mh_model *m, const Matcher &mt, CodedBatch &a, const uint64_t *hit_off) {
    if (mt.null() || !hit_off) return MH_ERR_ARG;
    const int rc = host_batch_args(a, a.index != nullptr);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    return MH_OK;
}

// One host-form search on the device: search() uploads the batch, runs the device call of the model's order and brings back
// the verdicts and hit_off; records() then brings the records the device kept to wherever the caller wants them.
struct HostSearch {
    DevBatch db;
    DevBuf d_ho, d_hits, d_pat, d_st, d_ws;
    std::vector<int32_t> sst;           // per-stream verdicts
    std::vector<uint64_t> hit_off;      // n + 1, as the device wrote them
    uint64_t cap = 0, nrec = 0;         // records asked for, records kept
    int dev_rc = MH_OK;

    int search(const mh_model *m, const Matcher &mt, const CodedBatch &a, bool want_hits, bool want_pattern, uint64_t hit_cap) {
        const hipStream_t st = nullptr;
        const size_t n = a.n, wsb = mh_dev_find_batch_workspace(n, a.sym_total, a.index ? a.chunk_symbols : 0);
        cap = want_hits ? hit_cap : 0;
        HIP_TRY(d_ho.alloc((n + 1) * 8));
        HIP_TRY(d_hits.alloc(size_t(cap) * 24));
        HIP_TRY(d_pat.alloc(size_t(cap) * 4));
        HIP_TRY(d_st.alloc(n * 4));
        HIP_TRY(d_ws.alloc(wsb));
        int rc = db.upload(a, st);
        if (rc != MH_OK) return rc;
        rc = find_shared(m, order2(m) ? mhf::Model::Shared2 : mhf::Model::Shared, mt, db.d, d_ho.as<uint64_t>(), want_hits ? d_hits.as<uint64_t>() : nullptr,
                         want_pattern ? d_pat.as<uint32_t>() : nullptr, cap, d_st.as<int32_t>(), d_ws.p, wsb, st);
        if (rc != MH_OK) return rc;
        dev_rc = mh_dev_status(d_ws.p, st);
        sst.resize(n);
        hit_off.resize(n + 1);
        if (n) HIP_TRY(hipMemcpy(sst.data(), d_st.p, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hit_off.data(), d_ho.p, (n + 1) * 8, hipMemcpyDeviceToHost));
        nrec = std::min<uint64_t>(hit_off[n], cap);
        return MH_OK;
    }

    int records(uint64_t *hits, uint32_t *hit_pattern) {
        if (!nrec) return MH_OK;
        HIP_TRY(hipMemcpy(hits, d_hits.p, size_t(nrec) * 24, hipMemcpyDeviceToHost));
        if (hit_pattern) HIP_TRY(hipMemcpy(hit_pattern, d_pat.p, size_t(nrec) * 4, hipMemcpyDeviceToHost));
        return MH_OK;
    }

    // the call's result (idx_st: what indexing the batch first found); the device's MH_ERR_CAPACITY: the hits do not fit
    int finish(const std::vector<int32_t> &idx_st, int32_t *stream_status) {
        const int first = first_failure(sst, idx_st, dev_rc);
        if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
        return first;
    }
};

// the hits of one decoded message under the host-side automaton, in (end, pattern) order
struct Hit { uint64_t begin, end; uint32_t pattern; };
void host_find(const Matcher &mt, const uint8_t *data, size_t n, std::vector<Hit> &out) {
    if (mt.dict) {
        uint64_t total = 0;
        mh_dict_find_bytes(mt.dict, data, n, nullptr, nullptr, 0, &total);
        std::vector<uint64_t> at(static_cast<size_t>(total) * 2);
        std::vector<uint32_t> pat(static_cast<size_t>(total));
        mh_dict_find_bytes(mt.dict, data, n, at.data(), pat.data(), total, &total);
        for (size_t r = 0; r < total; ++r) out.push_back(Hit{at[2 * r], at[2 * r + 1], pat[r]});
        return;
    }
    const mh_pattern_set *ps = mt.ps;
    uint64_t D = 0;
    for (size_t k = 0; k < n; ++k) {
        D = ((D << 1) | ps->first) & ps->mask[data[k]];
        for (uint64_t h = D & ps->last; h; h &= h - 1) {
            const uint32_t b = uint32_t(__builtin_ctzll(h));
            const uint32_t j = uint32_t(__builtin_popcountll(ps->last & ((1ull << b) - 1ull)));
            const uint32_t lo = 63u - uint32_t(__builtin_clzll(ps->first & ((2ull << b) - 1ull)));
            out.push_back(Hit{k + 1 - (b - lo + 1u), k + 1, j});
        }
    }
}

// mh_find_batch and mh_find_dict_batch
int find_batch_host(const mh_model *m, const Matcher &mt, CodedBatch a, uint64_t *hit_off, uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap,
                    int32_t *stream_status) {
    if (!order01(m)) return MH_ERR_ARG;
    int rc = host_args(m, mt, a, hit_off);
    if (rc != MH_OK) return rc;
    // index-free with a stream over the walk cap: index the batch first, then search it as an indexed batch; a stream the
    // indexing fails has no symbols, so no hits
    std::vector<uint64_t> own_so, own_idx;
    std::vector<int32_t> idx_st;
    if (over_walk_cap(a)) {
        own_so.assign(a.n + 1, 0);
        if ((rc = index_first(m, a, false, own_so.data(), own_idx, idx_st)) != MH_OK) return rc;
    }
    HostSearch hs;
    rc = hs.search(m, mt, a, hits != nullptr, hit_pattern != nullptr, hit_cap);
    if (rc != MH_OK) return rc;
    std::copy(hs.hit_off.begin(), hs.hit_off.end(), hit_off);
    if ((rc = hs.records(hits, hit_pattern)) != MH_OK) return rc;
    return hs.finish(idx_st, stream_status);
}

// mh_find_batch_o2 and mh_find_dict_batch_o2
int find_batch_o2_host(const mh_model *m, const Matcher &mt, CodedBatch a, uint64_t *hit_off, uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap,
                       int32_t *stream_status) {
    if (!order2(m)) return MH_ERR_ARG;
    int rc = host_args(m, mt, a, hit_off);
    if (rc != MH_OK) return rc;
    // index-free streams over the walk cap: the device call refuses them; each is decoded alone and searched by the
    // host-side automaton, its records spliced into place in stream order
    const uint8_t *payload = a.payload;
    const uint64_t *pay_off = a.pay_off, *nbits = a.nbits;
    const size_t n_streams = a.n;
    const uint8_t prev0 = a.prev0;
    std::vector<size_t> long_streams;
    if (!a.index)
        for (size_t i = 0; i < n_streams; ++i)
            if (nbits[i] > MH_BATCH_WALK_MAX_BITS) long_streams.push_back(i);
    HostSearch hs;
    rc = hs.search(m, mt, a, hits != nullptr, hit_pattern != nullptr, hit_cap);
    if (rc != MH_OK) return rc;
    if (long_streams.empty()) {
        std::copy(hs.hit_off.begin(), hs.hit_off.end(), hit_off);
        if ((rc = hs.records(hits, hit_pattern)) != MH_OK) return rc;
        return hs.finish({}, stream_status);
    }
    const uint64_t cap = hs.cap;
    const std::vector<uint64_t> &dho = hs.hit_off;
    std::vector<uint64_t> dh(static_cast<size_t>(hs.nrec) * 3);
    std::vector<uint32_t> dp(static_cast<size_t>(hs.nrec));
    if ((rc = hs.records(dh.data(), hit_pattern ? dp.data() : nullptr)) != MH_OK) return rc;
    uint64_t r = 0;
    size_t k = 0;
    std::vector<uint8_t> bytes;
    std::vector<Hit> found;
    for (size_t i = 0; i < n_streams; ++i) {
        hit_off[i] = r;
        if (k < long_streams.size() && long_streams[k] == i) {
            ++k;
            found.clear();
            hs.sst[i] = decode_alone(m, payload + pay_off[i], nbits[i], prev0, bytes);
            if (hs.sst[i] == MH_OK) host_find(mt, bytes.data(), bytes.size(), found);
            for (const Hit &h : found) {
                if (r < cap) {
                    hits[3 * r] = i; hits[3 * r + 1] = h.begin; hits[3 * r + 2] = h.end;
                    if (hit_pattern) hit_pattern[r] = h.pattern;
                }
                ++r;
            }
            continue;
        }
        for (uint64_t q = dho[i]; q < dho[i + 1]; ++q, ++r) {
            if (r >= cap) continue;                             // (q <= r: the device kept this record)
            hits[3 * r] = dh[3 * q]; hits[3 * r + 1] = dh[3 * q + 1]; hits[3 * r + 2] = dh[3 * q + 2];
            if (hit_pattern) hit_pattern[r] = dp[q];
        }
    }
    hit_off[n_streams] = r;
    hs.dev_rc = hits && r > cap ? MH_ERR_CAPACITY : MH_OK;
    return hs.finish({}, stream_status);
}

// the device image of a dictionary on the current device: mh_dict_create calls this through mhd::g_upload
int dict_upload(mh_dict *d) {
    if (!have_device()) return MH_OK;
    const mhd::DictImage L = mhd::dict_image(d->states, d->ncls, d->out_pat.size());
    std::vector<uint8_t> img(L.total, 0);
    std::memcpy(img.data(), d->cls, 256);
    std::memcpy(img.data() + L.off_trans, d->trans.data(), d->trans.size() * 2);
    std::memcpy(img.data() + L.off_out_off, d->out_off.data(), d->out_off.size() * 4);
    if (!d->out_pat.empty()) {
        std::memcpy(img.data() + L.off_out_pat, d->out_pat.data(), d->out_pat.size() * 4);
        std::memcpy(img.data() + L.off_out_len, d->out_len.data(), d->out_len.size());
    }
    std::memcpy(img.data() + L.off_depth, d->depth.data(), d->depth.size());
    HIP_TRY(hipGetDevice(&d->device));
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, L.total));
    d->d_image = p;                                              // (mh_dict_free releases it when the copy fails)
    HIP_TRY(hipMemcpy(p, img.data(), L.total, hipMemcpyHostToDevice));
    const uint8_t *b = static_cast<const uint8_t *>(p);
    d->dev = mhd::DictDev{b, reinterpret_cast<const uint16_t *>(b + L.off_trans), reinterpret_cast<const uint32_t *>(b + L.off_out_off),
                          reinterpret_cast<const uint32_t *>(b + L.off_out_pat), b + L.off_depth, b + L.off_out_len, d->ncls, d->states,
                          d->max_len};
    return MH_OK;
}
void dict_release(mh_dict *d) {
    (void)hipFree(d->d_image);
    d->d_image = nullptr;
}
const bool g_dict_hooks = (mhd::g_upload = dict_upload, mhd::g_release = dict_release, true);

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
    const uint64_t W = chunk_shift_of(chunk_symbols) >= 0 ? mhb::work_items(n_streams, sym_total, chunk_symbols) : 0;
    return mhf::find_layout(n_streams, W).total;
}

int mh_dev_find_batch(const mh_model *m, const mh_pattern_set *ps, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                      size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                      uint32_t chunk_symbols, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                      int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order01(m)) return MH_ERR_ARG;
    return find_shared(m, mhf::Model::Shared, Matcher(ps), {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                       d_hit_off, d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, stream);
}

size_t mh_dev_find_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    return mh_dev_find_batch_workspace(n_streams, sym_total, chunk_symbols);
}

int mh_dev_find_batch_o2(const mh_model *m, const mh_pattern_set *ps, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                         size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                         const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern,
                         uint64_t hit_cap, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order2(m)) return MH_ERR_ARG;
    return find_shared(m, mhf::Model::Shared2, Matcher(ps), {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                       d_hit_off, d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_find_each(const mh_model_set *s, const mh_pattern_set *ps, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                     size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                     uint32_t chunk_symbols, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                     int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    return find_each(s, Matcher(ps), {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                     d_hit_off, d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_find_batch(const mh_model *m, const mh_pattern_set *ps, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                  size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint64_t *hit_off,
                  uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap, int32_t *stream_status) {
    return find_batch_host(m, Matcher(ps), {payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols}, hit_off, hits,
                           hit_pattern, hit_cap, stream_status);
}

int mh_find_batch_o2(const mh_model *m, const mh_pattern_set *ps, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                     size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint64_t *hit_off,
                     uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap, int32_t *stream_status) {
    return find_batch_o2_host(m, Matcher(ps), {payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols}, hit_off, hits,
                           hit_pattern, hit_cap, stream_status);
}

// ---- dictionary search: the same calls with the DFA of an mh_dict as the matcher

size_t mh_dev_find_dict_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    return mh_dev_find_batch_workspace(n_streams, sym_total, chunk_symbols);
}

int mh_dev_find_dict_batch(const mh_model *m, const mh_dict *d, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                           size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                           const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern,
                           uint64_t hit_cap, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order01(m)) return MH_ERR_ARG;
    return find_shared(m, mhf::Model::Shared, Matcher(d), {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                       d_hit_off, d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_find_dict_batch_o2(const mh_model *m, const mh_dict *d, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                              size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                              const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern,
                              uint64_t hit_cap, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order2(m)) return MH_ERR_ARG;
    return find_shared(m, mhf::Model::Shared2, Matcher(d), {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                       d_hit_off, d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_find_dict_each(const mh_model_set *s, const mh_dict *d, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                          size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                          const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern,
                          uint64_t hit_cap, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    return find_each(s, Matcher(d), {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                     d_hit_off, d_hits, d_hit_pattern, hit_cap, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_find_dict_batch(const mh_model *m, const mh_dict *d, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                       size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint64_t *hit_off,
                       uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap, int32_t *stream_status) {
    return find_batch_host(m, Matcher(d), {payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols}, hit_off, hits,
                           hit_pattern, hit_cap, stream_status);
}

int mh_find_dict_batch_o2(const mh_model *m, const mh_dict *d, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                          size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                          uint64_t *hit_off, uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap, int32_t *stream_status) {
    return find_batch_o2_host(m, Matcher(d), {payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols}, hit_off, hits,
                           hit_pattern, hit_cap, stream_status);
}

}  // extern "C"
