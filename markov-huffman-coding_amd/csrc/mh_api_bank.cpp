// mh_api_bank.cpp — the bank calls of the C ABI (include/mh.h, "BANKS OF SHARED MODELS"): selection (kernels: mh_bank.hip), the set
// view over a bank, training (sort and gather in mh_bank.hip; histograms, trees and the set itself through the existing batch,
// model and set builders, so the reference's tie-breaking keeps one copy) and the host-buffer forms.
#include "mh_api_reader.hpp"
#include "mh_bank.h"

#include <memory>
#include <numeric>

using namespace mhapi;

namespace {

size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

bool bank_ok(const mh_model_set *b) { return b && b->d.n >= 1 && b->d.n <= MH_BANK_MAX; }

using SetPtr = std::unique_ptr<mh_model_set, void (*)(mh_model_set *)>;

// training workspace: offsets-check status block | select workspace | batch histogram workspace | counts | gathered bytes |
// sorted offsets + scan sums | group offsets | summary | perm | block counts | groups A, B | nbits | remap | changed
struct TrainWs {
    size_t off_sel, off_hist, off_counts, off_gdata, off_goff, off_sums, off_coff, off_summary, off_perm, off_bcnt, off_a, off_b, off_nbits,
        off_remap, off_changed, total;
};
TrainWs train_ws(uint64_t n, uint64_t total, uint64_t k) {
    TrainWs w;
    size_t at = 256;
    auto take = [&](size_t bytes) { const size_t o = at; at += al256(bytes); return o; };
    w.off_sel = take(mhbank::sel_layout(k, n).total);
    w.off_hist = take(mh_dev_histogram_batch_workspace(size_t(total)));
    w.off_counts = take(65536 * 8);
    w.off_gdata = take(size_t(total) + 16 * size_t(k) + 16);
    w.off_goff = take(size_t(n + 1) * 8);
    w.off_sums = take(size_t(mhb::scan_blocks(n + 1) + 1) * 8);
    w.off_coff = take(size_t(n + k) * 8);
    w.off_summary = take(3 * size_t(k + 1) * 8);
    w.off_perm = take(size_t(n) * 4);
    w.off_bcnt = take(size_t((n + mhbank::SORT_BLOCK - 1) / mhbank::SORT_BLOCK) * size_t(k) * 4);
    w.off_a = take(size_t(n) * 4);
    w.off_b = take(size_t(n) * 4);
    w.off_nbits = take(size_t(n) * 8);
    w.off_remap = take(size_t(k) * 4);
    w.off_changed = take(8);
    w.total = at;
    return w;
}

// one model per group of the streams (d_group, k groups): sort and gather, then per group holding a symbol the batch histogram
// of its streams and the model from its counts.  remap[c] = the group's entry in the new bank, MH_BANK_NONE when dropped.
int retrain(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, int order, uint8_t prev0, const uint32_t *d_group, uint32_t k,
            unsigned char *ws, const TrainWs &W, hipStream_t st, mh_model_set **bank, std::vector<uint32_t> &remap) {
    mhbank::GatherBufs g{};
    g.gdata = ws + W.off_gdata;
    g.goff = reinterpret_cast<unsigned long long *>(ws + W.off_goff);
    g.sums = reinterpret_cast<unsigned long long *>(ws + W.off_sums);
    g.coff = reinterpret_cast<unsigned long long *>(ws + W.off_coff);
    g.summary = reinterpret_cast<unsigned long long *>(ws + W.off_summary);
    g.perm = reinterpret_cast<uint32_t *>(ws + W.off_perm);
    g.bcnt = reinterpret_cast<uint32_t *>(ws + W.off_bcnt);
    HIP_TRY(mhbank::launch_gather(d_data, d_in_off, n, d_group, k, g, reinterpret_cast<const int *>(ws) + 1, st));
    std::vector<unsigned long long> sm(3 * size_t(k + 1));
    HIP_TRY(hipMemcpyAsync(sm.data(), g.summary, sm.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    remap.assign(k, mhbank::NONE);
    std::vector<mh_model *> models;
    auto free_models = [&]() { for (mh_model *m : models) mh_model_free(m); };
    uint64_t *counts = reinterpret_cast<uint64_t *>(ws + W.off_counts);
    void *hws = ws + W.off_hist;
    const size_t hbytes = W.off_counts - W.off_hist;
    int rc = MH_OK;
    for (uint32_t c = 0; c < k && rc == MH_OK; ++c) {
        const uint64_t start = sm[c], ns = sm[c + 1] - start, base = sm[k + 1 + c], bytes = sm[2 * (k + 1) + c];
        if (bytes == 0) continue;                                     // a group without a symbol: no entry
        const uint64_t *coff = reinterpret_cast<const uint64_t *>(g.coff + start + c);
        rc = order ? mh_dev_histogram_o1_batch(g.gdata + base, coff, ns, bytes, prev0, counts, hws, hbytes, st)
                   : mh_dev_histogram_o0_batch(g.gdata + base, coff, ns, bytes, counts, hws, hbytes, st);
        mh_model *m = nullptr;
        if (rc == MH_OK) rc = mh_dev_model_from_counts(counts, order, st, &m);
        if (rc == MH_OK) rc = mh_dev_status(hws, st);
        if (m) { remap[c] = uint32_t(models.size()); models.push_back(m); }
    }
    if (rc == MH_OK && models.empty()) rc = MH_ERR_ARG;             // (total > 0: some group holds a symbol)
    if (rc == MH_OK) rc = mh_model_set_from_models(models.data(), models.size(), bank);
    free_models();
    if (rc != MH_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ws + W.off_remap, remap.data(), size_t(k) * 4, hipMemcpyHostToDevice, st));
    return MH_OK;
}

// a bank of one empty model of this order (a batch without symbols)
int empty_bank(int order, mh_model_set **bank) {
    std::vector<uint64_t> zero(order ? 65536 : 256, 0);
    mh_model *m = nullptr;
    int rc = mh_model_from_counts(zero.data(), order, &m);
    if (rc != MH_OK) return rc;
    rc = mh_model_set_from_models(&m, 1, bank);
    mh_model_free(m);
    return rc;
}

}  // namespace

extern "C" {

size_t mh_dev_bank_select_workspace(size_t n_entries, size_t n_streams, size_t total) {
    (void)total;
    return mhbank::sel_layout(n_entries, n_streams).total;
}

int mh_dev_bank_select(const mh_model_set *bank, const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint8_t prev0,
                       uint32_t *d_choice, uint64_t *d_nbits, void *d_ws, size_t ws_bytes, void *stream) {
    if (!bank_ok(bank) || (!d_data && total) || !d_in_off || (!d_choice && n_streams) || !d_ws || !aligned16(d_ws)) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_bank_select_workspace(bank->d.n, n_streams, total)) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    HIP_TRY(mhbank::launch_select(bank->d, d_data, d_in_off, n_streams, total, prev0, d_choice, reinterpret_cast<unsigned long long *>(d_nbits),
                                  d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int mh_dev_model_set_pick(const mh_model_set *bank, const uint32_t *d_choice, size_t n_streams, void *stream, mh_model_set **out) {
    if (!out) return MH_ERR_ARG;
    *out = nullptr;
    if (!bank_ok(bank) || (!d_choice && n_streams)) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = n_streams;
    const size_t o_max = al256(n), o_ctx = o_max + al256(4 * n), o_st = o_ctx + al256(1024 * n), total = o_st + 256;
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, total));
    std::unique_ptr<mh_model_set> v(new (std::nothrow) mh_model_set);
    if (!v) { (void)hipFree(p); return MH_ERR_NOMEM; }
    v->rows.reset(p, [](void *q) { (void)hipFree(q); });
    unsigned char *b = static_cast<unsigned char *>(p);
    v->block = bank->block;
    v->d = bank->d;
    v->d.n = n;
    v->d.type = b;
    v->d.maxlen = reinterpret_cast<uint32_t *>(b + o_max);
    v->d.ctx_slot = reinterpret_cast<uint32_t *>(b + o_ctx);
    v->d.slot_base = nullptr;
    v->d.slot_stream = nullptr;
    v->max_len = bank->max_len;
    v->min_len = bank->min_len;
    v->view = true;
    int *status = reinterpret_cast<int *>(b + o_st);
    int h = 0;
    HIP_TRY(mhbank::launch_pick(bank->d, d_choice, v->d, status, st));
    HIP_TRY(hipMemcpyAsync(&h, status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h) return status_from_device(h);
    *out = v.release();
    return MH_OK;
}

size_t mh_dev_bank_train_workspace(size_t n_streams, size_t total, uint32_t k) {
    if (k > MH_BANK_MAX) k = MH_BANK_MAX;
    return train_ws(n_streams, total, k ? k : 1).total;
}

int mh_dev_bank_train(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, int order, uint8_t prev0, uint32_t k,
                      uint32_t max_iters, uint32_t *d_choice, int *iters_run, void *d_ws, size_t ws_bytes, void *stream, mh_model_set **bank) {
    if (!bank) return MH_ERR_ARG;
    *bank = nullptr;
    if (iters_run) *iters_run = 0;
    if ((!d_data && total) || !d_in_off || (!d_choice && n_streams) || !d_ws || !aligned16(d_ws)) return MH_ERR_ARG;
    if ((order != 0 && order != 1) || k < 1 || k > MH_BANK_MAX || max_iters < 1) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_bank_train_workspace(n_streams, total, k)) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t n = n_streams;
    const TrainWs W = train_ws(n, total, k);
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    void *sel_ws = ws + W.off_sel;
    const size_t sel_bytes = W.off_hist - W.off_sel;
    uint32_t *ga = reinterpret_cast<uint32_t *>(ws + W.off_a), *gb = reinterpret_cast<uint32_t *>(ws + W.off_b);
    uint64_t *nb = reinterpret_cast<uint64_t *>(ws + W.off_nbits);
    auto *changed = reinterpret_cast<unsigned long long *>(ws + W.off_changed);

    // the offsets first: everything after them trusts them
    HIP_TRY(mhbank::launch_check(d_in_off, n, total, ws, st));
    int head = 0;
    HIP_TRY(hipMemcpyAsync(&head, ws, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (head) return status_from_device(head);

    mh_model_set *cur = nullptr;
    if (n == 0 || total == 0) {                                       // nothing to train on: one empty model, every choice 0
        int rc = empty_bank(order, &cur);
        if (rc != MH_OK) return rc;
        if (n) {
            const hipError_t e = hipMemsetAsync(d_choice, 0, size_t(n) * 4, st);
            if (e == hipSuccess) rc = hipStreamSynchronize(st) == hipSuccess ? MH_OK : MH_ERR_HIP;
            else rc = hip_fail(e);
        }
        if (rc != MH_OK) { mh_model_set_free(cur); return rc; }
        *bank = cur;
        return MH_OK;
    }
    SetPtr own(nullptr, mh_model_set_free);
    std::vector<uint32_t> remap;
    auto select = [&](mh_model_set *b, uint32_t *dst) -> int {
        int rc = mh_dev_bank_select(b, d_data, d_in_off, n, total, prev0, dst, nb, sel_ws, sel_bytes, stream);
        if (rc == MH_OK) rc = mh_dev_status(sel_ws, stream);
        return rc;
    };

    // seed: the shared model, the streams sorted by their bits per byte under it, cut into equal-count groups
    HIP_TRY(hipMemsetAsync(ga, 0, size_t(n) * 4, st));
    int rc = retrain(d_data, d_in_off, n, order, prev0, ga, 1, ws, W, st, &cur, remap);
    if (rc != MH_OK) return rc;
    own.reset(cur);
    if ((rc = select(cur, gb)) != MH_OK) return rc;
    std::vector<uint64_t> bits(n), off(n + 1);
    HIP_TRY(hipMemcpyAsync(bits.data(), nb, size_t(n) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(off.data(), d_in_off, size_t(n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint32_t> order_idx(n), groups(n);
    std::iota(order_idx.begin(), order_idx.end(), 0u);
    auto len_of = [&](uint32_t i) -> unsigned __int128 { const uint64_t l = off[i + 1] - off[i]; return l ? l : 1; };   // empty: 0 / 1
    std::stable_sort(order_idx.begin(), order_idx.end(), [&](uint32_t a, uint32_t b) {
        return (unsigned __int128)bits[a] * len_of(b) < (unsigned __int128)bits[b] * len_of(a);
    });
    uint32_t kg = uint32_t(std::min<uint64_t>(k, n));
    for (uint64_t r = 0; r < n; ++r) groups[order_idx[r]] = uint32_t(r * kg / n);
    HIP_TRY(hipMemcpyAsync(ga, groups.data(), size_t(n) * 4, hipMemcpyHostToDevice, st));

    // iterations: retrain on the groups in ga, select into gb, stop when no choice moved
    int it = 0;
    for (uint32_t t = 1; t <= max_iters; ++t) {
        mh_model_set *nbank = nullptr;
        if ((rc = retrain(d_data, d_in_off, n, order, prev0, ga, kg, ws, W, st, &nbank, remap)) != MH_OK) return rc;
        own.reset(nbank);
        if ((rc = select(nbank, gb)) != MH_OK) return rc;
        HIP_TRY(mhbank::launch_changed(ga, gb, reinterpret_cast<const uint32_t *>(ws + W.off_remap), n, changed, st));
        unsigned long long moved = 0;
        HIP_TRY(hipMemcpyAsync(&moved, changed, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        it = int(t);
        std::swap(ga, gb);
        kg = uint32_t(nbank->d.n);
        if (!moved) break;
    }
    HIP_TRY(hipMemcpyAsync(d_choice, ga, size_t(n) * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (iters_run) *iters_run = it;
    *bank = own.release();
    return MH_OK;
}

/* ------------------------------------------------------- host-buffer calls */

int mh_bank_train(const uint8_t *data, const uint64_t *in_off, size_t n_streams, int order, uint8_t prev0, uint32_t k, uint32_t max_iters,
                  uint32_t *choice, int *iters_run, mh_model_set **bank) {
    if (!bank) return MH_ERR_ARG;
    *bank = nullptr;
    if (!in_off || (!choice && n_streams) || (order != 0 && order != 1) || k < 1 || k > MH_BANK_MAX || max_iters < 1) return MH_ERR_ARG;
    if (!offsets_ok(in_off, n_streams)) return MH_ERR_ARG;
    const uint64_t total = in_off[n_streams];
    if (!data && total) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const hipStream_t st = nullptr;
    const size_t n = n_streams, wsb = mh_dev_bank_train_workspace(n, size_t(total), k);
    DevBuf d_data, d_off, d_ch, d_ws;
    HIP_TRY(d_data.alloc(size_t(total)));
    HIP_TRY(d_off.alloc((n + 1) * 8));
    HIP_TRY(d_ch.alloc(n * 4));
    HIP_TRY(d_ws.alloc(wsb));
    if (total) HIP_TRY(stage_h2d(d_data.p, data, size_t(total), st));
    HIP_TRY(hipMemcpy(d_off.p, in_off, (n + 1) * 8, hipMemcpyHostToDevice));
    mh_model_set *b = nullptr;
    const int rc = mh_dev_bank_train(d_data.as<uint8_t>(), d_off.as<uint64_t>(), n, size_t(total), order, prev0, k, max_iters, d_ch.as<uint32_t>(),
                                     iters_run, d_ws.p, wsb, st, &b);
    if (rc != MH_OK) return rc;
    if (n) {
        const hipError_t e = hipMemcpy(choice, d_ch.p, n * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { mh_model_set_free(b); return hip_fail(e); }
    }
    *bank = b;
    return MH_OK;
}

size_t mh_encode_bank_bound(const mh_model_set *bank, const uint32_t *choice, const uint64_t *in_off, size_t n_streams) {
    if (!bank_ok(bank) || !in_off || (!choice && n_streams)) return 0;
    const size_t K = size_t(bank->d.n);
    for (size_t i = 0; i < n_streams; ++i)
        if (choice[i] >= K || in_off[i + 1] < in_off[i]) return 0;
    std::vector<uint32_t> ml(K);
    if (hipMemcpy(ml.data(), bank->d.maxlen, K * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    size_t b = n_streams + 16;
    for (size_t i = 0; i < n_streams; ++i) b += size_t(((in_off[i + 1] - in_off[i]) * uint64_t(ml[choice[i]]) + 7) / 8);
    return b;
}

int mh_encode_bank(const mh_model_set *bank, const uint8_t *data, const uint64_t *in_off, size_t n_streams, uint8_t prev0, const uint32_t *choice,
                   uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *nbits, uint64_t *index, uint32_t chunk_symbols) {
    if (!bank_ok(bank) || !in_off || !out_off || (!nbits && n_streams) || (!choice && n_streams) || (!out_payload && cap)) return MH_ERR_ARG;
    if (index && chunk_shift_of(chunk_symbols) < 0) return MH_ERR_ARG;
    if (!offsets_ok(in_off, n_streams)) return MH_ERR_ARG;
    const uint64_t total = in_off[n_streams];
    if (!data && total) return MH_ERR_ARG;
    for (size_t i = 0; i < n_streams; ++i)
        if (choice[i] >= bank->d.n) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const hipStream_t st = nullptr;
    const size_t n = n_streams;
    const size_t pbound = std::min(cap, mh_encode_bank_bound(bank, choice, in_off, n));
    const size_t nidx = index ? size_t(mh_batch_index_capacity(total, n, chunk_symbols)) : 0;
    const size_t wsb = mh_dev_encode_each_workspace(n, size_t(total));
    DevBuf d_data, d_off, d_ch, d_pay, d_po, d_nb, d_idx, d_ws;
    HIP_TRY(d_data.alloc(size_t(total)));
    HIP_TRY(d_off.alloc((n + 1) * 8));
    HIP_TRY(d_ch.alloc(n * 4));
    HIP_TRY(d_pay.alloc(pbound));
    HIP_TRY(d_po.alloc((n + 1) * 8));
    HIP_TRY(d_nb.alloc(n * 8));
    HIP_TRY(d_idx.alloc(nidx * 8));
    HIP_TRY(d_ws.alloc(wsb));
    if (total) HIP_TRY(stage_h2d(d_data.p, data, size_t(total), st));
    HIP_TRY(hipMemcpy(d_off.p, in_off, (n + 1) * 8, hipMemcpyHostToDevice));
    if (n) HIP_TRY(hipMemcpy(d_ch.p, choice, n * 4, hipMemcpyHostToDevice));
    mh_model_set *v = nullptr;
    int rc = mh_dev_model_set_pick(bank, d_ch.as<uint32_t>(), n, st, &v);
    if (rc != MH_OK) return rc;
    SetPtr own(v, mh_model_set_free);
    rc = mh_dev_encode_each(v, d_data.as<uint8_t>(), d_off.as<uint64_t>(), n, size_t(total), prev0, d_pay.as<uint8_t>(), pbound, d_po.as<uint64_t>(),
                            d_nb.as<uint64_t>(), index ? d_idx.as<uint64_t>() : nullptr, chunk_symbols, d_ws.p, wsb, st);
    if (rc == MH_OK) rc = mh_dev_status(d_ws.p, st);
    if (rc != MH_OK) return rc;
    HIP_TRY(hipMemcpy(out_off, d_po.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    if (out_off[n] > cap) return MH_ERR_CAPACITY;
    if (out_off[n]) HIP_TRY(stage_d2h(out_payload, d_pay.p, size_t(out_off[n]), st));
    if (n) HIP_TRY(hipMemcpy(nbits, d_nb.p, n * 8, hipMemcpyDeviceToHost));
    if (index && nidx) {
        std::vector<uint64_t> idx(nidx);
        HIP_TRY(hipMemcpy(idx.data(), d_idx.p, nidx * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {                              // the slices only: gap entries keep the caller's values
            const uint64_t len = in_off[i + 1] - in_off[i], cnt = (len + chunk_symbols - 1) / chunk_symbols;
            const uint64_t at = mh_batch_index_base(in_off[i], i, chunk_symbols);
            if (cnt) std::memcpy(index + at, idx.data() + at, size_t(cnt) * 8);
        }
    }
    return MH_OK;
}

namespace {
// entry k of a bank as a host-usable model, parsed from the bank's table file (index-free streams over the walk cap)
int bank_entry_model(const mh_model_set *bank, uint32_t k, mh_model **m) {
    const size_t cap = mh_model_set_tables_bound(bank), wsb = mh_dev_model_set_tables_workspace(bank), K = size_t(bank->d.n);
    DevBuf d_t, d_o, d_ws;
    HIP_TRY(d_t.alloc(cap));
    HIP_TRY(d_o.alloc((K + 1) * 8));
    HIP_TRY(d_ws.alloc(wsb));
    int rc = mh_dev_model_set_tables(bank, d_t.as<uint8_t>(), cap, d_o.as<uint64_t>(), d_ws.p, wsb, nullptr);
    if (rc == MH_OK) rc = mh_dev_status(d_ws.p, nullptr);
    if (rc != MH_OK) return rc;
    std::vector<uint64_t> off(K + 1);
    HIP_TRY(hipMemcpy(off.data(), d_o.p, (K + 1) * 8, hipMemcpyDeviceToHost));
    std::vector<uint8_t> t(size_t(off[k + 1] - off[k]));
    if (t.empty()) return MH_ERR_CORRUPT;                             // an empty order-0 model has no code to decode with
    HIP_TRY(hipMemcpy(t.data(), d_t.as<uint8_t>() + off[k], t.size(), hipMemcpyDeviceToHost));
    return mh_model_from_table_bits(t.data(), t.size(), m);
}
}  // namespace

int mh_decode_bank(const mh_model_set *bank, const uint32_t *choice, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                   size_t n_streams, uint8_t prev0, uint8_t *out, size_t out_cap, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                   int32_t *stream_status) {
    if (!bank_ok(bank) || (!choice && n_streams) || !sym_off || (!out && out_cap)) return MH_ERR_ARG;
    CodedBatch a{payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols};
    int rc = host_batch_args(a, index != nullptr);
    if (rc != MH_OK) return rc;
    for (size_t i = 0; i < n_streams; ++i)
        if (choice[i] >= bank->d.n) return MH_ERR_ARG;
    if (a.sym_total > out_cap) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const hipStream_t st = nullptr;
    const size_t n = n_streams;
    std::vector<size_t> long_streams;
    uint64_t dcap = a.sym_total;
    if (!index) {
        const uint64_t minl = uint64_t(bank->min_len > 0 ? bank->min_len : 1);
        uint64_t bound = 0;
        for (size_t i = 0; i < n; ++i) {
            if (nbits[i] > MH_BATCH_WALK_MAX_BITS) long_streams.push_back(i);
            else bound += nbits[i] / minl;
        }
        dcap = std::min<uint64_t>(out_cap, bound);
    }
    const size_t wsb = mh_dev_decode_each_workspace(n);
    DevBatch db;
    DevBuf d_ch, d_out, d_st, d_ws;
    HIP_TRY(d_ch.alloc(n * 4));
    HIP_TRY(d_out.alloc(size_t(dcap)));
    HIP_TRY(d_st.alloc(n * 4));
    HIP_TRY(d_ws.alloc(wsb));
    if (n) HIP_TRY(hipMemcpy(d_ch.p, choice, n * 4, hipMemcpyHostToDevice));
    if ((rc = db.upload(a, st)) != MH_OK) return rc;
    mh_model_set *v = nullptr;
    rc = mh_dev_model_set_pick(bank, d_ch.as<uint32_t>(), n, st, &v);
    if (rc != MH_OK) return rc;
    SetPtr own(v, mh_model_set_free);
    rc = mh_dev_decode_each(v, db.d.payload, db.d.pay_off, db.d.nbits, n, a.pay_total, prev0, d_out.as<uint8_t>(), dcap, db.so.as<uint64_t>(),
                            a.sym_total, db.d.index, chunk_symbols, d_st.as<int32_t>(), d_ws.p, wsb, st);
    if (rc != MH_OK) return rc;
    const int dev_rc = mh_dev_status(d_ws.p, st);
    std::vector<int32_t> sst(n);
    if (n) HIP_TRY(hipMemcpy(sst.data(), d_st.p, n * 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> dso(n + 1);
    HIP_TRY(hipMemcpy(dso.data(), db.so.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    // the streams the device walk refused (over MH_BATCH_WALK_MAX_BITS) decode one by one under their entry's table
    std::vector<std::vector<uint8_t>> extra(long_streams.size());
    std::vector<mh_model *> entry(bank->d.n, nullptr);
    for (size_t j = 0; j < long_streams.size(); ++j) {
        const size_t i = long_streams[j];
        int r = MH_OK;
        if (!entry[choice[i]]) r = bank_entry_model(bank, choice[i], &entry[choice[i]]);
        size_t got = 0;
        if (r == MH_OK) r = mh_decode_to(entry[choice[i]], payload + pay_off[i], nbits[i], prev0, grow_vec, &extra[j], &got, nullptr, 0, 0);
        extra[j].resize(r == MH_OK ? got : 0);
        sst[i] = r;
    }
    for (mh_model *m : entry)
        if (m) mh_model_free(m);
    const int first = first_failure(sst, {}, dev_rc);
    if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
    if (!long_streams.empty()) return splice_alone(dso, d_out.p, long_streams, extra, out, out_cap, sym_off, first, st);
    if (!index) std::copy(dso.begin(), dso.end(), sym_off);
    if (dso[n] && dso[n] <= out_cap) HIP_TRY(stage_d2h(out, d_out.p, size_t(dso[n]), st));
    return first;
}

}  // extern "C"
