// mh_api_each.cpp — the per-stream-model calls of the C ABI (include/mh.h, "BATCHES OF STREAMS, ONE MODEL EACH"): model
// sets trained on the device or built from host models and table files, their table files, encode and decode (kernels:
// mh_each.hip), and the host-buffer forms that group a batch by device footprint.
#include "mh_api_reader.hpp"
#include "mh_each.h"

#include <memory>

using namespace mhapi;

namespace {

size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// one device block for the whole set (mh_each.h, SetDev)
hipError_t set_alloc(mh_model_set *s, uint64_t n, uint64_t nslots) {
    const size_t sizes[] = {n, 4 * n, 1024 * n, 8 * (n + 1), 4 * nslots, nslots, 2 * nslots, 256 * nslots, 2048 * nslots, 512 * nslots, 1024 * nslots};
    size_t off[11], total = 0;
    for (int k = 0; k < 11; ++k) { off[k] = total; total += al256(sizes[k]); }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, total ? total : 256);
    if (e != hipSuccess) return e;
    s->block.reset(p, [](void *q) { (void)hipFree(q); });
    unsigned char *b = static_cast<unsigned char *>(p);
    s->d.n = n; s->d.nslots = nslots;
    s->d.type = b + off[0];
    s->d.maxlen = reinterpret_cast<uint32_t *>(b + off[1]);
    s->d.ctx_slot = reinterpret_cast<uint32_t *>(b + off[2]);
    s->d.slot_base = reinterpret_cast<unsigned long long *>(b + off[3]);
    s->d.slot_stream = reinterpret_cast<uint32_t *>(b + off[4]);
    s->d.slot_ctx = b + off[5];
    s->d.slot_leaves = reinterpret_cast<uint16_t *>(b + off[6]);
    s->d.len8 = b + off[7];
    s->d.code64 = reinterpret_cast<unsigned long long *>(b + off[8]);
    s->d.prim = reinterpret_cast<uint16_t *>(b + off[9]);
    s->d.tree = reinterpret_cast<uint32_t *>(b + off[10]);
    return hipSuccess;
}

// Host images of a set, one context at a time (models from host trees or table files)
struct HostSet {
    std::vector<uint8_t> type;
    std::vector<uint32_t> maxlen, ctx_slot, slot_stream;
    std::vector<unsigned long long> slot_base;
    std::vector<uint8_t> slot_ctx, len8;
    std::vector<uint16_t> slot_leaves, prim;
    std::vector<unsigned long long> code64;
    std::vector<uint32_t> tree;
    int max_len = 0, min_len = 0;
    explicit HostSet(size_t n) : type(n), maxlen(n), ctx_slot(n * 256, mhe::NO_SLOT), slot_base(n + 1) {}

    // context c of stream i: codes, first level and walk tree in the layout of mh_each.h (ids: root 0, the other inner
    // nodes in node order, as each_pack_kernel numbers them)
    int add(size_t i, uint32_t c, const mh::ContextCoder &cc) {
        const int root = cc.root();
        if (root < 0) return MH_OK;
        if (cc.node(root).leaf) return MH_ERR_BADTABLE;              // a tree without a code
        if (cc.max_len() > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
        std::vector<int> seen, stack{root};
        while (!stack.empty()) {                                      // the reachable nodes (at most 513)
            const int x = stack.back(); stack.pop_back();
            seen.push_back(x);
            if (!cc.node(x).leaf) { stack.push_back(cc.node(x).child[0]); stack.push_back(cc.node(x).child[1]); }
        }
        std::sort(seen.begin(), seen.end());
        std::vector<int> nid(seen.empty() ? 1 : size_t(seen.back()) + 1, -1);
        int next = 1, leaves = 0;
        for (int x : seen) {
            if (cc.node(x).leaf) ++leaves;
            else nid[x] = x == root ? 0 : next++;
        }
        if (next > 256) return MH_ERR_BADTABLE;
        const uint32_t slot = uint32_t(slot_stream.size());
        ctx_slot[i * 256 + c] = slot;
        slot_stream.push_back(uint32_t(i));
        slot_ctx.push_back(uint8_t(c));
        slot_leaves.push_back(uint16_t(leaves));
        auto enc = [&](int ch) -> uint32_t { return cc.node(ch).leaf ? (mh::TREE_LEAF | cc.node(ch).sym) : uint32_t(nid[ch]); };
        std::vector<uint32_t> tr(256, 0);
        for (int x : seen)
            if (!cc.node(x).leaf) tr[size_t(nid[x])] = (enc(cc.node(x).child[1]) << 16) | enc(cc.node(x).child[0]);
        tree.insert(tree.end(), tr.begin(), tr.end());
        for (uint32_t w = 0; w < 256; ++w) {
            int x = root, depth = 0;
            while (depth < 8 && !cc.node(x).leaf) { x = cc.node(x).child[(w >> (7 - depth)) & 1u]; ++depth; }
            prim.push_back(cc.node(x).leaf ? uint16_t(mh::DEC16_LEAF | (depth << 8) | cc.node(x).sym) : uint16_t(nid[x]));
        }
        for (int sym = 0; sym < 256; ++sym) {
            const mh::Code &k = cc.code(sym);
            len8.push_back(uint8_t(k.len));
            code64.push_back(k.right_aligned());
            if (k.len && (min_len == 0 || k.len < min_len)) min_len = k.len;
        }
        maxlen[i] = std::max<uint32_t>(maxlen[i], uint32_t(cc.max_len()));
        max_len = std::max(max_len, cc.max_len());
        return MH_OK;
    }
    int add_model(size_t i, const mh::Model &m) {
        type[i] = uint8_t(m.type);
        slot_base[i] = slot_stream.size();
        const int nctx = m.type ? 256 : 1;
        for (int c = 0; c < nctx; ++c) {
            const int rc = add(i, uint32_t(c), m.ctx[size_t(c)]);
            if (rc != MH_OK) return rc;
        }
        slot_base[i + 1] = slot_stream.size();
        return MH_OK;
    }
    // a table file straight into the images (src/markov_huffman.cpp:15-25, the same reading as mh::Model::load_table
    // without a 256-context model per stream); a 0-byte table is the empty order-0 model
    int add_table(size_t i, const uint8_t *t, size_t nb, mh::ContextCoder &cc) {
        slot_base[i] = slot_stream.size();
        slot_base[i + 1] = slot_stream.size();
        if (nb == 0) { type[i] = 0; return MH_OK; }
        mh::BitReader in(t, nb);
        if (!((t[0] >> 7) & 1)) {
            type[i] = 0;
            if (!cc.load(in)) return MH_ERR_BADTABLE;
            const int rc = add(i, 0, cc);
            slot_base[i + 1] = slot_stream.size();
            return rc;
        }
        type[i] = 1;
        in.bit();
        for (uint32_t c = 0; c < 256; ++c) {
            if (in.bit()) {
                if (!cc.load(in)) return MH_ERR_BADTABLE;
                const int rc = add(i, c, cc);
                if (rc != MH_OK) return rc;
            }
            if (in.failed()) return MH_ERR_BADTABLE;
        }
        slot_base[i + 1] = slot_stream.size();
        return MH_OK;
    }
    int upload(mh_model_set **out) {
        if (!have_device()) return MH_ERR_NO_DEVICE;
        mh_model_set *s = new (std::nothrow) mh_model_set;
        if (!s) return MH_ERR_NOMEM;
        const size_t n = type.size(), S = slot_stream.size();
        hipError_t e = set_alloc(s, n, S);
        auto up = [&](void *dst, const void *src, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
        };
        if (e == hipSuccess) {
            up(s->d.type, type.data(), n); up(s->d.maxlen, maxlen.data(), 4 * n); up(s->d.ctx_slot, ctx_slot.data(), 4 * ctx_slot.size());
            up(s->d.slot_base, slot_base.data(), 8 * (n + 1)); up(s->d.slot_stream, slot_stream.data(), 4 * S); up(s->d.slot_ctx, slot_ctx.data(), S);
            up(s->d.slot_leaves, slot_leaves.data(), 2 * S); up(s->d.len8, len8.data(), len8.size()); up(s->d.code64, code64.data(), 8 * code64.size());
            up(s->d.prim, prim.data(), 2 * prim.size()); up(s->d.tree, tree.data(), 4 * tree.size());
        }
        if (e != hipSuccess) { delete s; return hip_fail(e); }
        s->max_len = max_len; s->min_len = min_len;
        *out = s;
        return MH_OK;
    }
};

}  // namespace

// a table file parsed as mh_model_set_from_tables would parse it, without building anything on the device
int mhapi::check_table(const uint8_t *t, size_t nb) {
    HostSet h(1);
    mh::ContextCoder cc;
    return h.add_table(0, t, nb, cc);
}

namespace {

uint64_t stream_pay_bound(uint64_t len) {             // a context of k >= 2 leaves has codes of at most min(64, k - 1) bits
    const uint64_t l = len > 1 ? std::min<uint64_t>(64, len - 1) : 1;
    return (len * l + 7) / 8;
}

size_t group_budget() {
    const char *e = getenv("MH_EACH_GROUP_BYTES");
    const unsigned long long v = e ? strtoull(e, nullptr, 10) : 0;
    return v ? size_t(v) : size_t(MH_EACH_GROUP_BYTES);
}

}  // namespace

extern "C" {

size_t mh_dev_model_set_train_workspace(size_t n_streams) { return mhe::train_layout(n_streams).total; }

int mh_dev_model_set_train(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, int order, uint8_t prev0,
                           void *d_ws, size_t ws_bytes, void *stream, mh_model_set **out) {
    if (!out) return MH_ERR_ARG;
    *out = nullptr;
    if ((!d_data && total) || !d_in_off || !d_ws || !aligned16(d_ws) || (order != 0 && order != 1)) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_model_set_train_workspace(n_streams)) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const mhe::TrainLayout L = mhe::train_layout(n_streams);
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    HIP_TRY(mhe::launch_train_count(d_data, d_in_off, n_streams, total, order, prev0, d_ws, st));
    uint32_t head[4];
    uint64_t nslots = 0;
    HIP_TRY(hipMemcpyAsync(head, ws, sizeof head, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&nslots, ws + L.off_counts + n_streams * 8, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (head[mhe::TRAIN_STATUS]) return status_from_device(int(head[mhe::TRAIN_STATUS]));
    if (nslots > uint64_t(INT32_MAX)) return MH_ERR_ARG;                 // (tree_build_kernel's grid)
    mh_model_set *s = new (std::nothrow) mh_model_set;
    if (!s) return MH_ERR_NOMEM;
    DevBuf nodes;                                                        // tree_build_kernel's node arrays, until the end of the call
    hipError_t e = set_alloc(s, n_streams, nslots);
    if (e == hipSuccess) e = nodes.alloc(size_t(nslots) * mhe::TREE_NODE_BYTES);
    mhe::TreeNodes t{};
    if (e == hipSuccess) {
        unsigned char *b = static_cast<unsigned char *>(nodes.p);
        const size_t per = size_t(nslots) * mhk::TB_NODE_STRIDE;
        t.left = reinterpret_cast<uint16_t *>(b);
        t.right = t.left + per;
        t.meta = reinterpret_cast<uint32_t *>(t.right + per);
        t.sym = reinterpret_cast<uint8_t *>(t.meta + size_t(nslots) * mhk::TB_META_STRIDE);
        t.height = t.sym + per;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(s->d.slot_base, ws + L.off_counts, (n_streams + 1) * 8, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && nslots) e = hipMemsetAsync(s->d.code64, 0, size_t(nslots) * 2048, st);   // the counts
    if (e == hipSuccess) e = mhe::launch_train_build(d_data, d_in_off, total, order, prev0, s->d, t, d_ws, st);
    if (e == hipSuccess) e = hipMemcpyAsync(head, ws, sizeof head, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { delete s; return hip_fail(e); }
    int rc = head[mhe::TRAIN_STATUS] ? status_from_device(int(head[mhe::TRAIN_STATUS])) : MH_OK;
    if (rc == MH_OK && head[mhe::TRAIN_MAXLEN] > uint32_t(mh::MAX_CODE_BITS)) rc = MH_ERR_CODE_TOO_LONG;
    if (rc != MH_OK) { delete s; return rc; }
    s->max_len = int(head[mhe::TRAIN_MAXLEN]);
    s->min_len = head[mhe::TRAIN_MINLEN] == 0xFFFFFFFFu ? 0 : int(head[mhe::TRAIN_MINLEN]);
    *out = s;
    return MH_OK;
}

int mh_model_set_from_models(const mh_model *const *models, size_t n_streams, mh_model_set **out) {
    if (!out || (!models && n_streams)) return MH_ERR_ARG;
    *out = nullptr;
    for (size_t i = 0; i < n_streams; ++i)
        if (!models[i] || (models[i]->type != 0 && models[i]->type != 1)) return MH_ERR_ARG;
    HostSet h(n_streams);
    for (size_t i = 0; i < n_streams; ++i) {
        int rc = ensure_mirror(models[i]);
        if (rc == MH_OK) rc = h.add_model(i, models[i]->host);
        if (rc != MH_OK) return rc;
    }
    return h.upload(out);
}

int mh_model_set_from_tables(const uint8_t *tables, const uint64_t *tab_off, size_t n_streams, mh_model_set **out) {
    if (!out || !tab_off) return MH_ERR_ARG;
    *out = nullptr;
    if (!offsets_ok(tab_off, n_streams) || (!tables && tab_off[n_streams])) return MH_ERR_ARG;
    HostSet h(n_streams);
    mh::ContextCoder cc;
    for (size_t i = 0; i < n_streams; ++i) {
        const int rc = h.add_table(i, tables + tab_off[i], size_t(tab_off[i + 1] - tab_off[i]), cc);
        if (rc != MH_OK) return rc;
    }
    return h.upload(out);
}

void mh_model_set_free(mh_model_set *s) { delete s; }
size_t mh_model_set_size(const mh_model_set *s) { return s ? size_t(s->d.n) : 0; }
size_t mh_model_set_slots(const mh_model_set *s) { return s ? size_t(s->d.nslots) : 0; }

int mh_model_set_stream_info(const mh_model_set *s, size_t i, int *type, int *max_code_len) {
    if (!s || i >= s->d.n) return MH_ERR_ARG;
    uint8_t t = 0;
    uint32_t ml = 0;
    HIP_TRY(hipMemcpy(&t, s->d.type + i, 1, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&ml, s->d.maxlen + i, 4, hipMemcpyDeviceToHost));
    if (type) *type = t;
    if (max_code_len) *max_code_len = int(ml);
    return MH_OK;
}

int mh_model_set_code_lens(const mh_model_set *s, int *max_code_len, int *min_code_len) {
    if (!s) return MH_ERR_ARG;
    if (max_code_len) *max_code_len = s->max_len;
    if (min_code_len) *min_code_len = s->min_len;
    return MH_OK;
}

size_t mh_model_set_tables_bound(const mh_model_set *s) {
    // per stream the type bit and 256 context bits; per slot 10 bits per leaf, at most 256 + 1 leaves
    return s ? size_t(s->d.n) * 33 + size_t(s->d.nslots) * 322 + 16 : 0;
}

size_t mh_dev_model_set_tables_workspace(const mh_model_set *s) { return s ? mhe::tab_layout(s->d.n, s->d.nslots).total : 0; }

int mh_dev_model_set_tables(const mh_model_set *s, uint8_t *d_out, size_t cap, uint64_t *d_tab_off, void *d_ws, size_t ws_bytes, void *stream) {
    if (!s || s->view || (!d_out && cap) || !d_tab_off || !d_ws || !aligned16(d_out) || !aligned16(d_ws)) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_model_set_tables_workspace(s)) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    HIP_TRY(mhe::launch_tables(s->d, d_out, cap, reinterpret_cast<unsigned long long *>(d_tab_off), d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

size_t mh_encode_each_bound(const mh_model_set *s, size_t total, size_t n_streams) {
    size_t maxlen = s ? size_t(s->max_len) : 64;
    if (maxlen < 1) maxlen = 1;
    return (total * maxlen + 7) / 8 + n_streams + 16;
}

size_t mh_dev_encode_each_workspace(size_t n_streams, size_t total) { return mhb::enc_layout(n_streams, total).total; }

int mh_dev_encode_each(const mh_model_set *s, const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint8_t prev0,
                       uint8_t *d_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_nbits, uint64_t *d_index, uint32_t chunk_symbols,
                       void *d_ws, size_t ws_bytes, void *stream) {
    if (!s || n_streams != s->d.n || (!d_data && total) || !d_in_off || !d_out_off || (!d_nbits && n_streams) || (!d_payload && cap) || !d_ws)
        return MH_ERR_ARG;
    if (!aligned16(d_payload) || !aligned16(d_ws)) return MH_ERR_ARG;
    const int shift = d_index ? chunk_shift_of(chunk_symbols) : 0;
    if (shift < 0) return MH_ERR_ARG;
    if (ws_bytes < mh_dev_encode_each_workspace(n_streams, total)) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    mhe::EncEachParams p{};
    p.data = d_data; p.in_off = d_in_off; p.n = n_streams; p.total = total; p.prev0 = prev0;
    p.chunk_shift = uint32_t(shift);
    p.index = reinterpret_cast<unsigned long long *>(d_index);
    p.out = d_payload; p.cap = cap;
    p.out_off = reinterpret_cast<unsigned long long *>(d_out_off);
    p.nbits = reinterpret_cast<unsigned long long *>(d_nbits);
    p.set = s->d;
    HIP_TRY(mhe::launch_encode_each(p, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

size_t mh_dev_decode_each_workspace(size_t n_streams) { return mhb::dec_layout(n_streams).total; }

int mh_dev_decode_each(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams,
                       uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap, uint64_t *d_sym_off, uint64_t sym_total,
                       const uint64_t *d_index, uint32_t chunk_symbols, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!s || n_streams != s->d.n || !d_sym_off || (!d_out && out_cap) || !aligned16(d_out)) return MH_ERR_ARG;
    const CodedBatch a{d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols};
    const mhb::DecLayout L = mhb::dec_layout(n_streams);
    mhb::DecodeParams p{};
    mhb::DecBatchParams &b = p.b;
    const int rc = dev_batch_params(a, SymOff::Through, prev0, d_ws, ws_bytes, L.total, L.off_status, d_stream_status, b);
    if (rc != MH_OK) return rc;
    if (d_index && sym_total > out_cap) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    b.out = d_out; b.out_cap = out_cap;
    p.set = s->d;
    HIP_TRY(mhb::launch_decode(p, mhb::Model::Set, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

/* ------------------------------------------------------- host-buffer calls */

int mh_compress_each_bounds(const uint64_t *in_off, size_t n_streams, size_t *tables_bound, size_t *payload_bound) {
    if (!in_off || !offsets_ok(in_off, n_streams)) return MH_ERR_ARG;
    size_t pay = n_streams + 16;
    for (size_t i = 0; i < n_streams; ++i) pay += size_t(stream_pay_bound(in_off[i + 1] - in_off[i]));
    if (tables_bound) *tables_bound = n_streams * 33 + (size_t(in_off[n_streams]) * 20 + 7) / 8 + 16;
    if (payload_bound) *payload_bound = pay;
    return MH_OK;
}

namespace {

// one stream through the single-stream calls (histogram, model, table, encode) into the caller's buffers
int compress_direct(const uint8_t *m, size_t len, int order, uint8_t prev0, uint8_t *tables, size_t tab_cap, uint64_t &tab_pos,
                    uint8_t *payload, size_t cap, uint64_t &pay_pos, uint64_t &nbits, uint64_t *index, uint32_t chunk) {
    std::vector<uint64_t> counts(order ? 65536 : 256);
    int rc = order ? mh_histogram_o1(m, len, prev0, counts.data()) : mh_histogram_o0(m, len, counts.data());
    if (rc != MH_OK) return rc;
    mh_model *model = nullptr;
    if ((rc = mh_model_from_counts(counts.data(), order, &model)) != MH_OK) return rc;
    size_t tb = 0;
    rc = mh_model_write_table(model, nullptr, 0, &tb);
    if (rc == MH_OK && tab_pos + tb > tab_cap) rc = MH_ERR_CAPACITY;
    if (rc == MH_OK) rc = mh_model_write_table(model, tables + tab_pos, tb, &tb);
    std::vector<uint8_t> out;
    if (rc == MH_OK) {
        out.resize(mh_encode_bound(model, len));
        rc = mh_encode(model, m, len, prev0, out.data(), out.size(), &nbits, index, chunk);
    }
    mh_model_free(model);
    if (rc != MH_OK) return rc;
    const uint64_t pb = (nbits + 7) / 8;
    if (pay_pos + pb > cap) return MH_ERR_CAPACITY;
    if (pb) std::memcpy(payload + pay_pos, out.data(), size_t(pb));
    tab_pos += tb;
    pay_pos += pb;
    return MH_OK;
}

// streams [g0, g1) (none longer than MH_EACH_DIRECT_BYTES) on the device: train, tables, encode
int compress_group(const uint8_t *data, const uint64_t *in_off, size_t g0, size_t g1, int order, uint8_t prev0, uint8_t *tables, size_t tab_cap,
                   uint64_t *tab_off, uint64_t &tab_pos, uint8_t *payload, size_t cap, uint64_t *out_off, uint64_t &pay_pos, uint64_t *nbits,
                   uint64_t *index, uint32_t chunk) {
    const size_t n = g1 - g0;
    const uint64_t base = in_off[g0], total = in_off[g1] - base;
    std::vector<uint64_t> off(n + 1);
    for (size_t k = 0; k <= n; ++k) off[k] = in_off[g0 + k] - base;
    const hipStream_t st = nullptr;
    DevBuf d_data, d_off, d_ws;
    HIP_TRY(d_data.alloc(total));
    HIP_TRY(d_off.alloc((n + 1) * 8));
    if (total) HIP_TRY(stage_h2d(d_data.p, data + base, size_t(total), st));
    HIP_TRY(hipMemcpy(d_off.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    const size_t wtrain = mh_dev_model_set_train_workspace(n);
    const size_t wenc = mh_dev_encode_each_workspace(n, total);
    mh_model_set *s = nullptr;
    {
        DevBuf d_tw;
        HIP_TRY(d_tw.alloc(wtrain));
        const int rc = mh_dev_model_set_train(d_data.as<uint8_t>(), d_off.as<uint64_t>(), n, total, order, prev0, d_tw.p, wtrain, st, &s);
        if (rc != MH_OK) return rc;
    }
    std::unique_ptr<mh_model_set, void (*)(mh_model_set *)> own(s, mh_model_set_free);
    const size_t tbound = mh_model_set_tables_bound(s), wtab = mh_dev_model_set_tables_workspace(s);
    size_t pbound = n + 16;
    for (size_t k = 0; k < n; ++k) pbound += size_t(stream_pay_bound(off[k + 1] - off[k]));
    pbound = std::min(pbound, mh_encode_each_bound(s, total, n));
    const size_t nidx = index ? size_t(mh_batch_index_capacity(total, n, chunk)) : 0;
    DevBuf d_tab, d_toff, d_pay, d_poff, d_nb, d_idx;
    HIP_TRY(d_ws.alloc(std::max(wtab, wenc)));
    HIP_TRY(d_tab.alloc(tbound));
    HIP_TRY(d_toff.alloc((n + 1) * 8));
    HIP_TRY(d_pay.alloc(pbound));
    HIP_TRY(d_poff.alloc((n + 1) * 8));
    HIP_TRY(d_nb.alloc(n * 8));
    HIP_TRY(d_idx.alloc(nidx * 8));
    int rc = mh_dev_model_set_tables(s, d_tab.as<uint8_t>(), tbound, d_toff.as<uint64_t>(), d_ws.p, wtab, st);
    if (rc == MH_OK) rc = mh_dev_status(d_ws.p, st);
    if (rc != MH_OK) return rc;
    rc = mh_dev_encode_each(s, d_data.as<uint8_t>(), d_off.as<uint64_t>(), n, total, prev0, d_pay.as<uint8_t>(), pbound, d_poff.as<uint64_t>(),
                            d_nb.as<uint64_t>(), index ? d_idx.as<uint64_t>() : nullptr, chunk, d_ws.p, wenc, st);
    if (rc == MH_OK) rc = mh_dev_status(d_ws.p, st);
    if (rc != MH_OK) return rc;
    std::vector<uint64_t> toff(n + 1), poff(n + 1);
    HIP_TRY(hipMemcpy(toff.data(), d_toff.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(poff.data(), d_poff.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    if (tab_pos + toff[n] > tab_cap || pay_pos + poff[n] > cap) return MH_ERR_CAPACITY;
    if (toff[n]) HIP_TRY(stage_d2h(tables + tab_pos, d_tab.p, size_t(toff[n]), st));
    if (poff[n]) HIP_TRY(stage_d2h(payload + pay_pos, d_pay.p, size_t(poff[n]), st));
    if (n) HIP_TRY(hipMemcpy(nbits + g0, d_nb.p, n * 8, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; ++k) { tab_off[g0 + k] = tab_pos + toff[k]; out_off[g0 + k] = pay_pos + poff[k]; }
    tab_pos += toff[n];
    pay_pos += poff[n];
    if (index && nidx) {
        std::vector<uint64_t> idx(nidx);
        HIP_TRY(hipMemcpy(idx.data(), d_idx.p, nidx * 8, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; ++k) {
            const uint64_t len = off[k + 1] - off[k], cnt = (len + chunk - 1) / chunk;
            const uint64_t from = mh_batch_index_base(off[k], k, chunk), to = mh_batch_index_base(in_off[g0 + k], g0 + k, chunk);
            if (cnt) std::memcpy(index + to, idx.data() + from, size_t(cnt) * 8);
        }
    }
    return MH_OK;
}

// device footprint of one stream in a compress group: input, payload and table bounds, set (worst case: one slot per
// byte up to the context count), offsets, index and unit words
size_t stream_footprint(uint64_t len, int order, uint32_t chunk) {
    const uint64_t slots = std::min<uint64_t>(len, order ? 256 : 1);
    return size_t(len + stream_pay_bound(len) + 33 + (len * 20) / 8 + mhe::STREAM_BYTES + 64 + slots * (mhe::SLOT_BYTES + mhe::TREE_NODE_BYTES + 322) + len / 128 +
                  (chunk ? (len / chunk + 1) * 8 : 0));
}

}  // namespace

int mh_compress_each(const uint8_t *data, const uint64_t *in_off, size_t n_streams, int order, uint8_t prev0, uint8_t *tables, size_t tab_cap,
                     uint64_t *tab_off, uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *nbits, uint64_t *index, uint32_t chunk_symbols) {
    if (!in_off || !tab_off || !out_off || (!nbits && n_streams) || (!tables && tab_cap) || (!out_payload && cap)) return MH_ERR_ARG;
    if (order != 0 && order != 1) return MH_ERR_ARG;
    if (index && chunk_shift_of(chunk_symbols) < 0) return MH_ERR_ARG;
    if (!offsets_ok(in_off, n_streams)) return MH_ERR_ARG;
    if (!data && in_off[n_streams]) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const uint32_t chunk = index ? chunk_symbols : 0;
    const size_t budget = group_budget();
    uint64_t tab_pos = 0, pay_pos = 0;
    size_t g0 = 0, acc = 0;
    auto flush = [&](size_t g1) -> int {
        if (g1 == g0) return MH_OK;
        return compress_group(data, in_off, g0, g1, order, prev0, tables, tab_cap, tab_off, tab_pos, out_payload, cap, out_off, pay_pos, nbits, index, chunk);
    };
    for (size_t i = 0; i < n_streams; ++i) {
        const uint64_t len = in_off[i + 1] - in_off[i];
        if (len > MH_EACH_DIRECT_BYTES) {
            int rc = flush(i);
            if (rc != MH_OK) return rc;
            tab_off[i] = tab_pos;
            out_off[i] = pay_pos;
            rc = compress_direct(data + in_off[i], size_t(len), order, prev0, tables, tab_cap, tab_pos, out_payload, cap, pay_pos, nbits[i],
                                 index ? index + mh_batch_index_base(in_off[i], i, chunk) : nullptr, chunk);
            if (rc != MH_OK) return rc;
            g0 = i + 1; acc = 0;
            continue;
        }
        const size_t f = stream_footprint(len, order, chunk);
        if (i > g0 && acc + f > budget) {
            const int rc = flush(i);
            if (rc != MH_OK) return rc;
            g0 = i; acc = 0;
        }
        acc += f;
    }
    const int rc = flush(n_streams);
    if (rc != MH_OK) return rc;
    tab_off[n_streams] = tab_pos;
    out_off[n_streams] = pay_pos;
    return MH_OK;
}

namespace {
// streams [g0, g1) on the device; index-free streams over the walk cap are decoded by mh_decode with a host model.
// Output bytes go to out + pos (index: the caller's sym_off), statuses to sst.
int decompress_group(const uint8_t *tables, const uint64_t *tab_off, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                     size_t g0, size_t g1, uint8_t prev0, uint8_t *out, size_t out_cap, uint64_t *sym_off, uint64_t &pos, const uint64_t *index,
                     uint32_t chunk, std::vector<int32_t> &sst, int &first) {
    const size_t n = g1 - g0;
    std::vector<uint64_t> toff(n + 1), poff(n + 1), so(n + 1, 0);
    for (size_t k = 0; k <= n; ++k) { toff[k] = tab_off[g0 + k] - tab_off[g0]; poff[k] = pay_off[g0 + k] - pay_off[g0]; }
    if (index) for (size_t k = 0; k <= n; ++k) so[k] = sym_off[g0 + k] - sym_off[g0];
    mh_model_set *s = nullptr;
    int rc = mh_model_set_from_tables(tables + tab_off[g0], toff.data(), n, &s);
    if (rc != MH_OK) return rc;
    std::unique_ptr<mh_model_set, void (*)(mh_model_set *)> own(s, mh_model_set_free);
    const hipStream_t st = nullptr;
    const uint64_t pay_total = poff[n], sym_total = so[n];
    std::vector<size_t> long_streams;
    uint64_t dcap = sym_total;
    if (!index) {
        const uint64_t minl = uint64_t(s->min_len > 0 ? s->min_len : 1);
        dcap = 0;
        for (size_t k = 0; k < n; ++k) {
            if (nbits[g0 + k] > MH_BATCH_WALK_MAX_BITS) long_streams.push_back(k);
            else dcap += nbits[g0 + k] / minl;
        }
    }
    // the group as a batch of its own: offsets re-based to it, its index slices moved to where its sym_off puts them
    std::vector<uint64_t> idx;
    if (index) {
        idx.assign(size_t(mh_batch_index_capacity(sym_total, n, chunk)), 0);
        for (size_t k = 0; k < n; ++k) {
            const uint64_t len = so[k + 1] - so[k], cnt = (len + chunk - 1) / chunk;
            const uint64_t to = mh_batch_index_base(so[k], k, chunk), from = mh_batch_index_base(sym_off[g0 + k], g0 + k, chunk);
            if (cnt) std::memcpy(idx.data() + to, index + from, size_t(cnt) * 8);
        }
    }
    const CodedBatch a{payload + pay_off[g0], poff.data(), nbits + g0, n, pay_total, prev0, so.data(), sym_total, index ? idx.data() : nullptr, chunk};
    const size_t wsb = mh_dev_decode_each_workspace(n);
    DevBatch db;
    DevBuf d_out, d_st, d_ws;
    HIP_TRY(d_out.alloc(size_t(dcap)));
    HIP_TRY(d_st.alloc(n * 4));
    HIP_TRY(d_ws.alloc(wsb));
    if ((rc = db.upload(a, st)) != MH_OK) return rc;
    rc = mh_dev_decode_each(s, db.d.payload, db.d.pay_off, db.d.nbits, n, pay_total, prev0, d_out.as<uint8_t>(), dcap, db.so.as<uint64_t>(), sym_total,
                            db.d.index, chunk, d_st.as<int32_t>(), d_ws.p, wsb, st);
    if (rc != MH_OK) return rc;
    const int dev_rc = mh_dev_status(d_ws.p, st);
    std::vector<int32_t> g_st(n);
    if (n) HIP_TRY(hipMemcpy(g_st.data(), d_st.p, n * 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> dso(n + 1);
    HIP_TRY(hipMemcpy(dso.data(), db.so.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    std::vector<uint8_t> dev_bytes(static_cast<size_t>(dso[n]));
    if (!dev_bytes.empty()) HIP_TRY(stage_d2h(dev_bytes.data(), d_out.p, dev_bytes.size(), st));
    std::vector<std::vector<uint8_t>> extra(long_streams.size());
    for (size_t j = 0; j < long_streams.size(); ++j) {             // over the walk cap: the stream's own model through mh_decode
        const size_t k = long_streams[j], i = g0 + k;
        mh_model *m = nullptr;
        int r = toff[k + 1] > toff[k] ? mh_model_from_table_bits(tables + tab_off[i], size_t(toff[k + 1] - toff[k]), &m) : MH_ERR_CORRUPT;
        size_t nb = 0;
        if (r == MH_OK) r = mh_decode_to(m, payload + pay_off[i], nbits[i], prev0, grow_vec, &extra[j], &nb, nullptr, 0, 0);
        if (m) mh_model_free(m);
        extra[j].resize(r == MH_OK ? nb : 0);
        g_st[k] = r;
    }
    if (dev_rc != MH_OK && dev_rc != MH_ERR_ARG && first == MH_OK) {
        bool any = false;
        for (size_t k = 0; k < n; ++k) any |= g_st[k] != MH_OK;
        if (!any) first = dev_rc;
    }
    size_t j = 0;
    for (size_t k = 0; k < n; ++k) {
        const bool is_long = j < long_streams.size() && long_streams[j] == k;
        const uint8_t *src = is_long ? extra[j].data() : dev_bytes.data() + dso[k];
        const uint64_t len = is_long ? extra[j].size() : dso[k + 1] - dso[k];
        if (is_long) ++j;
        sst[g0 + k] = g_st[k];
        if (g_st[k] != MH_OK && first == MH_OK) first = g_st[k];
        const uint64_t at = index ? sym_off[g0 + k] : pos;
        if (!index) sym_off[g0 + k] = pos;
        if (at + len > out_cap) { sst[g0 + k] = MH_ERR_CAPACITY; if (first == MH_OK) first = MH_ERR_CAPACITY; }
        else if (len && g_st[k] == MH_OK) std::memcpy(out + at, src, size_t(len));
        pos += len;
    }
    return MH_OK;
}
}  // namespace

int mh_decompress_each(const uint8_t *tables, const uint64_t *tab_off, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                       size_t n_streams, uint8_t prev0, uint8_t *out, size_t out_cap, uint64_t *sym_off, const uint64_t *index,
                       uint32_t chunk_symbols, int32_t *stream_status) {
    if (!tab_off || !sym_off || (!out && out_cap)) return MH_ERR_ARG;
    if (!offsets_ok(tab_off, n_streams) || (!tables && tab_off[n_streams])) return MH_ERR_ARG;
    CodedBatch a{payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols};
    const int arc = host_batch_args(a, index != nullptr);
    if (arc != MH_OK) return arc;
    if (a.sym_total > out_cap) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const uint32_t chunk = index ? chunk_symbols : 0;
    const size_t budget = group_budget();
    std::vector<int32_t> sst(n_streams, MH_OK);
    int first = MH_OK;
    uint64_t pos = 0;
    size_t g0 = 0, acc = 0;
    for (size_t i = 0; i <= n_streams; ++i) {
        size_t f = 0;
        if (i < n_streams) {
            // payload, output (at most nbits symbols), table-derived set (at most one slot per 10 table bits + 1)
            const uint64_t tb = tab_off[i + 1] - tab_off[i];
            f = size_t(pay_off[i + 1] - pay_off[i] + nbits[i] + mhe::STREAM_BYTES + 64 + std::min<uint64_t>(tb * 8 / 20 + 1, 256) * mhe::SLOT_BYTES +
                       (index ? (sym_off[i + 1] - sym_off[i]) / chunk * 8 + 8 : 0));
        }
        if (i == n_streams || (i > g0 && acc + f > budget)) {
            if (i > g0) {
                const int rc = decompress_group(tables, tab_off, payload, pay_off, nbits, g0, i, prev0, out, out_cap, sym_off, pos, index, chunk, sst, first);
                if (rc != MH_OK) return rc;
            }
            g0 = i; acc = 0;
        }
        acc += f;
    }
    if (!index) sym_off[n_streams] = pos;
    if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
    return first;
}

}  // extern "C"
