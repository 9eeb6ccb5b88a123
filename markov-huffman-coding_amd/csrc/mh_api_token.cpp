// mh_api_token.cpp — the span-token calls of the C ABI (include/mh.h, "TOKENS FROM MATCHED BYTES"): the argument rules of the
// device call (kernels: mh_token.hip) and the host form, which reads its batch through mh_api_reader.hpp.  The digest of a
// byte string and the format rules are mh_token_host.cpp's.
#include "mh_api_reader.hpp"
#include "mh_token.h"

using namespace mhapi;

extern "C" {

size_t mh_dev_span_tokens_workspace(size_t n_streams, size_t n_reps) {
    (void)n_streams;                                               // nothing is kept per stream
    return mht::token_layout(n_reps).total;
}

int mh_dev_span_tokens_batch(const mh_span_tokens_args *a, const mh_launch *launch) {
    if (!a || !launch || a->struct_size != sizeof(mh_span_tokens_args)) return MH_ERR_ARG;
    if ((a->src != nullptr) == (a->src_set != nullptr) || (a->src && !order012(a->src))) return MH_ERR_ARG;
    const mh_coded_batch_args &b = a->batch;
    if (a->src_set && b.n_streams != a->src_set->d.n) return MH_ERR_ARG;
    if (a->flags & ~MH_TOKEN_FOLD) return MH_ERR_ARG;
    if (!a->d_span_off || !a->d_rep_off || !a->d_fmt_off || (a->n_formats && !a->d_hex_digits)) return MH_ERR_ARG;
    if ((a->n_reps && (!a->d_spans || !a->d_rep_tag)) || (b.n_streams && !a->d_stream_status)) return MH_ERR_ARG;
    void *d_ws = launch->d_ws;
    int shift;
    if (!dev_batch_ptrs_ok(b.d_payload, b.pay_total, b.d_pay_off, b.d_nbits, b.n_streams, d_ws) ||
        !index_args_ok(b.d_index, b.chunk_symbols, b.d_sym_off, shift))
        return MH_ERR_ARG;
    if (launch->ws_bytes < mht::token_layout(a->n_reps).total) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if ((a->src ? a->src->max_len : a->src_set->max_len) > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (a->src && !a->src->d_prim) return MH_ERR_NO_DEVICE;
    mht::TokenParams p{};
    p.b.payload = b.d_payload; p.b.pay_off = b.d_pay_off; p.b.nbits = b.d_nbits; p.b.n_streams = b.n_streams;
    p.b.prev0 = ctx_of_prev0(a->src, b.prev0);
    p.b.sym_off = b.d_index ? b.d_sym_off : nullptr;               // (read under an index only)
    p.b.index = b.d_index; p.b.chunk_shift = uint32_t(shift);
    p.b.walk_max_bits = MH_BATCH_WALK_MAX_BITS;
    mhb::Model model = mhb::Model::Set;
    if (a->src) {
        fill_dec_tables(a->src, p.b.tab);
        model = order2(a->src) ? mhb::Model::Shared2 : mhb::Model::Shared;
    } else {
        p.b.set = a->src_set->d;
    }
    p.pay_total = b.pay_total; p.sym_total = b.d_index ? b.sym_total : 0;
    p.stream_status = a->d_stream_status;
    p.span_off = reinterpret_cast<const unsigned long long *>(a->d_span_off);
    p.spans = reinterpret_cast<const unsigned long long *>(a->d_spans);
    p.span_tag = a->d_span_tag;
    p.k0 = mht::load_le64(a->key); p.k1 = mht::load_le64(a->key + 8);
    p.fold = (a->flags & MH_TOKEN_FOLD) != 0;
    p.fmt_off = a->d_fmt_off; p.fmt_bytes = a->d_fmt_bytes; p.hex_digits = a->d_hex_digits; p.n_formats = a->n_formats;
    p.n_reps = a->n_reps;
    p.rep_off = reinterpret_cast<unsigned long long *>(a->d_rep_off);
    p.rep_bytes = a->d_rep_bytes; p.rep_cap = a->rep_cap; p.rep_tag = a->d_rep_tag;
    HIP_TRY(mht::launch_span_tokens(p, model, d_ws, static_cast<hipStream_t>(launch->stream)));
    return MH_OK;
}

int mh_span_tokens_batch(const mh_model *src, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams,
                         uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, const uint64_t *span_off,
                         const uint64_t *spans, const uint32_t *span_tag, const uint8_t *key, uint32_t flags, const uint64_t *fmt_off,
                         const uint8_t *fmt_bytes, const uint8_t *hex_digits, size_t n_formats, uint64_t *rep_off, uint8_t *rep_bytes,
                         size_t rep_cap, uint32_t *rep_tag, int32_t *stream_status) {
    if (!order012(src) || !key || (flags & ~MH_TOKEN_FOLD) || !span_off || !rep_off) return MH_ERR_ARG;
    int rc = mht::formats_check(fmt_off, fmt_bytes, hex_digits, n_formats);
    if (rc != MH_OK) return rc;
    CodedBatch a{payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols};
    if ((rc = host_batch_args(a, a.index != nullptr)) != MH_OK) return rc;
    if (!offsets_ok(span_off, n_streams)) return MH_ERR_ARG;
    const size_t n_reps = size_t(span_off[n_streams]);
    if (n_reps && (!spans || !rep_tag || !n_formats)) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (src->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    // an index-free batch with a stream over the walk cap is indexed first (a span's positions do not depend on the index)
    std::vector<uint64_t> own_idx, own_so(n_streams + 1, 0);
    std::vector<int32_t> idx_st;
    if (over_walk_cap(a) && (rc = index_first(src, a, false, own_so.data(), own_idx, idx_st)) != MH_OK) return rc;
    const hipStream_t st = nullptr;
    DevBatch db;
    if ((rc = db.upload(a, st)) != MH_OK) return rc;
    const size_t fmt_total = size_t(fmt_off[2 * n_formats]);
    const size_t wsb = mh_dev_span_tokens_workspace(n_streams, n_reps);
    DevBuf d_soff, d_sp, d_tag, d_foff, d_fb, d_hex, d_roff, d_rb, d_rtag, d_st, d_ws;
    HIP_TRY(d_soff.alloc((n_streams + 1) * 8));
    HIP_TRY(d_sp.alloc(n_reps * 16));
    HIP_TRY(d_tag.alloc(n_reps * 4));
    HIP_TRY(d_foff.alloc((2 * n_formats + 1) * 8));
    HIP_TRY(d_fb.alloc(fmt_total));
    HIP_TRY(d_hex.alloc(n_formats));
    HIP_TRY(d_roff.alloc((n_reps + 1) * 8));
    HIP_TRY(d_rb.alloc(rep_bytes ? rep_cap : 0));
    HIP_TRY(d_rtag.alloc(n_reps * 4));
    HIP_TRY(d_st.alloc(n_streams * 4));
    HIP_TRY(d_ws.alloc(wsb));
    HIP_TRY(hipMemcpy(d_soff.p, span_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
    if (n_reps) HIP_TRY(hipMemcpy(d_sp.p, spans, n_reps * 16, hipMemcpyHostToDevice));
    if (n_reps && span_tag) HIP_TRY(hipMemcpy(d_tag.p, span_tag, n_reps * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_foff.p, fmt_off, (2 * n_formats + 1) * 8, hipMemcpyHostToDevice));
    if (fmt_total) HIP_TRY(hipMemcpy(d_fb.p, fmt_bytes, fmt_total, hipMemcpyHostToDevice));
    if (n_formats) HIP_TRY(hipMemcpy(d_hex.p, hex_digits, n_formats, hipMemcpyHostToDevice));
    mh_span_tokens_args t{};
    t.struct_size = sizeof t;
    t.src = src;
    t.batch = mh_coded_batch_args{db.d.payload, db.d.pay_off, db.d.nbits, db.d.n, db.d.pay_total, db.d.prev0,
                                  const_cast<uint64_t *>(db.d.sym_off), db.d.sym_total, db.d.index, db.d.chunk_symbols};
    t.d_span_off = d_soff.as<uint64_t>(); t.d_spans = d_sp.as<uint64_t>(); t.d_span_tag = span_tag ? d_tag.as<uint32_t>() : nullptr;
    std::memcpy(t.key, key, 16);
    t.flags = flags;
    t.d_fmt_off = d_foff.as<uint64_t>(); t.d_fmt_bytes = d_fb.as<uint8_t>(); t.d_hex_digits = d_hex.as<uint8_t>(); t.n_formats = n_formats;
    t.n_reps = n_reps;
    t.d_rep_off = d_roff.as<uint64_t>(); t.d_rep_bytes = rep_bytes ? d_rb.as<uint8_t>() : nullptr; t.rep_cap = rep_cap;
    t.d_rep_tag = d_rtag.as<uint32_t>(); t.d_stream_status = d_st.as<int32_t>();
    const mh_launch launch{d_ws.p, wsb, st};
    if ((rc = mh_dev_span_tokens_batch(&t, &launch)) != MH_OK) return rc;
    const int dev_rc = mh_dev_status(d_ws.p, st);
    std::vector<int32_t> sst(n_streams);
    if (n_streams) HIP_TRY(hipMemcpy(sst.data(), d_st.p, n_streams * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rep_off, d_roff.p, (n_reps + 1) * 8, hipMemcpyDeviceToHost));
    if (n_reps) HIP_TRY(hipMemcpy(rep_tag, d_rtag.p, n_reps * 4, hipMemcpyDeviceToHost));
    const bool fits = rep_bytes && dev_rc != MH_ERR_CAPACITY && rep_off[n_reps] <= rep_cap;
    if (fits && rep_off[n_reps]) HIP_TRY(hipMemcpy(rep_bytes, d_rb.p, size_t(rep_off[n_reps]), hipMemcpyDeviceToHost));
    // a stream that indexing the batch first failed has no symbols on the device, where its spans got tokens of the empty
    // string: every entry of a failed stream is empty, so they are taken out here and the table is closed up
    bool idx_failed = false;
    for (int32_t v : idx_st) idx_failed |= v != MH_OK;
    if (idx_failed) {
        uint64_t from = 0, to = 0;
        for (size_t i = 0; i < n_streams; ++i)
            for (uint64_t r = span_off[i]; r < span_off[i + 1]; ++r) {
                const uint64_t len = rep_off[r + 1] - from;
                from = rep_off[r + 1];
                rep_off[r] = to;
                if (idx_st[i] != MH_OK) continue;
                if (fits && len) std::memmove(rep_bytes + to, rep_bytes + (from - len), size_t(len));
                to += len;
            }
        rep_off[n_reps] = to;
    }
    const int first = first_failure(sst, idx_st, dev_rc);
    if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
    return first;
}

}  // extern "C"
