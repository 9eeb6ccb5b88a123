// mh_api_recode.cpp — the re-coding calls of the C ABI (include/mh.h, "RE-CODING BATCHES" and the re-coding part of "ORDER 2
// IN SEARCH AND RE-CODING"): the training histogram of a compressed batch and the batch coded again under another model,
// under one shared source model of any order or a model set (kernels: mh_recode.hip), with the edits of "EDITING BATCHES" and
// the splices of "SPLICING BATCHES", their order-2 forms of "ORDER 2 IN EDITING AND SPLICING", and the host-buffer forms.  The order
// rules of an entry point are in that entry point; everything behind them is here once.
#include "mh_api_reader.hpp"
#include "mh_recode.h"

using namespace mhapi;

namespace {

// the source's models: a shared model's decode tables (order 0/1 as mh_dev_decode_batch hands them over, order 2 as
// mh_dev_decode_batch_o2), or the set
int source_tables(const mh_model *m, const mh_model_set *set, mhr::Src &s, mhb::Model &model) {
    if (set) {
        if (!have_device()) return MH_ERR_NO_DEVICE;
        s.set = set->d;
        model = mhb::Model::Set;
        return MH_OK;
    }
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    fill_dec_tables(m, s.b);
    model = m->type == 2 ? mhb::Model::Shared2 : mhb::Model::Shared;
    return MH_OK;
}

// behind the order rules of mh_dev_histogram_coded_batch, _each and _batch_o2: m or set is the source (m: null under a set)
int histogram_coded(const mh_model *m, const mh_model_set *set, int order, const CodedBatch &a, uint64_t *d_counts, int32_t *d_stream_status,
                    void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_counts) return MH_ERR_ARG;
    mhr::HistParams p{};
    const mhr::HistLayout L = mhr::hist_layout(a.n);
    const int rc = dev_batch_params(a, SymOff::Through, ctx_of_prev0(m, a.prev0), d_ws, ws_bytes, L.total, L.off_status, d_stream_status, p.s.b);
    if (rc != MH_OK) return rc;
    p.order = uint32_t(order);
    p.counts = reinterpret_cast<unsigned long long *>(d_counts);
    mhb::Model model;
    const int t = source_tables(m, set, p.s, model);
    if (t != MH_OK) return t;
    HIP_TRY(mhr::launch_histogram_coded(p, model, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

// behind the order rules of mh_dev_recode_batch, _each, _batch_o2 and the _edit calls: m or set is the source; a.sym_off is
// written by an index-free re-code; seam: the workspace of the _o2 call, which has room for the seam's arrays; ed: the edit
// of an _edit call (the _o2 edit passes seam as well)
int recode(const mh_model *m, const mh_model_set *set, const mh_model *dst, bool seam, const mhr::Edit *ed, const CodedBatch &a,
           uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_index, uint64_t *d_dropped,
           int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_out_off || (!d_out_nbits && a.n)) return MH_ERR_ARG;
    if (!a.index && !a.sym_off) return MH_ERR_ARG;                    // index-free: the decoded lengths are an output
    if (ed && !ed->map) return MH_ERR_ARG;
    if (!aligned16(d_out_payload)) return MH_ERR_ARG;
    int oshift = 0;                                                   // index-free: the chunk size is the destination index's
    if (!a.index && d_out_index && (oshift = chunk_shift_of(a.chunk_symbols)) < 0) return MH_ERR_ARG;
    mhr::EditParams p{};
    const mhr::RecodeLayout L = mhr::recode_layout(a.n, work_items_of(a), seam);
    const int rc = dev_batch_params(a, SymOff::Through, ctx_of_prev0(m, a.prev0), d_ws, ws_bytes, L.total, L.off_status, d_stream_status, p.s.b);
    if (rc != MH_OK) return rc;
    if (a.index) oshift = int(p.s.b.chunk_shift);
    p.out = d_out_payload; p.cap = d_out_payload ? cap : 0;
    p.out_off = reinterpret_cast<unsigned long long *>(d_out_off);
    p.out_nbits = reinterpret_cast<unsigned long long *>(d_out_nbits);
    p.out_index = reinterpret_cast<unsigned long long *>(d_out_index);
    p.dropped = reinterpret_cast<unsigned long long *>(d_dropped);
    p.out_chunk_shift = uint32_t(oshift);
    if (dst->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    mhb::Model model;
    const int t = source_tables(m, set, p.s, model);
    if (t != MH_OK) return t;
    if (!dst->d_len8 || !dst->d_code64) return MH_ERR_NO_DEVICE;
    p.dst.len8 = dst->d_len8;
    p.dst.code64 = reinterpret_cast<const unsigned long long *>(dst->d_code64);
    p.dst.enc64 = dst->type == 2 ? reinterpret_cast<const unsigned long long *>(dst->d_enc64) : nullptr;
    p.dst.ctx_mask = dst->type == 2 ? 0xFFFFu : (dst->type ? 0xFFu : 0u);
    if (ed) {
        p.ed = *ed;
        HIP_TRY(mhr::launch_recode_edit(p, model, d_ws, static_cast<hipStream_t>(stream)));
    } else {
        HIP_TRY(mhr::launch_recode(p, model, d_ws, static_cast<hipStream_t>(stream)));
    }
    return MH_OK;
}

mhr::Edit edit_of(const uint64_t *d_span_off, const uint64_t *d_spans, const uint8_t *d_map) {
    return mhr::Edit{reinterpret_cast<const unsigned long long *>(d_span_off), reinterpret_cast<const unsigned long long *>(d_spans), d_map, 0u};
}

// the splice of a _splice call as the caller names it
struct SpliceArgs {
    const uint64_t *span_off, *spans;
    const uint8_t *rep;
    uint32_t rep_len;
    uint64_t *out_sym_off;
    uint64_t index_cap;
    uint64_t n_spans;                   // host forms: what the workspace is sized for
    // a _splice_table call: rep / rep_len unused, span r replaced by table entry span_tag[r]
    bool table = false;
    const uint32_t *span_tag = nullptr;
    const uint64_t *rep_off = nullptr;
    const uint8_t *rep_bytes = nullptr;
    size_t n_reps = 0;
};

// what a _splice entry point refuses before anything else: order 2 on either side (m: null under a set), the replacement;
// o2 (the _o2 call): an order-2 source under any destination instead
int splice_args(const mh_model *m, const mh_model_set *set, size_t n, const mh_model *dst, const SpliceArgs &s, bool o2 = false) {
    if (o2) {
        if (!order2(m) || !order012(dst)) return MH_ERR_ARG;
    } else {
        if (set ? n != set->d.n : !order01(m)) return MH_ERR_ARG;
        if (!order01(dst)) return MH_ERR_ARG;
    }
    if (s.rep_len > MH_SPLICE_MAX_REP || (s.rep_len && !s.rep) || !s.span_off || !s.out_sym_off) return MH_ERR_ARG;
    if (s.table && (!s.span_tag || !s.rep_off)) return MH_ERR_ARG;
    return MH_OK;
}

// the workspace of a _splice or _splice_table call
mhr::SpliceLayout splice_layout_of(const SpliceArgs &s, uint64_t n, uint64_t nwork, uint64_t n_spans) {
    return s.table ? mhr::splice_table_layout(n, nwork, n_spans, s.n_reps) : mhr::splice_layout(n, nwork, n_spans);
}

// behind splice_args: recode() with the splice in place of the edit, its own workspace layout and out_sym_off
int splice(const mh_model *m, const mh_model_set *set, const mh_model *dst, const SpliceArgs &s, const CodedBatch &a, uint8_t *d_out_payload,
           size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_index, uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws,
           size_t ws_bytes, void *stream) {
    if (!d_out_off || (!d_out_nbits && a.n)) return MH_ERR_ARG;
    if (!a.index && !a.sym_off) return MH_ERR_ARG;                    // index-free: the decoded lengths are an output
    if (!aligned16(d_out_payload)) return MH_ERR_ARG;
    int oshift = 0;                                                   // index-free: the chunk size is the destination index's
    if (!a.index && d_out_index && (oshift = chunk_shift_of(a.chunk_symbols)) < 0) return MH_ERR_ARG;
    mhr::SpliceTableParams p{};
    const mhr::SpliceLayout L = splice_layout_of(s, a.n, work_items_of(a), 0);
    const int rc = dev_batch_params(a, SymOff::Through, ctx_of_prev0(m, a.prev0), d_ws, ws_bytes, L.total, L.off_status, d_stream_status, p.s.b);
    if (rc != MH_OK) return rc;
    if (a.index) oshift = int(p.s.b.chunk_shift);
    p.out = d_out_payload; p.cap = d_out_payload ? cap : 0;
    p.out_off = reinterpret_cast<unsigned long long *>(d_out_off);
    p.out_nbits = reinterpret_cast<unsigned long long *>(d_out_nbits);
    p.out_index = reinterpret_cast<unsigned long long *>(d_out_index);
    p.dropped = reinterpret_cast<unsigned long long *>(d_dropped);
    p.out_chunk_shift = uint32_t(oshift);
    if (dst->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    mhb::Model model;
    const int t = source_tables(m, set, p.s, model);
    if (t != MH_OK) return t;
    if (!dst->d_len8 || !dst->d_code64) return MH_ERR_NO_DEVICE;
    p.dst.len8 = dst->d_len8;
    p.dst.code64 = reinterpret_cast<const unsigned long long *>(dst->d_code64);
    p.dst.enc64 = dst->type == 2 ? reinterpret_cast<const unsigned long long *>(dst->d_enc64) : nullptr;
    p.dst.ctx_mask = dst->type == 2 ? 0xFFFFu : (dst->type ? 0xFFu : 0u);
    p.sp.span_off = reinterpret_cast<const unsigned long long *>(s.span_off);
    p.sp.spans = reinterpret_cast<const unsigned long long *>(s.spans);
    p.sp.rep = s.rep;
    p.sp.rep_len = s.rep_len;
    p.sp.out_sym_off = reinterpret_cast<unsigned long long *>(s.out_sym_off);
    p.sp.index_cap = s.index_cap;
    if (s.table) {
        p.tb.span_tag = s.span_tag;
        p.tb.rep_off = reinterpret_cast<const unsigned long long *>(s.rep_off);
        p.tb.rep_bytes = s.rep_bytes;
        p.tb.n_reps = s.n_reps;
        HIP_TRY(mhr::launch_recode_splice_table(p, model, d_ws, ws_bytes, static_cast<hipStream_t>(stream)));
        return MH_OK;
    }
    HIP_TRY(mhr::launch_recode_splice(p, model, d_ws, ws_bytes, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

size_t recode_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols, bool seam) {
    const uint64_t W = chunk_shift_of(chunk_symbols) >= 0 ? mhb::work_items(n_streams, sym_total, chunk_symbols) : 0;
    return mhr::recode_layout(n_streams, W, seam).total;
}

// The host forms behind their order rules: the argument checks in the order of mh_decode_batch, then an index-free batch of
// an order-0/1 source with a stream over the walk cap (index_first) is indexed first and re-coded as an indexed batch, with the
// chunk size of out_index when the call writes one; a stream the indexing fails (idx_st) has no symbols, so no payload.  An
// index-free batch is sized for symbol_bound symbols.  always_index (the _o2 editing forms): every index-free batch is indexed
// first, whatever its streams' lengths.
int host_args(const mh_model *src, const mh_model *dst, CodedBatch &a, bool index_first_ok, const uint64_t *out_off, const uint64_t *out_nbits,
              const uint64_t *out_index, uint64_t *sym_off, std::vector<uint64_t> &own_idx, std::vector<int32_t> &idx_st,
              bool always_index = false) {
    if (!out_off || (!out_nbits && a.n) || !sym_off) return MH_ERR_ARG;
    int rc = host_batch_args(a, a.index || out_index);
    if (rc != MH_OK) return rc;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (src->max_len > mh::MAX_CODE_BITS || dst->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    const bool first = always_index ? !a.index && a.n > 0 : over_walk_cap(a);
    if (index_first_ok && first && (rc = index_first(src, a, out_index != nullptr, sym_off, own_idx, idx_st)) != MH_OK) return rc;
    if (!a.index) a.sym_total = symbol_bound(src->min_len, a.nbits, a.n);
    return MH_OK;
}

// One host-form re-code on the device: run() uploads the batch, runs the device call of the family and brings back the
// verdicts, offsets, lengths and dropped counts; payload() and slices() then bring what the device wrote to wherever the
// caller wants it.
struct HostRecode {
    DevBatch db;
    DevBuf d_out, d_oo, d_onb, d_oidx, d_drop, d_st, d_ws, d_oso;
    const SpliceArgs *spl = nullptr;    // a _splice call: spans and rep on the device, out_sym_off the caller's (set before run)
    std::vector<int32_t> sst;           // per-stream verdicts
    std::vector<uint64_t> drop;         // per-stream dropped symbols
    size_t noidx = 0, dcap = 0;         // entries of the destination index, bytes of the payload buffer
    int dev_rc = MH_OK;

    // seam: the _o2 call; ed: the edit of an _edit call, on the device; sym_off: the caller's, written when index-free
    int run(bool seam, const mhr::Edit *ed, const mh_model *src, const mh_model *dst, const CodedBatch &a, uint64_t *sym_off, bool want_payload,
            size_t cap, uint64_t *out_off, uint64_t *out_nbits, const uint64_t *out_index) {
        const hipStream_t st = nullptr;
        const size_t n = a.n;
        noidx = !out_index ? 0 : (spl ? size_t(spl->index_cap) : size_t(mh_batch_index_capacity(a.sym_total, n, a.chunk_symbols)));
        const size_t wsb = spl ? splice_layout_of(*spl, n, work_items_of(a), spl->n_spans).total
                               : recode_workspace(n, a.sym_total, a.index ? a.chunk_symbols : 0, seam);
        dcap = want_payload ? cap : 0;
        HIP_TRY(d_out.alloc(dcap));
        HIP_TRY(d_oo.alloc((n + 1) * 8));
        HIP_TRY(d_onb.alloc(n * 8));
        HIP_TRY(d_oidx.alloc(noidx * 8));
        HIP_TRY(d_drop.alloc(n * 8));
        HIP_TRY(d_st.alloc(n * 4));
        HIP_TRY(d_ws.alloc(wsb));
        if (spl) HIP_TRY(d_oso.alloc((n + 1) * 8));
        int rc = db.upload(a, st);
        if (rc != MH_OK) return rc;
        if (noidx) HIP_TRY(hipMemcpy(d_oidx.p, out_index, noidx * 8, hipMemcpyHostToDevice));   // gap entries stay what the caller had
        if (spl) {
            SpliceArgs d = *spl;
            d.out_sym_off = d_oso.as<uint64_t>();
            rc = splice(src, nullptr, dst, d, db.d, want_payload ? d_out.as<uint8_t>() : nullptr, dcap, d_oo.as<uint64_t>(), d_onb.as<uint64_t>(),
                        out_index ? d_oidx.as<uint64_t>() : nullptr, d_drop.as<uint64_t>(), d_st.as<int32_t>(), d_ws.p, wsb, st);
        } else {
            rc = recode(src, nullptr, dst, seam, ed, db.d, want_payload ? d_out.as<uint8_t>() : nullptr, dcap, d_oo.as<uint64_t>(), d_onb.as<uint64_t>(),
                        out_index ? d_oidx.as<uint64_t>() : nullptr, d_drop.as<uint64_t>(), d_st.as<int32_t>(), d_ws.p, wsb, st);
        }
        if (rc != MH_OK) return rc;
        dev_rc = mh_dev_status(d_ws.p, st);
        sst.resize(n);
        drop.resize(n);
        if (n) HIP_TRY(hipMemcpy(sst.data(), d_st.p, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_off, d_oo.p, (n + 1) * 8, hipMemcpyDeviceToHost));
        if (n) HIP_TRY(hipMemcpy(out_nbits, d_onb.p, n * 8, hipMemcpyDeviceToHost));
        if (n) HIP_TRY(hipMemcpy(drop.data(), d_drop.p, n * 8, hipMemcpyDeviceToHost));
        if (!a.index) HIP_TRY(hipMemcpy(sym_off, db.so.p, (n + 1) * 8, hipMemcpyDeviceToHost));
        if (spl) HIP_TRY(hipMemcpy(spl->out_sym_off, d_oso.p, (n + 1) * 8, hipMemcpyDeviceToHost));
        return MH_OK;
    }

    // the device's payload (`bytes` of it) and index slices; nothing when the payload did not fit
    bool fit() const { return dev_rc != MH_ERR_CAPACITY; }
    int payload(uint8_t *to, uint64_t bytes) {
        if (to && bytes && bytes <= dcap && fit()) HIP_TRY(stage_d2h(to, d_out.p, size_t(bytes), nullptr));
        return MH_OK;
    }
    int slices(uint64_t *to) {
        if (noidx && fit()) HIP_TRY(hipMemcpy(to, d_oidx.p, noidx * 8, hipMemcpyDeviceToHost));
        return MH_OK;
    }

    // the call's result (idx_st: what indexing the batch first found); the device's MH_ERR_CAPACITY: the payload does not fit
    int finish(const std::vector<int32_t> &idx_st, uint64_t *dropped, int32_t *stream_status) {
        if (dropped) std::copy(drop.begin(), drop.end(), dropped);
        const int first = first_failure(sst, idx_st, dev_rc);
        if (stream_status) std::copy(sst.begin(), sst.end(), stream_status);
        return first;
    }
};

// mh_recode_edit_batch and mh_recode_edit_batch_o2 behind their order rules (seam: the _o2 call)
int host_edit(bool seam, const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
              size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, const uint64_t *span_off,
              const uint64_t *spans, const uint8_t *map, uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *out_nbits,
              uint64_t *out_index, uint64_t *dropped, int32_t *stream_status) {
    if (!map) return MH_ERR_ARG;
    if (span_off && (!offsets_ok(span_off, n_streams) || (span_off[n_streams] && !spans))) return MH_ERR_ARG;
    // (a span's positions do not depend on the index that an over-cap batch gets first)
    CodedBatch a{payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols};
    std::vector<uint64_t> own_idx;
    std::vector<int32_t> idx_st;
    int rc = host_args(src, dst, a, true, out_off, out_nbits, out_index, sym_off, own_idx, idx_st, seam);
    if (rc != MH_OK) return rc;
    DevBuf d_soff, d_sp, d_map;
    const size_t nsp = span_off ? size_t(span_off[n_streams]) : 0;
    HIP_TRY(d_soff.alloc(span_off ? (n_streams + 1) * 8 : 0));
    HIP_TRY(d_sp.alloc(nsp * 16));
    HIP_TRY(d_map.alloc(256));
    if (span_off) HIP_TRY(hipMemcpy(d_soff.p, span_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
    if (nsp) HIP_TRY(hipMemcpy(d_sp.p, spans, nsp * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_map.p, map, 256, hipMemcpyHostToDevice));
    const mhr::Edit ed = edit_of(span_off ? d_soff.as<uint64_t>() : nullptr, d_sp.as<uint64_t>(), d_map.as<uint8_t>());
    HostRecode hr;
    rc = hr.run(seam, &ed, src, dst, a, sym_off, out_payload != nullptr, cap, out_off, out_nbits, out_index);
    if (rc != MH_OK) return rc;
    if ((rc = hr.payload(out_payload, out_off[n_streams])) != MH_OK || (rc = hr.slices(out_index)) != MH_OK) return rc;
    return hr.finish(idx_st, dropped, stream_status);
}


// mh_recode_splice_table_batch and mh_recode_splice_table_batch_o2 (o2: that call's order rule)
int host_splice_table(bool o2, const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                      size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, const uint64_t *span_off,
                      const uint64_t *spans, const uint32_t *span_tag, const uint64_t *rep_off, const uint8_t *rep_bytes, size_t n_reps,
                      uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_sym_off, uint64_t *out_index,
                      uint64_t index_cap, uint64_t *dropped, int32_t *stream_status) {
    SpliceArgs s{span_off, spans, nullptr, 0, out_sym_off, out_index ? index_cap : 0, 0, true, span_tag, rep_off, rep_bytes, n_reps};
    int rc = splice_args(src, nullptr, n_streams, dst, s, o2);
    if (rc != MH_OK) return rc;
    if (!offsets_ok(span_off, n_streams) || (span_off[n_streams] && !spans)) return MH_ERR_ARG;
    // the table, as the device checks it, before a device is touched
    if (rep_off[0] != 0 || (span_off[n_streams] && !n_reps)) return MH_ERR_ARG;
    for (size_t k = 0; k < n_reps; ++k)
        if (rep_off[k + 1] < rep_off[k] || rep_off[k + 1] - rep_off[k] > MH_SPLICE_MAX_REP) return MH_ERR_ARG;
    const size_t rep_total = size_t(rep_off[n_reps]);
    if (rep_total && !rep_bytes) return MH_ERR_ARG;
    CodedBatch a{payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols};
    std::vector<uint64_t> own_idx;
    std::vector<int32_t> idx_st;
    rc = host_args(src, dst, a, true, out_off, out_nbits, out_index, sym_off, own_idx, idx_st, o2);
    if (rc != MH_OK) return rc;
    DevBuf d_soff, d_sp, d_tag, d_roff, d_rep;
    s.n_spans = span_off[n_streams];
    HIP_TRY(d_soff.alloc((n_streams + 1) * 8));
    HIP_TRY(d_sp.alloc(size_t(s.n_spans) * 16));
    HIP_TRY(d_tag.alloc(size_t(s.n_spans) * 4 + 4));
    HIP_TRY(d_roff.alloc((n_reps + 1) * 8));
    HIP_TRY(d_rep.alloc(rep_total));
    HIP_TRY(hipMemcpy(d_soff.p, span_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
    if (s.n_spans) HIP_TRY(hipMemcpy(d_sp.p, spans, size_t(s.n_spans) * 16, hipMemcpyHostToDevice));
    if (s.n_spans) HIP_TRY(hipMemcpy(d_tag.p, span_tag, size_t(s.n_spans) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_roff.p, rep_off, (n_reps + 1) * 8, hipMemcpyHostToDevice));
    if (rep_total) HIP_TRY(hipMemcpy(d_rep.p, rep_bytes, rep_total, hipMemcpyHostToDevice));
    s.span_off = d_soff.as<uint64_t>(); s.spans = d_sp.as<uint64_t>(); s.span_tag = d_tag.as<uint32_t>();
    s.rep_off = d_roff.as<uint64_t>(); s.rep_bytes = rep_total ? d_rep.as<uint8_t>() : nullptr;
    HostRecode hr;
    hr.spl = &s;
    rc = hr.run(false, nullptr, src, dst, a, sym_off, out_payload != nullptr, cap, out_off, out_nbits, out_index);
    if (rc != MH_OK) return rc;
    if ((rc = hr.payload(out_payload, out_off[n_streams])) != MH_OK || (rc = hr.slices(out_index)) != MH_OK) return rc;
    return hr.finish(idx_st, dropped, stream_status);
}

}  // namespace

// an index-free order-2 stream over the walk cap, decoded alone
int mhapi::decode_alone(const mh_model *m, const uint8_t *payload, uint64_t nbits, uint8_t prev0, std::vector<uint8_t> &out) {
    const uint64_t minl = uint64_t(m->min_len > 0 ? m->min_len : 1);
    out.assign(size_t(nbits / minl) + 1, 0);
    size_t nb = 0;
    const int rc = mh_decode(m, payload, nbits, prev0, out.data(), out.size(), &nb, nullptr, 0, 0);
    out.resize(rc == MH_OK ? nb : 0);
    return rc;
}

extern "C" {

/* -------------------------------------------------------------------------------------------- coded histogram */

size_t mh_dev_histogram_coded_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    (void)sym_total; (void)chunk_symbols;                             // the counting keeps nothing per chunk
    return mhr::hist_layout(n_streams).total;
}

size_t mh_dev_histogram_coded_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    return mh_dev_histogram_coded_workspace(n_streams, sym_total, chunk_symbols);
}

int mh_dev_histogram_coded_batch(const mh_model *src, int order, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                                 size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                                 const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_counts, int32_t *d_stream_status, void *d_ws,
                                 size_t ws_bytes, void *stream) {
    if (!order01(src) || (order != 0 && order != 1)) return MH_ERR_ARG;
    return histogram_coded(src, nullptr, order,
                           {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols}, d_counts,
                           d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_histogram_coded_each(const mh_model_set *src, int order, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                                size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                                const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_counts, int32_t *d_stream_status, void *d_ws,
                                size_t ws_bytes, void *stream) {
    if (!src || n_streams != src->d.n || (order != 0 && order != 1)) return MH_ERR_ARG;
    return histogram_coded(nullptr, src, order,
                           {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols}, d_counts,
                           d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_histogram_coded_batch_o2(const mh_model *src, int order, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                                    size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                                    const uint64_t *d_index, uint32_t chunk_symbols, uint64_t *d_counts, int32_t *d_stream_status, void *d_ws,
                                    size_t ws_bytes, void *stream) {
    if (!order012(src) || order < 0 || order > 2 || (src->type != 2 && order != 2)) return MH_ERR_ARG;
    return histogram_coded(src, nullptr, order,
                           {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols}, d_counts,
                           d_stream_status, d_ws, ws_bytes, stream);
}

/* ---------------------------------------------------------------------------------------------------- re-code */

size_t mh_dev_recode_batch_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    return recode_workspace(n_streams, sym_total, chunk_symbols, false);
}

size_t mh_dev_recode_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    return recode_workspace(n_streams, sym_total, chunk_symbols, true);
}

int mh_dev_recode_batch(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                        size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                        uint32_t chunk_symbols, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits,
                        uint64_t *d_out_index, uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order01(src) || !order01(dst)) return MH_ERR_ARG;
    return recode(src, nullptr, dst, false, nullptr, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_recode_each(const mh_model_set *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                       size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                       uint32_t chunk_symbols, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits,
                       uint64_t *d_out_index, uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!src || n_streams != src->d.n || !order01(dst)) return MH_ERR_ARG;
    return recode(nullptr, src, dst, false, nullptr, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_recode_batch_o2(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                           size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                           uint32_t chunk_symbols, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits,
                           uint64_t *d_out_index, uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order012(src) || !order012(dst) || (src->type != 2 && dst->type != 2)) return MH_ERR_ARG;
    return recode(src, nullptr, dst, true, nullptr, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_recode_batch(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                    size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint8_t *out_payload,
                    size_t cap, uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_index, uint64_t *dropped, int32_t *stream_status) {
    if (!order01(src) || !order01(dst)) return MH_ERR_ARG;
    CodedBatch a{payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols};
    std::vector<uint64_t> own_idx;
    std::vector<int32_t> idx_st;
    int rc = host_args(src, dst, a, true, out_off, out_nbits, out_index, sym_off, own_idx, idx_st);
    if (rc != MH_OK) return rc;
    HostRecode hr;
    rc = hr.run(false, nullptr, src, dst, a, sym_off, out_payload != nullptr, cap, out_off, out_nbits, out_index);
    if (rc != MH_OK) return rc;
    if ((rc = hr.payload(out_payload, out_off[n_streams])) != MH_OK || (rc = hr.slices(out_index)) != MH_OK) return rc;
    return hr.finish(idx_st, dropped, stream_status);
}

/* ------------------------------------------------------------------------------------------------------- edit */

int mh_spans_from_hits(const uint64_t *hit_off, const uint64_t *hits, uint64_t hit_cap, size_t n_streams, uint64_t *span_off, uint64_t *spans) {
    if (!hit_off || !span_off) return MH_ERR_ARG;
    std::fill(span_off, span_off + n_streams + 1, uint64_t(0));
    const uint64_t total = hit_off[n_streams];
    if (total > hit_cap) return MH_ERR_CAPACITY;
    if (total && (!hits || !spans)) return MH_ERR_ARG;
    if (!offsets_ok(hit_off, n_streams)) return MH_ERR_ARG;
    uint64_t ns = 0;
    std::vector<uint64_t> least;
    for (size_t i = 0; i < n_streams; ++i) {
        span_off[i] = ns;
        const uint64_t a = hit_off[i], k = hit_off[i + 1] - a;
        if (!k) continue;
        const uint64_t *h = hits + 3 * a;
        least.resize(size_t(k));                                       // least[r]: the least begin of the records r' >= r
        uint64_t m = ~uint64_t(0);
        for (uint64_t r = k; r-- > 0;) least[size_t(r)] = m = std::min(m, h[3 * r + 1]);
        for (uint64_t r = 0; r < k; ++r) {
            if (r == 0 || h[3 * (r - 1) + 2] < least[size_t(r)]) spans[2 * ns++] = least[size_t(r)];
            spans[2 * (ns - 1) + 1] = h[3 * r + 2];
        }
    }
    span_off[n_streams] = ns;
    return MH_OK;
}

size_t mh_dev_spans_from_hits_workspace(size_t n_streams, uint64_t hit_cap) {
    (void)n_streams;                                                  // per stream: only the offsets the caller passes
    return mhr::span_layout(hit_cap).total;
}

int mh_dev_spans_from_hits(const uint64_t *d_hit_off, const uint64_t *d_hits, uint64_t hit_cap, size_t n_streams, uint64_t *d_span_off,
                           uint64_t *d_spans, void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_hit_off || !d_span_off || !d_ws || (hit_cap && (!d_hits || !d_spans)) || !aligned16(d_ws)) return MH_ERR_ARG;
    if (hit_cap >= (uint64_t(1) << 40)) return MH_ERR_ARG;
    if (ws_bytes < mhr::span_layout(hit_cap).total) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    HIP_TRY(mhr::launch_spans_from_hits(reinterpret_cast<const unsigned long long *>(d_hit_off), reinterpret_cast<const unsigned long long *>(d_hits),
                                        hit_cap, n_streams, reinterpret_cast<unsigned long long *>(d_span_off),
                                        reinterpret_cast<unsigned long long *>(d_spans), d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

int mh_spans_from_hits_tagged(const uint64_t *hit_off, const uint64_t *hits, const uint32_t *hit_pattern, uint64_t hit_cap, size_t n_streams,
                              uint64_t *span_off, uint64_t *spans, uint32_t *span_tag) {
    if (!hit_pattern) return MH_ERR_ARG;
    const int rc = mh_spans_from_hits(hit_off, hits, hit_cap, n_streams, span_off, spans);
    if (rc != MH_OK) return rc;
    if (span_off[n_streams] && !span_tag) return MH_ERR_ARG;
    // span q of stream i holds the records whose end lies in (end(q - 1), end(q)]: records ascend by end
    for (size_t i = 0; i < n_streams; ++i) {
        uint64_t r = hit_off[i];
        for (uint64_t q = span_off[i]; q < span_off[i + 1]; ++q) {
            uint32_t t = ~uint32_t(0);
            for (; r < hit_off[i + 1] && hits[3 * r + 2] <= spans[2 * q + 1]; ++r) t = std::min(t, hit_pattern[r]);
            span_tag[q] = t;
        }
    }
    return MH_OK;
}

size_t mh_dev_spans_from_hits_tagged_workspace(size_t n_streams, uint64_t hit_cap) { return mh_dev_spans_from_hits_workspace(n_streams, hit_cap); }

int mh_dev_spans_from_hits_tagged(const uint64_t *d_hit_off, const uint64_t *d_hits, const uint32_t *d_hit_pattern, uint64_t hit_cap,
                                  size_t n_streams, uint64_t *d_span_off, uint64_t *d_spans, uint32_t *d_span_tag, void *d_ws, size_t ws_bytes,
                                  void *stream) {
    if (!d_hit_pattern || (hit_cap && !d_span_tag)) return MH_ERR_ARG;
    if (!d_hit_off || !d_span_off || !d_ws || (hit_cap && (!d_hits || !d_spans)) || !aligned16(d_ws)) return MH_ERR_ARG;
    if (hit_cap >= (uint64_t(1) << 40)) return MH_ERR_ARG;
    if (ws_bytes < mhr::span_layout(hit_cap).total) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    HIP_TRY(mhr::launch_spans_from_hits_tagged(reinterpret_cast<const unsigned long long *>(d_hit_off),
                                               reinterpret_cast<const unsigned long long *>(d_hits), d_hit_pattern, hit_cap, n_streams,
                                               reinterpret_cast<unsigned long long *>(d_span_off), reinterpret_cast<unsigned long long *>(d_spans),
                                               d_span_tag, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

size_t mh_dev_recode_edit_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    return recode_workspace(n_streams, sym_total, chunk_symbols, false);
}

int mh_dev_recode_edit_batch(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                             size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                             uint32_t chunk_symbols, const uint64_t *d_span_off, const uint64_t *d_spans, const uint8_t *d_map,
                             uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_index,
                             uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!order01(src) || !order01(dst)) return MH_ERR_ARG;
    const mhr::Edit ed = edit_of(d_span_off, d_spans, d_map);
    return recode(src, nullptr, dst, false, &ed, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_recode_edit_each(const mh_model_set *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                            size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                            uint32_t chunk_symbols, const uint64_t *d_span_off, const uint64_t *d_spans, const uint8_t *d_map,
                            uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_index,
                            uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!src || n_streams != src->d.n || !order01(dst)) return MH_ERR_ARG;
    const mhr::Edit ed = edit_of(d_span_off, d_spans, d_map);
    return recode(nullptr, src, dst, false, &ed, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_recode_edit_batch(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                         size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                         const uint64_t *span_off, const uint64_t *spans, const uint8_t *map, uint8_t *out_payload, size_t cap, uint64_t *out_off,
                         uint64_t *out_nbits, uint64_t *out_index, uint64_t *dropped, int32_t *stream_status) {
    if (!order01(src) || !order01(dst)) return MH_ERR_ARG;
    return host_edit(false, src, dst, payload, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols, span_off, spans, map, out_payload, cap,
                     out_off, out_nbits, out_index, dropped, stream_status);
}

/* ----------------------------------------------------------------------------------------------------- splice */

size_t mh_dev_recode_splice_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols, uint64_t n_spans) {
    const uint64_t W = chunk_shift_of(chunk_symbols) >= 0 ? mhb::work_items(n_streams, sym_total, chunk_symbols) : 0;
    return mhr::splice_layout(n_streams, W, n_spans).total;
}

int mh_dev_recode_splice_batch(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                               size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                               uint32_t chunk_symbols, const uint64_t *d_span_off, const uint64_t *d_spans, const uint8_t *d_rep, uint32_t rep_len,
                               uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_sym_off,
                               uint64_t *d_out_index, uint64_t index_cap, uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
                               void *stream) {
    const SpliceArgs s{d_span_off, d_spans, d_rep, rep_len, d_out_sym_off, index_cap, 0};
    const int rc = splice_args(src, nullptr, n_streams, dst, s);
    if (rc != MH_OK) return rc;
    return splice(src, nullptr, dst, s, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_recode_splice_each(const mh_model_set *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                              size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                              uint32_t chunk_symbols, const uint64_t *d_span_off, const uint64_t *d_spans, const uint8_t *d_rep, uint32_t rep_len,
                              uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_sym_off,
                              uint64_t *d_out_index, uint64_t index_cap, uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes,
                              void *stream) {
    if (!src) return MH_ERR_ARG;
    const SpliceArgs s{d_span_off, d_spans, d_rep, rep_len, d_out_sym_off, index_cap, 0};
    const int rc = splice_args(nullptr, src, n_streams, dst, s);
    if (rc != MH_OK) return rc;
    return splice(nullptr, src, dst, s, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_recode_splice_batch(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                           size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                           const uint64_t *span_off, const uint64_t *spans, const uint8_t *rep, uint32_t rep_len, uint8_t *out_payload, size_t cap,
                           uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_sym_off, uint64_t *out_index, uint64_t index_cap, uint64_t *dropped,
                           int32_t *stream_status) {
    SpliceArgs s{span_off, spans, rep, rep_len, out_sym_off, out_index ? index_cap : 0, 0};
    int rc = splice_args(src, nullptr, n_streams, dst, s);
    if (rc != MH_OK) return rc;
    if (!offsets_ok(span_off, n_streams) || (span_off[n_streams] && !spans)) return MH_ERR_ARG;
    // (a span's positions do not depend on the index that an over-cap batch gets first)
    CodedBatch a{payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols};
    std::vector<uint64_t> own_idx;
    std::vector<int32_t> idx_st;
    rc = host_args(src, dst, a, true, out_off, out_nbits, out_index, sym_off, own_idx, idx_st);
    if (rc != MH_OK) return rc;
    DevBuf d_soff, d_sp, d_rep;
    s.n_spans = span_off[n_streams];
    HIP_TRY(d_soff.alloc((n_streams + 1) * 8));
    HIP_TRY(d_sp.alloc(size_t(s.n_spans) * 16));
    HIP_TRY(d_rep.alloc(rep_len));
    HIP_TRY(hipMemcpy(d_soff.p, span_off, (n_streams + 1) * 8, hipMemcpyHostToDevice));
    if (s.n_spans) HIP_TRY(hipMemcpy(d_sp.p, spans, size_t(s.n_spans) * 16, hipMemcpyHostToDevice));
    if (rep_len) HIP_TRY(hipMemcpy(d_rep.p, rep, rep_len, hipMemcpyHostToDevice));
    s.span_off = d_soff.as<uint64_t>(); s.spans = d_sp.as<uint64_t>(); s.rep = rep_len ? d_rep.as<uint8_t>() : nullptr;
    HostRecode hr;
    hr.spl = &s;
    rc = hr.run(false, nullptr, src, dst, a, sym_off, out_payload != nullptr, cap, out_off, out_nbits, out_index);
    if (rc != MH_OK) return rc;
    if ((rc = hr.payload(out_payload, out_off[n_streams])) != MH_OK || (rc = hr.slices(out_index)) != MH_OK) return rc;
    return hr.finish(idx_st, dropped, stream_status);
}

/* ----------------------------------------------------------------------------------------------- table splice */

size_t mh_dev_recode_splice_table_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols, uint64_t n_spans, size_t n_reps) {
    const uint64_t W = chunk_shift_of(chunk_symbols) >= 0 ? mhb::work_items(n_streams, sym_total, chunk_symbols) : 0;
    return mhr::splice_table_layout(n_streams, W, n_spans, n_reps).total;
}

int mh_dev_recode_splice_table_batch(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
                                     const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off,
                                     uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, const uint64_t *d_span_off,
                                     const uint64_t *d_spans, const uint32_t *d_span_tag, const uint64_t *d_rep_off, const uint8_t *d_rep_bytes,
                                     size_t n_reps, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits,
                                     uint64_t *d_out_sym_off, uint64_t *d_out_index, uint64_t index_cap, uint64_t *d_dropped,
                                     int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    const SpliceArgs s{d_span_off, d_spans, nullptr, 0, d_out_sym_off, index_cap, 0, true, d_span_tag, d_rep_off, d_rep_bytes, n_reps};
    const int rc = splice_args(src, nullptr, n_streams, dst, s);
    if (rc != MH_OK) return rc;
    return splice(src, nullptr, dst, s, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_dev_recode_splice_table_each(const mh_model_set *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
                                    const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off,
                                    uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, const uint64_t *d_span_off,
                                    const uint64_t *d_spans, const uint32_t *d_span_tag, const uint64_t *d_rep_off, const uint8_t *d_rep_bytes,
                                    size_t n_reps, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits,
                                    uint64_t *d_out_sym_off, uint64_t *d_out_index, uint64_t index_cap, uint64_t *d_dropped,
                                    int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream) {
    if (!src) return MH_ERR_ARG;
    const SpliceArgs s{d_span_off, d_spans, nullptr, 0, d_out_sym_off, index_cap, 0, true, d_span_tag, d_rep_off, d_rep_bytes, n_reps};
    const int rc = splice_args(nullptr, src, n_streams, dst, s);
    if (rc != MH_OK) return rc;
    return splice(nullptr, src, dst, s, {d_payload, d_pay_off, d_nbits, n_streams, pay_total, prev0, d_sym_off, sym_total, d_index, chunk_symbols},
                  d_out_payload, cap, d_out_off, d_out_nbits, d_out_index, d_dropped, d_stream_status, d_ws, ws_bytes, stream);
}

int mh_recode_splice_table_batch(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                                 size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                                 const uint64_t *span_off, const uint64_t *spans, const uint32_t *span_tag, const uint64_t *rep_off,
                                 const uint8_t *rep_bytes, size_t n_reps, uint8_t *out_payload, size_t cap, uint64_t *out_off,
                                 uint64_t *out_nbits, uint64_t *out_sym_off, uint64_t *out_index, uint64_t index_cap, uint64_t *dropped,
                                 int32_t *stream_status) {
    return host_splice_table(false, src, dst, payload, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols, span_off, spans, span_tag,
                             rep_off, rep_bytes, n_reps, out_payload, cap, out_off, out_nbits, out_sym_off, out_index, index_cap, dropped,
                             stream_status);
}

int mh_recode_batch_o2(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                       size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint8_t *out_payload,
                       size_t cap, uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_index, uint64_t *dropped, int32_t *stream_status) {
    if (!order012(src) || !order012(dst) || (src->type != 2 && dst->type != 2)) return MH_ERR_ARG;
    // index-free with a stream over the walk cap.  Order-0/1 source: index first.  Order-2 source (not yet on mh_index_batch_o2): the
    // device call refuses such a stream; it is decoded alone, coded by mh_encode under dst and spliced into place in stream order.
    CodedBatch a{payload, pay_off, nbits, n_streams, 0, prev0, sym_off, 0, index, chunk_symbols};
    std::vector<uint64_t> own_idx;
    std::vector<int32_t> idx_st;
    int rc = host_args(src, dst, a, src->type != 2, out_off, out_nbits, out_index, sym_off, own_idx, idx_st);
    if (rc != MH_OK) return rc;
    std::vector<size_t> long_streams;
    if (!a.index)
        for (size_t i = 0; i < n_streams; ++i)
            if (nbits[i] > MH_BATCH_WALK_MAX_BITS) long_streams.push_back(i);
    HostRecode hr;
    rc = hr.run(true, nullptr, src, dst, a, sym_off, out_payload != nullptr, cap, out_off, out_nbits, out_index);
    if (rc != MH_OK) return rc;
    if (long_streams.empty()) {
        if ((rc = hr.payload(out_payload, out_off[n_streams])) != MH_OK || (rc = hr.slices(out_index)) != MH_OK) return rc;
    } else {
        // the device's part, then every stream moved to its place behind the long streams' payloads, symbols and slices
        const bool dev_fit = hr.dev_rc != MH_ERR_CAPACITY;
        std::vector<uint8_t> dev_out(out_payload && dev_fit ? size_t(out_off[n_streams]) : 0);
        if (!dev_out.empty()) HIP_TRY(stage_d2h(dev_out.data(), hr.d_out.p, dev_out.size(), nullptr));
        std::vector<uint64_t> dev_idx(dev_fit ? hr.noidx : 0);
        if (!dev_idx.empty()) HIP_TRY(hipMemcpy(dev_idx.data(), hr.d_oidx.p, hr.noidx * 8, hipMemcpyDeviceToHost));
        // dst's code lengths, for the dropped symbols of the long streams
        const uint32_t dmask = dst->type == 2 ? 0xFFFFu : (dst->type ? 0xFFu : 0u);
        std::vector<uint8_t> len8((size_t(dmask) + 1) << 8);
        if (!dst->d_len8) return MH_ERR_NO_DEVICE;
        HIP_TRY(hipMemcpy(len8.data(), dst->d_len8, len8.size(), hipMemcpyDeviceToHost));
        const std::vector<uint64_t> dso(sym_off, sym_off + n_streams + 1), doo(out_off, out_off + n_streams + 1);
        std::vector<uint8_t> bytes, coded;
        std::vector<uint64_t> slice;
        uint64_t pos = 0, sym = 0;
        size_t k = 0;
        bool fits = dev_fit;
        for (size_t i = 0; i < n_streams; ++i) {
            const bool is_long = k < long_streams.size() && long_streams[k] == i;
            uint64_t len = doo[i + 1] - doo[i], cnt = dso[i + 1] - dso[i];
            const uint8_t *from = dev_out.empty() ? nullptr : dev_out.data() + doo[i];
            const uint64_t *ifrom = dev_idx.empty() ? nullptr : dev_idx.data() + mh_batch_index_base(dso[i], i, chunk_symbols ? chunk_symbols : 1);
            if (is_long) {
                ++k;
                len = cnt = 0;
                hr.sst[i] = decode_alone(src, payload + pay_off[i], nbits[i], prev0, bytes);
                if (hr.sst[i] == MH_OK) {
                    coded.assign(mh_encode_bound(dst, bytes.size()) + 16, 0);
                    slice.assign(out_index ? size_t(mh_index_entries(bytes.size(), chunk_symbols)) : 0, 0);
                    uint64_t nb = 0;
                    const int er = mh_encode(dst, bytes.data(), bytes.size(), prev0, coded.data(), coded.size(), &nb,
                                             out_index ? slice.data() : nullptr, out_index ? chunk_symbols : 0);
                    if (er != MH_OK) return er;
                    out_nbits[i] = nb;
                    len = (nb + 7) / 8; cnt = bytes.size();
                    from = coded.data(); ifrom = slice.data();
                    uint32_t c16 = uint32_t(prev0) * 0x101u;
                    uint64_t d = 0;
                    for (uint8_t b : bytes) {
                        const uint8_t l = len8[(size_t(c16 & dmask) << 8) | b];
                        d += l == 0 || l > 64;
                        c16 = ((c16 << 8) | b) & 0xFFFFu;
                    }
                    hr.drop[i] = d;
                }
            }
            out_off[i] = pos;
            sym_off[i] = sym;
            if (out_payload && len) {
                if (pos + len > cap || !from) fits = false;
                else std::memcpy(out_payload + pos, from, size_t(len));
            }
            if (out_index && cnt && ifrom && fits) {
                const uint64_t ne = mh_index_entries(cnt, chunk_symbols);
                std::memcpy(out_index + mh_batch_index_base(sym, i, chunk_symbols), ifrom, size_t(ne) * 8);
            }
            pos += len;
            sym += cnt;
        }
        out_off[n_streams] = pos;
        sym_off[n_streams] = sym;
        hr.dev_rc = (out_payload && !fits) ? MH_ERR_CAPACITY : MH_OK;
    }
    return hr.finish(idx_st, dropped, stream_status);
}

/* ------------------------------------------------------------------------ order 2 in editing and splicing */

// the seam's arrays, as recode_layout(…, seam) lays them out: 8 bytes per chunk number more than the order-0/1 call
size_t mh_dev_recode_edit_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    return recode_workspace(n_streams, sym_total, chunk_symbols, true);
}

// nothing new per span or per chunk: the table splice's
size_t mh_dev_recode_splice_table_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols, uint64_t n_spans, size_t n_reps) {
    return mh_dev_recode_splice_table_workspace(n_streams, sym_total, chunk_symbols, n_spans, n_reps);
}

static CodedBatch batch_of(const mh_coded_batch_args &b) {
    return {b.d_payload, b.d_pay_off, b.d_nbits, b.n_streams, b.pay_total, b.prev0, b.d_sym_off, b.sym_total, b.d_index, b.chunk_symbols};
}

int mh_dev_recode_edit_batch_o2(const mh_recode_edit_o2_args *a) {
    if (!a || a->struct_size != sizeof(*a)) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;                      // (an order-2 model exists on a device alone)
    if (!order012(a->src) || !order012(a->dst) || (a->src->type != 2 && a->dst->type != 2)) return MH_ERR_ARG;
    const mhr::Edit ed = edit_of(a->d_span_off, a->d_spans, a->d_map);
    return recode(a->src, nullptr, a->dst, true, &ed, batch_of(a->batch), a->d_out_payload, a->cap, a->d_out_off, a->d_out_nbits, a->d_out_index,
                  a->d_dropped, a->d_stream_status, a->d_ws, a->ws_bytes, a->stream);
}

int mh_dev_recode_splice_table_batch_o2(const mh_recode_splice_o2_args *a) {
    if (!a || a->struct_size != sizeof(*a)) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;                      // (an order-2 model exists on a device alone)
    const SpliceArgs s{a->d_span_off, a->d_spans, nullptr, 0, a->d_out_sym_off, a->index_cap, 0, true, a->d_span_tag, a->d_rep_off, a->d_rep_bytes,
                       a->n_reps};
    const int rc = splice_args(a->src, nullptr, a->batch.n_streams, a->dst, s, true);
    if (rc != MH_OK) return rc;
    return splice(a->src, nullptr, a->dst, s, batch_of(a->batch), a->d_out_payload, a->cap, a->d_out_off, a->d_out_nbits, a->d_out_index, a->d_dropped,
                  a->d_stream_status, a->d_ws, a->ws_bytes, a->stream);
}

int mh_recode_edit_batch_o2(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                            size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                            const uint64_t *span_off, const uint64_t *spans, const uint8_t *map, uint8_t *out_payload, size_t cap,
                            uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_index, uint64_t *dropped, int32_t *stream_status) {
    if (!order012(src) || !order012(dst) || (src->type != 2 && dst->type != 2)) return MH_ERR_ARG;
    return host_edit(true, src, dst, payload, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols, span_off, spans, map, out_payload, cap,
                     out_off, out_nbits, out_index, dropped, stream_status);
}

int mh_recode_splice_table_batch_o2(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off,
                                    const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index,
                                    uint32_t chunk_symbols, const uint64_t *span_off, const uint64_t *spans, const uint32_t *span_tag,
                                    const uint64_t *rep_off, const uint8_t *rep_bytes, size_t n_reps, uint8_t *out_payload, size_t cap,
                                    uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_sym_off, uint64_t *out_index, uint64_t index_cap,
                                    uint64_t *dropped, int32_t *stream_status) {
    return host_splice_table(true, src, dst, payload, pay_off, nbits, n_streams, prev0, sym_off, index, chunk_symbols, span_off, spans, span_tag,
                             rep_off, rep_bytes, n_reps, out_payload, cap, out_off, out_nbits, out_sym_off, out_index, index_cap, dropped,
                             stream_status);
}

}  // extern "C"
