// mh_api_reader.hpp — what every call that READS a compressed batch does with the batch, written once for the mh_api_*.cpp
// files (host code only: no kernel file includes this): the ten arguments as one struct, the argument checks of the device
// calls and of the host forms, the upload, indexing an over-cap batch first, the call's verdict and the splice of streams
// decoded alone.  What a family does differently is a parameter here or stays in its own file ("One
// compressed-batch reader on the host side").
#pragma once
#include "mh_api_internal.hpp"
#include "mh_batch.h"

namespace mhapi {

// The compressed batch of a call: device pointers in a device call, the caller's buffers in a host form (which reads
// pay_total and sym_total from the offsets once host_batch_args has passed).
struct CodedBatch {
    const uint8_t *payload;
    const uint64_t *pay_off, *nbits;
    size_t n;
    uint64_t pay_total;
    uint8_t prev0;
    const uint64_t *sym_off;
    uint64_t sym_total;
    const uint64_t *index;
    uint32_t chunk_symbols;
};

// ---------------------------------------------------------------------------------------------------- device calls

// the pointers every device call reads the batch through, the segment-state calls included
inline bool dev_batch_ptrs_ok(const uint8_t *d_payload, uint64_t pay_total, const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n,
                              const void *d_ws) {
    if ((!d_payload && pay_total) || !d_pay_off || (!d_nbits && n) || !d_ws) return false;
    return aligned16(d_payload) && aligned16(d_ws);
}

// an index needs a valid chunk size and sym_off; shift: log2 of the chunk size, 0 without an index
inline bool index_args_ok(const uint64_t *index, uint32_t chunk_symbols, const uint64_t *sym_off, int &shift) {
    shift = 0;
    return !index || ((shift = chunk_shift_of(chunk_symbols)) >= 0 && sym_off);
}

// the work items of an indexed batch as the workspace layouts count them (0: index-free, or a chunk size the checks refuse)
inline uint64_t work_items_of(const CodedBatch &a) {
    return a.index && chunk_shift_of(a.chunk_symbols) >= 0 ? mhb::work_items(a.n, a.sym_total, a.chunk_symbols) : 0;
}

// what an index-free call hands the kernels as sym_off / sym_total
enum class SymOff {
    UnderIndex,   // search, digests: read under an index only, null and 0 without one
    Through       // decode, re-coding: an index-free call writes the decoded lengths there
};

// The checks all device calls share, in the order of mh_dev_decode_batch (pointers and alignment, the index, then the
// workspace: ws_need bytes), and the batch part of the kernels' parameters.  The caller's own null tests come before this
// call, its capacity tests after.  The per-stream statuses go to the caller's array or the workspace's slot at off_status.
inline int dev_batch_params(const CodedBatch &a, SymOff so, uint32_t ctx0, void *d_ws, size_t ws_bytes, size_t ws_need, size_t off_status,
                            int32_t *d_stream_status, mhb::DecBatchParams &b) {
    int shift;
    if (!dev_batch_ptrs_ok(a.payload, a.pay_total, a.pay_off, a.nbits, a.n, d_ws) || !index_args_ok(a.index, a.chunk_symbols, a.sym_off, shift))
        return MH_ERR_ARG;
    if (ws_bytes < ws_need) return MH_ERR_CAPACITY;
    const bool keep = a.index || so == SymOff::Through;
    b.payload = a.payload; b.pay_off = a.pay_off; b.nbits = a.nbits; b.n = a.n; b.pay_total = a.pay_total; b.prev0 = ctx0;
    b.sym_off = keep ? reinterpret_cast<unsigned long long *>(const_cast<uint64_t *>(a.sym_off)) : nullptr;   // (read only under an index)
    b.sym_total = keep ? a.sym_total : 0;
    b.index = a.index; b.chunk_shift = uint32_t(shift);
    b.walk_max_bits = MH_BATCH_WALK_MAX_BITS;
    b.stream_status = d_stream_status ? d_stream_status : ws_status(d_ws, off_status);
    return MH_OK;
}

// ------------------------------------------------------------------------------------------------------ host forms

// The checks all host forms share, in the order of mh_decode_batch: pointers, the chunk size (chunked: the call reads or
// writes an index), the offsets, a missing payload, every nbits against its bytes, sym_off under an index.  Fills pay_total
// and sym_total.  The caller's own null tests come before this call; its capacity test, have_device and the code-length
// test after, in the caller's order.
inline int host_batch_args(CodedBatch &a, bool chunked) {
    if (!a.pay_off || (!a.nbits && a.n) || (a.index && !a.sym_off)) return MH_ERR_ARG;
    if (chunked && chunk_shift_of(a.chunk_symbols) < 0) return MH_ERR_ARG;
    if (!offsets_ok(a.pay_off, a.n)) return MH_ERR_ARG;
    if (!a.payload && a.pay_off[a.n]) return MH_ERR_ARG;
    for (size_t i = 0; i < a.n; ++i)
        if (a.nbits[i] > (a.pay_off[i + 1] - a.pay_off[i]) * 8) return MH_ERR_ARG;
    if (a.index && !offsets_ok(a.sym_off, a.n)) return MH_ERR_ARG;
    a.pay_total = a.pay_off[a.n];
    a.sym_total = a.index ? a.sym_off[a.n] : 0;
    return MH_OK;
}

// A host form's batch on the device.  `a` may be a sub-range of the caller's batch with offsets re-based to it.  sym_off and
// the index go up only when there is an index; so always has room for the n + 1 offsets an index-free call writes.
struct DevBatch {
    DevBuf pl, po, nb, so, idx;
    size_t nidx = 0;                    // entries of the index
    CodedBatch d{};                     // the device view: what the device call of the family takes

    int upload(const CodedBatch &a, hipStream_t st) {
        nidx = a.index ? size_t(mh_batch_index_capacity(a.sym_total, a.n, a.chunk_symbols)) : 0;
        HIP_TRY(pl.alloc(size_t(a.pay_total) + 64));
        HIP_TRY(po.alloc((a.n + 1) * 8));
        HIP_TRY(nb.alloc(a.n * 8));
        HIP_TRY(so.alloc((a.n + 1) * 8));
        if (a.index) HIP_TRY(idx.alloc(nidx * 8));
        if (a.pay_total) HIP_TRY(stage_h2d(pl.p, a.payload, size_t(a.pay_total), st));
        HIP_TRY(hipMemcpy(po.p, a.pay_off, (a.n + 1) * 8, hipMemcpyHostToDevice));
        if (a.n) HIP_TRY(hipMemcpy(nb.p, a.nbits, a.n * 8, hipMemcpyHostToDevice));
        if (a.index) {
            HIP_TRY(hipMemcpy(so.p, a.sym_off, (a.n + 1) * 8, hipMemcpyHostToDevice));
            if (nidx) HIP_TRY(hipMemcpy(idx.p, a.index, nidx * 8, hipMemcpyHostToDevice));
        }
        d = a;
        d.payload = pl.as<uint8_t>(); d.pay_off = po.as<uint64_t>(); d.nbits = nb.as<uint64_t>();
        d.sym_off = so.as<uint64_t>(); d.index = a.index ? idx.as<uint64_t>() : nullptr;
        return MH_OK;
    }
};

// at most this many symbols in the batch: what an index-free call sizes its output and a new index for
inline uint64_t symbol_bound(int min_len, const uint64_t *nbits, size_t n) {
    const uint64_t minl = uint64_t(min_len > 0 ? min_len : 1);
    uint64_t bound = 0;
    for (size_t i = 0; i < n; ++i) bound += nbits[i] / minl;
    return bound;
}

// an index-free batch with a stream over the walk cap, which the device calls refuse
inline bool over_walk_cap(const CodedBatch &a) {
    if (a.index) return false;
    for (size_t i = 0; i < a.n; ++i)
        if (a.nbits[i] > MH_BATCH_WALK_MAX_BITS) return true;
    return false;
}

// Such a batch is indexed first (mh_index_batch / mh_index_batch_o2 never refuse a valid stream) and read as an indexed
// batch: `a` then has the new index (own_idx) over sym_off, which the indexing writes (n + 1 entries; re-coding passes the
// caller's array, whose output it is).  A stream the indexing fails keeps that error (idx_st) and has no symbols.
// keep_chunk: the caller's chunk size is that of an index the call writes, so the new index has it too.
inline int index_first(const mh_model *m, CodedBatch &a, bool keep_chunk, uint64_t *sym_off, std::vector<uint64_t> &own_idx,
                       std::vector<int32_t> &idx_st) {
    if (!keep_chunk) a.chunk_symbols = MH_CHUNK_DEFAULT;
    own_idx.assign(size_t(mh_batch_index_capacity(symbol_bound(m->min_len, a.nbits, a.n), a.n, a.chunk_symbols)), 0);
    idx_st.assign(a.n, MH_OK);
    const int rc = (order2(m) ? mh_index_batch_o2 : mh_index_batch)(m, a.payload, a.pay_off, a.nbits, a.n, a.prev0, a.chunk_symbols, sym_off,
                                                                    own_idx.data(), own_idx.size(), idx_st.data());
    if (rc == MH_ERR_HIP || rc == MH_ERR_NO_DEVICE || rc == MH_ERR_NOMEM || rc == MH_ERR_CAPACITY) return rc;
    a.sym_off = sym_off;
    a.sym_total = sym_off[a.n];
    a.index = own_idx.data();
    return MH_OK;
}

// The call's verdict: the first failed stream's error, else the device's (unless that is the kernels' MH_ERR_ARG, which
// the stream's own status carries).  idx_st: what indexing the batch first found; it overrides the stream's status.
inline int first_failure(std::vector<int32_t> &sst, const std::vector<int32_t> &idx_st, int dev_rc) {
    for (size_t i = 0; i < idx_st.size(); ++i)
        if (idx_st[i] != MH_OK) sst[i] = idx_st[i];
    int first = MH_OK;
    for (size_t i = 0; i < sst.size() && first == MH_OK; ++i) first = sst[i];
    if (first == MH_OK && dev_rc != MH_OK && dev_rc != MH_ERR_ARG) first = dev_rc;
    return first;
}

// Streams decoded alone (alone: their numbers, ascending; extra: their bytes) go back between the device's (d_out, laid out
// by dso) in stream order; sym_off gets the true offsets.  What does not fit is counted, not written: MH_ERR_CAPACITY
// unless a stream failed before (first).
inline int splice_alone(const std::vector<uint64_t> &dso, const void *d_out, const std::vector<size_t> &alone,
                        const std::vector<std::vector<uint8_t>> &extra, uint8_t *out, size_t out_cap, uint64_t *sym_off, int first,
                        hipStream_t st) {
    const size_t n = dso.size() - 1;
    std::vector<uint8_t> dev_bytes(static_cast<size_t>(dso[n]));
    if (!dev_bytes.empty()) HIP_TRY(stage_d2h(dev_bytes.data(), d_out, dev_bytes.size(), st));
    uint64_t pos = 0;
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool is_alone = k < alone.size() && alone[k] == i;
        const uint8_t *src = is_alone ? extra[k].data() : dev_bytes.data() + dso[i];
        const uint64_t len = is_alone ? extra[k].size() : dso[i + 1] - dso[i];
        if (is_alone) ++k;
        sym_off[i] = pos;
        if (pos + len > out_cap) { if (first == MH_OK) first = MH_ERR_CAPACITY; pos += len; continue; }
        if (len) std::memcpy(out + pos, src, size_t(len));
        pos += len;
    }
    sym_off[n] = pos;
    return first;
}

}  // namespace mhapi
