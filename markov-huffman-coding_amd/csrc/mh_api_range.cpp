// mh_api_range.cpp — the byte-range calls of the C ABI (include/mh.h, "RANDOM ACCESS: BYTE RANGES OF AN INDEXED STREAM" and
// "RANDOM ACCESS INTO ORDER-2 STREAMS"): ranges of one indexed stream decoded on the device under an order-0/1 or an order-2
// model (kernels: mh_range.hip), and the host-buffer form that uploads only the payload bytes of the chunks the ranges touch.
#include "mh_api_internal.hpp"
#include "mh_batch.h"
#include "mh_range.h"

using namespace mhapi;

namespace {

thread_local uint64_t t_range_upload = 0;   // payload bytes the calling thread's last mh_decode_ranges(_o2) uploaded

// Byte spans of the payload closer than this are uploaded as one window: one transfer and one launch cost more than the
// bytes in between (a PCIe transfer of 1 MiB takes about as long as the fixed cost of a call).
constexpr uint64_t RANGE_MERGE_GAP = uint64_t(1) << 20;

// a run of whole chunks [c0, c1] of one range, cut so that its payload bytes and its output fit a segment
struct Piece {
    uint64_t j;            // range
    uint64_t b, e;         // symbols
    uint64_t lo, hi;       // payload bytes [lo, hi) of its chunks
    uint64_t c0, c1;       // chunks
    uint64_t at;           // output offset in the caller's buffer
};

// mh_dev_decode_ranges (o2 = false: an order-0/1 model) and mh_dev_decode_ranges_o2 (an order-2 model)
int dev_decode_ranges(const mh_model *m, bool o2, const uint8_t *d_payload, uint64_t payload_byte_base, uint64_t payload_bytes, uint64_t nbits,
                      const uint64_t *d_index, uint32_t chunk_symbols, uint64_t n_symbols, const uint32_t *d_fine, const uint64_t *d_ranges,
                      size_t n_ranges, uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap, int32_t *d_range_status, void *d_ws,
                      size_t ws_bytes, void *stream) {
    if (!(o2 ? order2(m) : order01(m)) || (!d_payload && payload_bytes) || (!d_index && n_symbols) || !d_ws) return MH_ERR_ARG;
    if (n_ranges && (!d_ranges || !d_out_at || !d_range_status)) return MH_ERR_ARG;
    if ((!d_out && out_cap) || !aligned16(d_out) || !aligned16(d_ws)) return MH_ERR_ARG;
    const int shift = chunk_shift_of(chunk_symbols);
    if (shift < 0 || n_symbols > nbits) return MH_ERR_ARG;
    // the order-2 fine index exists for chunks of up to 1024 symbols (its entries are 16-bit distances from the chunk's entry)
    if (o2 && d_fine && (shift > 10 || (reinterpret_cast<uintptr_t>(d_fine) & 3u))) return MH_ERR_ARG;
    if (payload_byte_base > (nbits + 7) / 8 || payload_bytes > (nbits + 7) / 8 - payload_byte_base) return MH_ERR_ARG;
    if (ws_bytes < mhq::range_layout(n_ranges).total) return MH_ERR_CAPACITY;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    if (!m->d_prim || !have_device()) return MH_ERR_NO_DEVICE;
    mhq::RangeParams p{};
    p.payload = d_payload; p.win_base = payload_byte_base; p.win_bytes = payload_bytes;
    p.nbits = nbits; p.n_symbols = n_symbols;
    p.index = d_index; p.chunk_shift = uint32_t(shift);
    p.fine = d_fine;
    p.unit_shift = d_fine ? uint32_t(MH_T_SUB_SHIFT) : uint32_t(shift);
    p.n_units = (n_symbols + (uint64_t(1) << p.unit_shift) - 1) >> p.unit_shift;
    p.ranges = d_ranges; p.n = n_ranges;
    p.out = d_out; p.out_at = d_out_at; p.out_cap = out_cap;
    p.status = d_range_status;
    fill_dec_tables(m, p.tab);
    HIP_TRY(mhq::launch_ranges(p, o2 ? mhb::Model::Shared2 : mhb::Model::Shared, d_ws, static_cast<hipStream_t>(stream)));
    return MH_OK;
}

}  // namespace

extern "C" {

uint64_t mh_last_range_upload_bytes(void) { return t_range_upload; }

size_t mh_dev_decode_ranges_workspace(size_t n_ranges) { return mhq::range_layout(n_ranges).total; }
size_t mh_dev_decode_ranges_o2_workspace(size_t n_ranges) { return mhq::range_layout(n_ranges).total; }

int mh_dev_decode_ranges(const mh_model *m, const uint8_t *d_payload, uint64_t payload_byte_base, uint64_t payload_bytes, uint64_t nbits,
                         const uint64_t *d_index, uint32_t chunk_symbols, uint64_t n_symbols, const uint32_t *d_fine,
                         const uint64_t *d_ranges, size_t n_ranges, uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                         int32_t *d_range_status, void *d_ws, size_t ws_bytes, void *stream) {
    return dev_decode_ranges(m, false, d_payload, payload_byte_base, payload_bytes, nbits, d_index, chunk_symbols, n_symbols, d_fine, d_ranges,
                             n_ranges, d_out, d_out_at, out_cap, d_range_status, d_ws, ws_bytes, stream);
}

int mh_dev_decode_ranges_o2(const mh_model *m, const uint8_t *d_payload, uint64_t payload_byte_base, uint64_t payload_bytes, uint64_t nbits,
                            const uint64_t *d_index, uint32_t chunk_symbols, uint64_t n_symbols, const uint32_t *d_fine,
                            const uint64_t *d_ranges, size_t n_ranges, uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                            int32_t *d_range_status, void *d_ws, size_t ws_bytes, void *stream) {
    return dev_decode_ranges(m, true, d_payload, payload_byte_base, payload_bytes, nbits, d_index, chunk_symbols, n_symbols, d_fine, d_ranges,
                             n_ranges, d_out, d_out_at, out_cap, d_range_status, d_ws, ws_bytes, stream);
}

/* ------------------------------------------------------- host-buffer call */

int mh_decode_ranges(const mh_model *m, const uint8_t *payload, uint64_t nbits, const uint64_t *index, uint32_t chunk_symbols,
                     uint64_t n_symbols, const uint64_t *ranges, size_t n_ranges, uint8_t *out, size_t out_cap, uint64_t *out_off,
                     int32_t *range_status) {
    return decode_ranges_host(m, false, payload, nbits, index, chunk_symbols, n_symbols, ranges, n_ranges, out, out_cap, out_off,
                              range_status);
}

int mh_decode_ranges_o2(const mh_model *m, const uint8_t *payload, uint64_t nbits, const uint64_t *index, uint32_t chunk_symbols,
                        uint64_t n_symbols, const uint64_t *ranges, size_t n_ranges, uint8_t *out, size_t out_cap, uint64_t *out_off,
                        int32_t *range_status) {
    return decode_ranges_host(m, true, payload, nbits, index, chunk_symbols, n_symbols, ranges, n_ranges, out, out_cap, out_off,
                              range_status);
}

}  // extern "C"

namespace mhapi {

int decode_ranges_host(const mh_model *m, bool o2, const uint8_t *payload, uint64_t nbits, const uint64_t *index, uint32_t chunk_symbols,
                       uint64_t n_symbols, const uint64_t *ranges, size_t n_ranges, uint8_t *out, size_t out_cap, uint64_t *out_off,
                       int32_t *range_status) {
    t_range_upload = 0;
    if (!(o2 ? order2(m) : order01(m)) || (!payload && nbits) || (!index && n_symbols) || (!ranges && n_ranges) || !out_off || (!out && out_cap))
        return MH_ERR_ARG;
    const int shift = chunk_shift_of(chunk_symbols);
    if (shift < 0 || n_symbols > nbits) return MH_ERR_ARG;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    if (m->max_len > mh::MAX_CODE_BITS) return MH_ERR_CODE_TOO_LONG;
    // outputs packed in range order; a refused range has length 0, one that does not fit keeps its length
    std::vector<int32_t> rst(n_ranges, MH_OK);
    uint64_t pos = 0;
    for (size_t j = 0; j < n_ranges; ++j) {
        out_off[j] = pos;
        const uint64_t b = ranges[2 * j], e = ranges[2 * j + 1];
        if (b > e || e > n_symbols) { rst[j] = MH_ERR_ARG; continue; }
        if (pos + (e - b) > out_cap) rst[j] = MH_ERR_CAPACITY;
        pos += e - b;
    }
    out_off[n_ranges] = pos;

    // every range as runs of whole chunks whose payload bytes and output each fit a segment (a single chunk always fits:
    // a segment holds at least MH_CHUNK_MAX symbols, and a chunk's payload is a few KiB)
    const uint64_t seg = segment_bytes();
    const uint64_t nchunks = mh_index_entries(n_symbols, chunk_symbols);
    const uint64_t pos_mask = o2 ? MH_INDEX2_BIT_MASK : MH_INDEX_BIT_MASK;     // (order 2: two context bytes above)
    auto ent = [&](uint64_t c) { return index[c] & pos_mask; };
    auto cend = [&](uint64_t c) { return c + 1 < nchunks ? ent(c + 1) : nbits; };
    std::vector<Piece> pieces;
    for (size_t j = 0; j < n_ranges; ++j) {
        const uint64_t b = ranges[2 * j], e = ranges[2 * j + 1];
        if (rst[j] != MH_OK || b == e) continue;
        const size_t keep = pieces.size();
        const uint64_t c1 = (e - 1) >> shift;
        // a range that ends inside its last chunk does not depend on the entry behind that chunk (include/mh.h: such an item
        // is checked for null table entries and for running past nbits only): where that entry gives no end, the chunk's
        // span is what its symbols in front of `end` can take at most
        const bool inside = e != n_symbols && (e & ((uint64_t(1) << shift) - 1u)) != 0;
        auto cbound = [&](uint64_t k) {
            const uint64_t t = cend(k), sk = ent(k);
            if (k != c1 || !inside || (t >= sk && t <= nbits) || sk > nbits) return t;
            return std::min(nbits, sk + (e - (k << shift)) * uint64_t(m->max_len > 0 ? m->max_len : 1));
        };
        for (uint64_t c = b >> shift; c <= c1;) {
            const uint64_t s = ent(c);
            auto fits = [&](uint64_t k) {
                const uint64_t t = cbound(k);
                return t >= s && t <= nbits && ((t + 7) >> 3) - (s >> 3) <= seg && ((k - c + 1) << shift) <= seg;
            };
            if (s > nbits || cbound(c) < s || cbound(c) > nbits) { rst[j] = MH_ERR_CORRUPT; break; }   // (the device checks the rest)
            uint64_t lo = c, hi = c1;                                                              // last chunk that fits
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) >> 1;
                if (fits(mid)) lo = mid; else hi = mid - 1;
            }
            Piece q;
            q.j = j;
            q.b = std::max(b, c << shift);
            q.e = std::min(e, (lo + 1) << shift);
            q.lo = s >> 3;
            q.hi = (cbound(lo) + 7) >> 3;
            q.c0 = c; q.c1 = lo;
            q.at = out_off[j] + (q.b - b);
            pieces.push_back(q);
            c = lo + 1;
        }
        if (rst[j] != MH_OK) pieces.resize(keep);
    }
    std::stable_sort(pieces.begin(), pieces.end(), [](const Piece &x, const Piece &y) { return x.lo < y.lo; });

    // windows: runs of pieces whose spans lie closer than RANGE_MERGE_GAP, cut at a segment of payload and of output
    struct Window { size_t p0, p1; uint64_t lo, hi, c0, c1, out; };
    std::vector<Window> wins;
    for (size_t k = 0; k < pieces.size(); ++k) {
        const Piece &q = pieces[k];
        if (!wins.empty()) {
            Window &w = wins.back();
            const uint64_t hi = std::max(w.hi, q.hi);
            if (q.lo < w.hi + RANGE_MERGE_GAP && hi - w.lo <= seg && w.out + (q.e - q.b) <= seg) {
                w.p1 = k + 1; w.hi = hi; w.c0 = std::min(w.c0, q.c0); w.c1 = std::max(w.c1, q.c1); w.out += q.e - q.b;
                continue;
            }
        }
        wins.push_back(Window{k, k + 1, q.lo, q.hi, q.c0, q.c1, q.e - q.b});
    }
    size_t max_n = 0;
    uint64_t max_bytes = 0, max_out = 0, max_idx = 0;
    for (const Window &w : wins) {
        max_n = std::max(max_n, w.p1 - w.p0);
        max_bytes = std::max(max_bytes, w.hi - w.lo);
        max_out = std::max(max_out, w.out);
        max_idx = std::max(max_idx, w.c1 - w.c0 + 3);
    }

    const hipStream_t st = nullptr;
    if (!wins.empty()) {
        const size_t wsb = mhq::range_layout(max_n).total;
        DevBuf d_pl, d_idx, d_rng, d_out, d_st, d_ws;
        HIP_TRY(d_pl.alloc(size_t(max_bytes)));
        HIP_TRY(d_idx.alloc(size_t(max_idx) * 8));
        HIP_TRY(d_rng.alloc(max_n * 24));                        // begin, end | out_at
        HIP_TRY(d_out.alloc(size_t(max_out)));
        HIP_TRY(d_st.alloc(max_n * 4));
        HIP_TRY(d_ws.alloc(wsb));
        std::vector<uint64_t> h_rng(max_n * 3);
        std::vector<int32_t> h_st(max_n);
        std::vector<uint8_t> h_out(static_cast<size_t>(max_out));
        for (const Window &w : wins) {
            const size_t k = w.p1 - w.p0;
            const uint64_t bytes = w.hi - w.lo;
            HIP_TRY(stage_h2d(d_pl.p, payload + w.lo, size_t(bytes), st));
            t_range_upload += bytes;
            // the index entries the lanes read: the window's chunks, the one in front (order check) and the one behind (end)
            const uint64_t i0 = w.c0 ? w.c0 - 1 : 0, i1 = std::min(w.c1 + 2, nchunks);
            HIP_TRY(hipMemcpyAsync(d_idx.p, index + i0, size_t(i1 - i0) * 8, hipMemcpyHostToDevice, st));
            const uint64_t *d_index = reinterpret_cast<const uint64_t *>(reinterpret_cast<uintptr_t>(d_idx.p) - uintptr_t(i0) * 8u);
            uint64_t o = 0;
            for (size_t i = 0; i < k; ++i) {
                const Piece &q = pieces[w.p0 + i];
                h_rng[2 * i] = q.b; h_rng[2 * i + 1] = q.e;
                h_rng[2 * k + i] = o;
                o += q.e - q.b;
            }
            HIP_TRY(hipMemcpyAsync(d_rng.p, h_rng.data(), k * 24, hipMemcpyHostToDevice, st));
            const int rc = dev_decode_ranges(m, o2, d_pl.as<uint8_t>(), w.lo, bytes, nbits, d_index, chunk_symbols, n_symbols, nullptr,
                                             d_rng.as<uint64_t>(), k, d_out.as<uint8_t>(), d_rng.as<uint64_t>() + 2 * k, w.out,
                                             d_st.as<int32_t>(), d_ws.p, wsb, st);
            if (rc != MH_OK) return rc;
            HIP_TRY(hipMemcpyAsync(h_st.data(), d_st.p, k * 4, hipMemcpyDeviceToHost, st));
            if (w.out) HIP_TRY(stage_d2h(h_out.data(), d_out.p, size_t(w.out), st));
            HIP_TRY(hipStreamSynchronize(st));
            for (size_t i = 0; i < k; ++i) {
                const Piece &q = pieces[w.p0 + i];
                if (h_st[i] != MH_OK) { if (rst[q.j] == MH_OK) rst[q.j] = h_st[i]; continue; }
                std::memcpy(out + q.at, h_out.data() + h_rng[2 * k + i], size_t(q.e - q.b));
            }
        }
    }
    int first = MH_OK;
    for (size_t j = 0; j < n_ranges && first == MH_OK; ++j) first = rst[j];
    if (range_status) std::copy(rst.begin(), rst.end(), range_status);
    return first;
}

}  // namespace mhapi
