// mh_api_select.cpp — the selecting calls of the C ABI (include/mh.h, "SELECTING RECORDS OF BATCHES"): the argument rules
// of the two device calls (kernels: mh_select.hip) and the host forms, which are plain C++ and need no device.
#include "mh_api_internal.hpp"
#include "mh_select.h"

using namespace mhapi;

namespace {

// The rules both forms of the select call check before anything runs.  have_sym (out): every source has symbol offsets.
int select_rules(const mh_coded_batch_args *sources, uint32_t n_sources, const uint64_t *picks, size_t n_picks, const uint8_t *out_payload,
                 const uint64_t *out_off, const uint64_t *out_nbits, const uint64_t *out_sym_off, const uint64_t *out_index,
                 uint32_t chunk_symbols, bool &have_sym) {
    if (!sources || n_sources < 1 || n_sources > MH_SELECT_MAX_SOURCES) return MH_ERR_ARG;
    if ((!picks && n_picks) || !out_off || (!out_nbits && n_picks)) return MH_ERR_ARG;
    if (out_index && chunk_shift_of(chunk_symbols) < 0) return MH_ERR_ARG;
    have_sym = true;
    for (uint32_t s = 0; s < n_sources; ++s) {
        const mh_coded_batch_args &b = sources[s];
        if (!b.d_pay_off || (!b.d_nbits && b.n_streams) || b.n_streams > mhs::STREAM_MASK) return MH_ERR_ARG;
        if (out_payload && !b.d_payload && b.pay_total) return MH_ERR_ARG;
        if (!b.d_sym_off) have_sym = false;
        if (out_index && (!b.d_sym_off || !b.d_index || b.chunk_symbols != chunk_symbols)) return MH_ERR_ARG;
    }
    if (out_sym_off && !have_sym) return MH_ERR_ARG;
    return MH_OK;
}

bool offsets_ok_to(const uint64_t *off, size_t n, uint64_t total) { return offsets_ok(off, n) && off[n] == total; }

}  // namespace

extern "C" {

size_t mh_dev_select_batch_workspace(size_t total_source_streams, size_t n_picks) {
    (void)total_source_streams;                                    // nothing is kept per source stream
    return mhs::select_layout(n_picks).total;
}

int mh_dev_select_batch(const mh_select_args *a) {
    if (!a || a->struct_size != sizeof(mh_select_args)) return MH_ERR_ARG;
    bool have_sym = false;
    const int rc = select_rules(a->sources, a->n_sources, a->d_picks, a->n_picks, a->d_out_payload, a->d_out_off, a->d_out_nbits, a->d_out_sym_off,
                                a->d_out_index, a->chunk_symbols, have_sym);
    if (rc != MH_OK) return rc;
    void *d_ws = a->launch.d_ws;
    if (!d_ws || !aligned16(d_ws) || !aligned16(a->d_out_payload)) return MH_ERR_ARG;
    const mhs::SelectLayout L = mhs::select_layout(a->n_picks);
    if (a->launch.ws_bytes < L.total) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    mhs::SelectParams p{};
    for (uint32_t s = 0; s < a->n_sources; ++s) {
        const mh_coded_batch_args &b = a->sources[s];
        p.src[s] = {b.d_payload, b.d_pay_off, b.d_nbits, b.d_sym_off, b.d_index, b.n_streams, b.pay_total, b.sym_total, p.checks};
        p.checks += uint64_t(b.n_streams) + 1;
    }
    p.n_sources = a->n_sources;
    p.chunk_shift = a->d_out_index ? uint32_t(chunk_shift_of(a->chunk_symbols)) : 0u;
    p.picks = a->d_picks;
    p.n = a->n_picks;
    p.out = a->d_out_payload;
    p.cap = a->cap;
    p.out_off = reinterpret_cast<unsigned long long *>(a->d_out_off);
    p.out_nbits = reinterpret_cast<unsigned long long *>(a->d_out_nbits);
    p.out_sym_off = reinterpret_cast<unsigned long long *>(a->d_out_sym_off);
    p.out_index = reinterpret_cast<unsigned long long *>(a->d_out_index);
    p.index_cap = a->index_cap;
    p.pick_status = a->d_pick_status ? a->d_pick_status : ws_status(d_ws, L.off_status);
    p.have_sym = have_sym;
    HIP_TRY(mhs::launch_select(p, d_ws, static_cast<hipStream_t>(a->launch.stream)));
    return MH_OK;
}

size_t mh_dev_picks_from_hits_workspace(size_t n_streams) { return mhs::picks_layout(n_streams).total; }

int mh_dev_picks_from_hits(const mh_picks_args *a) {
    if (!a || a->struct_size != sizeof(mh_picks_args)) return MH_ERR_ARG;
    if ((!a->d_picks && a->n_streams) || !a->d_n_kept || a->source >= MH_SELECT_MAX_SOURCES || (a->flags & ~MH_PICKS_WITHOUT_HITS)) return MH_ERR_ARG;
    if (a->n_streams > mhs::STREAM_MASK || !a->launch.d_ws || !aligned16(a->launch.d_ws)) return MH_ERR_ARG;
    if (a->launch.ws_bytes < mhs::picks_layout(a->n_streams).total) return MH_ERR_CAPACITY;
    if (!have_device()) return MH_ERR_NO_DEVICE;
    const mhs::PicksParams p{a->d_hit_off, a->d_stream_status, a->n_streams, a->source, a->flags, reinterpret_cast<unsigned long long *>(a->d_picks),
                             reinterpret_cast<unsigned long long *>(a->d_n_kept)};
    HIP_TRY(mhs::launch_picks(p, a->launch.d_ws, static_cast<hipStream_t>(a->launch.stream)));
    return MH_OK;
}

int mh_select_batch(const mh_coded_batch_args *sources, uint32_t n_sources, const uint64_t *picks, size_t n_picks, uint8_t *out_payload, size_t cap,
                    uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_sym_off, uint64_t *out_index, uint64_t index_cap, uint32_t chunk_symbols,
                    int32_t *pick_status) {
    bool have_sym = false;
    int rc = select_rules(sources, n_sources, picks, n_picks, out_payload, out_off, out_nbits, out_sym_off, out_index, chunk_symbols, have_sym);
    if (rc != MH_OK) return rc;
    for (uint32_t s = 0; s < n_sources; ++s) {
        const mh_coded_batch_args &b = sources[s];
        if (!offsets_ok_to(b.d_pay_off, b.n_streams, b.pay_total)) return MH_ERR_ARG;
        if (b.d_sym_off && !offsets_ok_to(b.d_sym_off, b.n_streams, b.sym_total)) return MH_ERR_ARG;
    }
    const uint32_t cs = out_index ? uint32_t(chunk_shift_of(chunk_symbols)) : 0u;
    // a pick's stream in its source, or nullptr for an empty output stream (MH_SELECT_NONE or a refused pick)
    auto source_of = [&](size_t j, uint64_t &i, bool &refused) -> const mh_coded_batch_args * {
        const uint64_t s = picks[j] >> mhs::SRC_SHIFT;
        i = picks[j] & mhs::STREAM_MASK;
        refused = false;
        if (picks[j] == MH_SELECT_NONE) return nullptr;
        refused = s >= n_sources || i >= sources[s].n_streams ||
                  sources[s].d_nbits[i] > (sources[s].d_pay_off[i + 1] - sources[s].d_pay_off[i]) * 8u;
        return refused ? nullptr : &sources[s];
    };
    uint64_t bytes = 0, syms = 0;
    for (size_t j = 0; j < n_picks; ++j) {
        uint64_t i;
        bool refused;
        const mh_coded_batch_args *b = source_of(j, i, refused);
        if (refused && rc == MH_OK) rc = MH_ERR_ARG;
        if (pick_status) pick_status[j] = refused ? MH_ERR_ARG : MH_OK;
        out_off[j] = bytes;
        if (out_sym_off) out_sym_off[j] = syms;
        out_nbits[j] = b ? b->d_nbits[i] : 0;
        if (b) bytes += (b->d_nbits[i] + 7) >> 3;
        if (b && have_sym) syms += b->d_sym_off[i + 1] - b->d_sym_off[i];
    }
    out_off[n_picks] = bytes;
    if (out_sym_off) out_sym_off[n_picks] = syms;
    if ((out_payload && bytes > cap) || (out_index && (syms >> cs) + n_picks + 1 > index_cap)) return rc != MH_OK ? rc : MH_ERR_CAPACITY;
    syms = 0;
    for (size_t j = 0; j < n_picks; ++j) {
        uint64_t i;
        bool refused;
        const mh_coded_batch_args *b = source_of(j, i, refused);
        if (!b) continue;
        if (out_payload) std::copy_n(b->d_payload + b->d_pay_off[i], out_off[j + 1] - out_off[j], out_payload + out_off[j]);
        if (!have_sym) continue;
        const uint64_t so = b->d_sym_off[i], m = b->d_sym_off[i + 1] - so;
        if (out_index) std::copy_n(b->d_index + (so >> cs) + i, (m + chunk_symbols - 1) >> cs, out_index + (syms >> cs) + j);
        syms += m;
    }
    return rc;
}

int mh_picks_from_hits(const uint64_t *hit_off, const int32_t *stream_status, size_t n_streams, uint32_t source, uint32_t flags, uint64_t *picks,
                       uint64_t *n_kept) {
    if ((!picks && n_streams) || !n_kept || source >= MH_SELECT_MAX_SOURCES || (flags & ~MH_PICKS_WITHOUT_HITS) || n_streams > mhs::STREAM_MASK)
        return MH_ERR_ARG;
    uint64_t kept = 0;
    for (size_t i = 0; i < n_streams; ++i) {
        bool k = true;
        if (hit_off) k = (hit_off[i + 1] > hit_off[i]) != bool(flags & MH_PICKS_WITHOUT_HITS);
        if (k && stream_status) k = stream_status[i] == MH_OK;
        if (k) picks[kept++] = (uint64_t(source) << mhs::SRC_SHIFT) | i;
    }
    *n_kept = kept;
    std::fill(picks + kept, picks + n_streams, uint64_t(MH_SELECT_NONE));
    return MH_OK;
}

}  // extern "C"
