// mh_select.h — the launch interface between the selecting calls of the C ABI (mh_api_select.cpp) and their kernels
// (mh_select.hip): a new batch from picked streams of up to MH_SELECT_MAX_SOURCES compressed batches, and a pick list from a
// per-stream predicate (include/mh.h, "SELECTING RECORDS OF BATCHES").  Model-free: payload bytes and 64-bit index entries
// are copied as they are, so nothing here knows a table.  The batch layouts are those of mh_batch.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"

namespace mhs {

constexpr uint32_t MAX_SOURCES = 8;                  // MH_SELECT_MAX_SOURCES
constexpr uint64_t NONE = ~uint64_t(0);              // MH_SELECT_NONE
constexpr uint32_t SRC_SHIFT = 56;                   // pick = source << 56 | stream
constexpr uint64_t STREAM_MASK = (uint64_t(1) << SRC_SHIFT) - 1;
constexpr uint32_t WITHOUT_HITS = 1;                 // MH_PICKS_WITHOUT_HITS

// An output stream's bytes are cut along the aligned 1 KiB windows of the OUTPUT, one wave (64 lanes x 16 bytes) each: the
// windows that hold bytes of pick j are numbered from out_off_j / PIECE + j, the closed form of mh_batch.h's work units.
constexpr uint32_t PIECE_SHIFT = 10, PIECE = 1u << PIECE_SHIFT;
constexpr uint32_t GATHER_RUN = 8;                  // consecutive window numbers a wave takes after one search

struct Source {
    const uint8_t *payload;
    const uint64_t *pay_off;        // n + 1
    const uint64_t *nbits;          // n
    const uint64_t *sym_off;        // n + 1, or nullptr
    const uint64_t *index;          // slices at sym_off_i / chunk + i, or nullptr
    uint64_t n, pay_total, sym_total;
    uint64_t first;                 // the check kernel's threads [first, first + n] look at this source's offsets
};

// workspace: status block | lens u64[2 (n + 1)] | block sums | osym u64[n + 1] | from u64[n] | ifrom u64[n] | pick status
// (when the caller passes none).  lens: [0, n] the picks' payload bytes, [n + 1, 2n + 1] their symbol counts, entries n and 2n + 1 zero; one
// exclusive scan over the whole array turns the first half into out_off and the second into out_off[n] + out_sym_off; osym
// is out_sym_off by itself, which the index kernel searches (the caller's d_out_sym_off may be NULL).
// from / ifrom: the address of a pick's first payload byte and of its first index entry in its source.
struct SelectLayout {
    size_t off_lens, off_sums, off_osym, off_from, off_ifrom, off_status, total;
};
inline SelectLayout select_layout(uint64_t n_picks) {
    SelectLayout l;
    const uint64_t len = 2 * (n_picks + 1);
    l.off_lens = 64;
    l.off_sums = l.off_lens + size_t(len) * 8;
    l.off_osym = l.off_sums + size_t(mhb::scan_blocks(len) + 1) * 8;
    l.off_from = l.off_osym + size_t(n_picks + 1) * 8;
    l.off_ifrom = l.off_from + size_t(n_picks) * 8;
    l.off_status = l.off_ifrom + size_t(n_picks) * 8;
    l.total = (l.off_status + size_t(n_picks) * 4 + 255) & ~size_t(255);
    return l;
}

struct SelectParams {
    Source src[MAX_SOURCES];
    uint32_t n_sources;
    uint32_t chunk_shift;           // of the index, when one is written
    uint64_t checks;                // sum of n + 1 over the sources: the check kernel's offset threads
    const uint64_t *picks;
    uint64_t n;                     // picks
    uint8_t *out;                   // nullptr: count only
    uint64_t cap;
    unsigned long long *out_off;    // n + 1
    unsigned long long *out_nbits;  // n
    unsigned long long *out_sym_off;// n + 1, or nullptr
    unsigned long long *out_index;  // or nullptr
    uint64_t index_cap;
    int *pick_status;               // n (caller's array or the workspace's)
    bool have_sym;                  // every source has sym_off
};

// workspace of the pick helper: status block | keep u64[n + 1] (scanned in place) | block sums
struct PicksLayout {
    size_t off_keep, off_sums, total;
};
inline PicksLayout picks_layout(uint64_t n_streams) {
    PicksLayout l;
    l.off_keep = 64;
    l.off_sums = l.off_keep + size_t(n_streams + 1) * 8;
    l.total = (l.off_sums + size_t(mhb::scan_blocks(n_streams + 1) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

struct PicksParams {
    const uint64_t *hit_off;        // n + 1, or nullptr
    const int *stream_status;       // n, or nullptr
    uint64_t n;
    uint32_t source, flags;
    unsigned long long *picks;      // n
    unsigned long long *n_kept;     // 1
};

hipError_t launch_select(const SelectParams &p, void *d_ws, hipStream_t st);
hipError_t launch_picks(const PicksParams &p, void *d_ws, hipStream_t st);

}  // namespace mhs
