// mh_batch.h — launch interface between the batch calls of the C ABI (mh_api_batch.cpp) and their kernels (mh_batch.hip):
// many independent order-0/1 streams under one shared model, each starting in context prev0 (include/mh.h, "BATCHES OF
// INDEPENDENT STREAMS"), and the batch decoders of every model kind (launch_decode).  The common kernel headers are included
// read-only; nothing here changes a single-stream path.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_kernels.h"

namespace mhb {

// device status values beyond mh_kernels.h's (first int32 of a batch workspace; per-stream status arrays hold MH_* codes)
enum { BATCH_STATUS_ARG = 4 };

// A stream is cut into work units of B_SUB input bytes, one wave (64 lanes x 16 bytes) each.  Stream i's units are numbered
// from unit_base(in_off_i, i) = in_off_i / B_SUB + i (the closed form of mh_batch_index_base): no scan is needed to find them,
// and a workload of `total` bytes in n streams has at most total / B_SUB + n + 1 unit numbers.
constexpr uint32_t B_SUB = 1024;
constexpr uint32_t B_VEC = 16;
constexpr int B_THREADS = 1024;                 // 16 waves: the encode tables take 128 KiB of LDS, one workgroup per CU
constexpr uint32_t SCAN_BLOCK = 1024;           // elements per workgroup of the segmented-offset scans

inline uint64_t units_of(uint64_t total, uint64_t n_streams) { return total / B_SUB + n_streams + 1; }
inline uint64_t scan_blocks(uint64_t len) { return (len + SCAN_BLOCK - 1) / SCAN_BLOCK; }
// chunk numbers of an indexed batch: stream i's chunks from sym_off_i / chunk_symbols + i (0 chunk_symbols: index-free, none)
inline uint64_t work_items(uint64_t n_streams, uint64_t sym_total, uint32_t chunk_symbols) {
    return chunk_symbols ? sym_total / chunk_symbols + n_streams + 1 : 0;
}

// encode workspace: status block | unit bits (u64, scanned in place) | scan block sums | tail word
struct EncLayout {
    size_t off_units, off_sums, off_tail, total;
};
inline EncLayout enc_layout(uint64_t n_streams, uint64_t total) {
    EncLayout l;
    const uint64_t u = units_of(total, n_streams);
    const uint64_t len = u > n_streams + 1 ? u : n_streams + 1;
    l.off_units = 64;
    l.off_sums = l.off_units + size_t(u) * 8;
    l.off_tail = l.off_sums + size_t(scan_blocks(len) + 1) * 8;
    l.total = (l.off_tail + 8 + 255) & ~size_t(255);
    return l;
}

// decode workspace: status block | per-stream status (when the caller passes none) | symbol counts (scanned) | block sums
struct DecLayout {
    size_t off_status, off_counts, off_sums, total;
};
inline DecLayout dec_layout(uint64_t n_streams) {
    DecLayout l;
    l.off_status = 64;
    l.off_counts = (l.off_status + size_t(n_streams) * 4 + 15) & ~size_t(15);
    l.off_sums = l.off_counts + size_t(n_streams + 1) * 8;
    l.total = (l.off_sums + size_t(scan_blocks(n_streams + 1) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

struct EncBatchParams {
    const uint8_t *data;            // concatenated input
    const uint64_t *in_off;         // n + 1 stream offsets
    uint64_t n, total;
    uint32_t prev0;
    uint32_t chunk_shift;           // 0: no index
    unsigned long long *index;      // stream i at in_off_i >> chunk_shift + i, or nullptr
    uint8_t *out;                   // packed payloads, 16-byte aligned
    uint64_t cap;
    unsigned long long *out_off;    // n + 1 byte offsets (written)
    unsigned long long *nbits;      // n payload lengths (written)
    const uint16_t *enc16;          // slot order, 12-bit codes or ENC16_ESCAPE
    const uint8_t *len_slot;        // slot order
    const uint8_t *len8;            // prev * 256 + sym
    const uint64_t *code64;         // prev * 256 + sym, right aligned
    int max_len;
};

struct DecBatchParams {
    const uint8_t *payload;
    const uint64_t *pay_off;        // n + 1 byte offsets of the payloads
    const uint64_t *nbits;          // n
    uint64_t n, pay_total;
    uint32_t prev0;
    uint8_t *out;
    uint64_t out_cap;
    unsigned long long *sym_off;    // n + 1 output offsets: input with an index, output without
    uint64_t sym_total;             // with an index: sym_off[n] as the caller knows it
    const uint64_t *index;          // nullptr: index-free (one lane walks one stream)
    uint32_t chunk_shift;
    uint64_t walk_max_bits;         // index-free: longer streams are refused (per-stream MH_ERR_ARG)
    int *stream_status;             // n (caller's array or the workspace's)
    const uint16_t *prim;
    const uint16_t *sec;
    const uint32_t *sec_base;
    const uint32_t *tree;
    uint32_t P, nsec, sec_lds, direct, H;
};

// The model a batch to decode was coded under, for the call families that serve all three (decoding: launch_decode, search:
// mh_find.h, re-coding: mh_recode.h, ...).  Shared: one order-0/1 model (the tables go to LDS, prev0 is a byte, index entries
// carry one context byte).  Set: stream i under set model i (mh_each.h).  Shared2: one order-2 model: DecBatchParams holds the
// model's order-2 tables (prim / sec / sec_base / tree of 65536 contexts, general form, read from L2, sec_lds = direct = 0),
// prev0 is the 16-bit start context, index entries carry the context in bits 48..63.
enum class Model { Shared, Set, Shared2 };

// LDS bytes of a shared model's decode tables as mhb::load_tables (mh_batch_dev.hpp) lays them out: the two are a pair, and
// this is the only copy of the size.  T: any struct with P, nsec and sec_lds (DecBatchParams, the single-stream DecodeParams).
template <typename T>
inline size_t tables_lds(const T &t) {
    return 1024 + (size_t(256) << t.P) * 2 + (t.sec_lds ? ((size_t(t.nsec) * 2 + 15) & ~size_t(15)) : 0);
}

// histogram fix-up: validates the offsets, then moves each stream's first pair from the concatenation's context to prev0
hipError_t launch_hist_fixup(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total, uint32_t prev0,
                             unsigned long long *d_counts, int order, int *d_status, hipStream_t st);
hipError_t launch_encode_batch(const EncBatchParams &p, void *d_ws, hipStream_t st);
// A batch to decode under any model kind: DecodeParams { DecBatchParams b; mhe::SetDev set; } is defined in mh_each.h, which
// knows the model set (mh_each.h includes this header, so the struct cannot be completed here); a caller includes both.
// model: what the batch was coded under; workspace: dec_layout.
struct DecodeParams;
hipError_t launch_decode(const DecodeParams &p, Model model, void *d_ws, hipStream_t st);

}  // namespace mhb
