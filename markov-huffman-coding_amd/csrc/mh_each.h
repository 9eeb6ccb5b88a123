// mh_each.h — launch interface between the per-stream-model calls of the C ABI (mh_api_each.cpp) and their kernels
// (mh_each.hip): many independent order-0/1 streams, each under a model of its own (include/mh.h, "BATCHES OF STREAMS, ONE
// MODEL EACH").  The batch layouts (closed-form units and index slices, packed payloads) are those of mh_batch.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"
#include "mh_kernels.h"

namespace mhe {

constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;
constexpr uint32_t SLOT_ENTRIES = 256;
// device bytes of one live context: len8 u8[256] | code64 u64[256] | prim u16[256] | tree u32[256], + stream/context/leaves
constexpr size_t SLOT_BYTES = 256 * (1 + 8 + 2 + 4) + 4 + 1 + 2;
// device bytes per stream: type, longest code, context -> slot map, first slot
constexpr size_t STREAM_BYTES = 1 + 4 + 256 * 4 + 8;

// A model set on the device.  Stream i's contexts map to slots through ctx_slot[i * 256 + ctx] (order 0: ctx 0 only);
// NO_SLOT marks an empty context.  Slots of one stream are consecutive, in ascending context order, from slot_base[i].
// Per slot, 256 entries each:
//   len8, code64   the encoder's code of every symbol (len 0: no code), right aligned
//   prim           the reference's 8-bit first level (src/huffman.cpp:97-123), indexed by the next 8 stream bits MSB
//                  first: leaf = 0x8000 | len(1..8) << 8 | symbol, 0x8000 alone = no code with this prefix, else the
//                  walk-tree id of the inner node at depth 8
//   tree           walk tree, node 0 = root: right << 16 | left, a child is 0x8000 | symbol for a leaf, else its id
// During training code64 holds the slot's 256 counts until the tree build replaces them with the codes.
struct SetDev {
    uint64_t n, nslots;
    uint8_t *type;               // n: 0 or 1
    uint32_t *maxlen;            // n: longest code of the stream's model
    uint32_t *ctx_slot;          // n * 256
    unsigned long long *slot_base;   // n + 1
    uint32_t *slot_stream;       // nslots
    uint8_t *slot_ctx;           // nslots
    uint16_t *slot_leaves;       // nslots: leaves of the tree (a one-symbol context has two)
    uint8_t *len8;               // nslots * 256
    unsigned long long *code64;  // nslots * 256
    uint16_t *prim;              // nslots * 256
    uint32_t *tree;              // nslots * 256
};

// train workspace: status block (status, stop, longest code, shortest code) | live-context masks (4 x u64 per stream) |
// live-context counts -> slot bases (n + 1, scanned) | scan block sums
struct TrainLayout {
    size_t off_masks, off_counts, off_sums, total;
};
inline TrainLayout train_layout(uint64_t n) {
    TrainLayout l;
    l.off_masks = 64;
    l.off_counts = l.off_masks + size_t(n) * 32;
    l.off_sums = l.off_counts + size_t(n + 1) * 8;
    l.total = (l.off_sums + size_t(mhb::scan_blocks(n + 1) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

// table workspace: status block | per-slot table bits (nslots + 1, scanned) | scan block sums | tail word
struct TabLayout {
    size_t off_bits, off_sums, off_tail, total;
};
inline TabLayout tab_layout(uint64_t n, uint64_t nslots) {
    TabLayout l;
    const uint64_t len = nslots + 1 > n + 1 ? nslots + 1 : n + 1;
    l.off_bits = 64;
    l.off_sums = l.off_bits + size_t(nslots + 1) * 8;
    l.off_tail = l.off_sums + size_t(mhb::scan_blocks(len) + 1) * 8;
    l.total = (l.off_tail + 8 + 255) & ~size_t(255);
    return l;
}

// status block words of the train workspace
enum { TRAIN_STATUS = 0, TRAIN_STOP = 1, TRAIN_MAXLEN = 2, TRAIN_MINLEN = 3 };

// node arrays and meta records of tree_build_kernel (mh_kernels.h, TB_NODE_STRIDE / TB_META_STRIDE per slot): the train
// call's temporary buffer
struct TreeNodes {
    uint16_t *left, *right;
    uint8_t *sym, *height;
    uint32_t *meta;
};
constexpr size_t TREE_NODE_BYTES = 520 * 6 + 16 * 4;          // per slot

// train, part 1: checks the offsets, finds each stream's live contexts, scans their counts into d_ws's slot bases
hipError_t launch_train_count(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total, int order, uint32_t prev0,
                              void *d_ws, hipStream_t st);
// train, part 2 (s.nslots known, s allocated, its counts zeroed): slot map, per-slot histograms, one tree per slot
hipError_t launch_train_build(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t total, int order, uint32_t prev0, const SetDev &s,
                              const TreeNodes &t, void *d_ws, hipStream_t st);
// every stream's table file, packed back to back: tab_off[n + 1]
hipError_t launch_tables(const SetDev &s, uint8_t *d_out, uint64_t cap, unsigned long long *d_tab_off, void *d_ws, hipStream_t st);

struct EncEachParams {
    const uint8_t *data;
    const uint64_t *in_off;
    uint64_t n, total;
    uint32_t prev0;
    uint32_t chunk_shift;           // 0: no index
    unsigned long long *index;
    uint8_t *out;
    uint64_t cap;
    unsigned long long *out_off;
    unsigned long long *nbits;
    SetDev set;
};
hipError_t launch_encode_each(const EncEachParams &p, void *d_ws, hipStream_t st);

}  // namespace mhe

namespace mhb {

// The parameters of mhb::launch_decode (mh_batch.h; kernels: mh_batch.hip).  The other call families over compressed batches
// begin their parameters the same way (FindParams, CrcParams): it is what the symbol decoders (mhb::Dec<K>, mh_symdec_dev.hpp)
// read.
struct DecodeParams {
    DecBatchParams b;               // the batch and, under a shared model, its decode tables
    mhe::SetDev set;                // the models under a set
};

}  // namespace mhb
