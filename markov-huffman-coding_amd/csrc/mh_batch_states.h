// mh_batch_states.h — launch interface between the segment-state calls of the C ABI (mh_api_batch_states.cpp) and their
// kernels (mh_batch_states.hip): a batch of index-free streams (order 0/1: what the reference writes; order 2: what
// mh_dev_encode_batch_o2 writes without its sidecar index) is cut into S-bit segments, every segment's true entry state is
// found in a fixed number of launches, and the settled states then drive an index writer or a decoder with one lane per
// segment (include/mh.h, "SEGMENT STATES OF INDEX-FREE BATCHES" and "SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES").
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"
#include "mh_each.h"
#include "mh_kernels.h"

namespace mhs {

// Segment length S in bits.  Segment k of stream i is number seg_base(pay_off_i, i) + k = pay_off_i * 8 / S + i + k (the
// closed form of mh_batch_index_base): ceil(nbits_i / S) <= ceil(bytes_i * 8 / S) numbers never overlap the next stream's.
// A workload of pay_total bytes in n streams has at most pay_total * 8 / S + n + 1 segment numbers.
constexpr uint32_t SEG_BITS = 512;
constexpr uint32_t SEG_SHIFT = 6;                   // log2(SEG_BITS / 8): segment numbers from byte offsets
static_assert((8u << SEG_SHIFT) == SEG_BITS, "segment numbering works on payload bytes");
constexpr uint32_t WARMUP_BITS = 256;               // speculation: decode this much of the predecessor's bits first
constexpr uint32_t WARMUP2_BITS = SEG_BITS;         // order 2: the whole predecessor (segment 1 then starts from the true start state)
constexpr int REPAIR_PASSES = 8;                    // fixed number of repair launches before the one-lane fallback
constexpr int ST_THREADS = 256;

inline uint64_t segs_of(uint64_t pay_total, uint64_t n) { return pay_total * 8 / SEG_BITS + n + 1; }

// one segment: entry and end state = context << 56 | stream-relative bit position (order 2: the two context bytes << 48 |
// position, the order-2 index-entry format); end == SEG_BAD when the decode met a null table entry; count = symbols whose code starts in [k * S, min((k + 1) * S, nbits))
struct SegRec {
    unsigned long long entry, end, count;
};
constexpr unsigned long long SEG_BAD = ~0ull;

// workspace: header | per-stream status (n, i32) | first / last inconsistent segment per stream (n, u64 each) |
// records, two buffers (ping-pong) | segment counts (scanned in place) | scan block sums
// Header words (i32): 0 status, 1 stop, 2 .. 2 + K changed flags of the speculation and the repair passes, 12 streams the
// fallback walk walked, 16 status of the states call; u64 from byte 128: the tag of the batch the states belong to.
enum { HDR_STATUS = 0, HDR_STOP = 1, HDR_CHANGED = 2, HDR_WALKED = 12, HDR_STATES_STATUS = 16 };
static_assert(HDR_CHANGED + REPAIR_PASSES < HDR_WALKED, "the changed flags end in front of the walk counter");
constexpr unsigned long long TAG_MAGIC = 0x6273656700000000ull;     // tag word 0: TAG_MAGIC | kind
// the stop word: 0 run, 1 bad offsets or no states of this batch (MH_ERR_ARG), STOP_CAPACITY the index does not fit
enum { STOP_CAPACITY = 2 };
constexpr size_t HDR_TAG = 128;
constexpr int TAG_WORDS = 8;
constexpr size_t HDR_BYTES = 256;
struct Layout {
    size_t off_status, off_first, off_last, off_rec0, off_rec1, off_counts, off_sums, total;
};
inline Layout layout(uint64_t n, uint64_t pay_total) {
    Layout l;
    const uint64_t g = segs_of(pay_total, n);
    l.off_status = HDR_BYTES;
    l.off_first = (l.off_status + size_t(n) * 4 + 15) & ~size_t(15);
    l.off_last = l.off_first + size_t(n) * 8;
    l.off_rec0 = l.off_last + size_t(n) * 8;
    l.off_rec1 = l.off_rec0 + size_t(g) * sizeof(SegRec);
    l.off_counts = l.off_rec1 + size_t(g) * sizeof(SegRec);
    l.off_sums = l.off_counts + size_t(g) * 8;
    l.total = (l.off_sums + size_t(mhb::scan_blocks(g) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

enum Kind { KIND_SHARED = 1, KIND_SET = 2, KIND_SHARED2 = 3 };

struct StParams {
    const uint8_t *payload;
    const uint64_t *pay_off;        // n + 1
    const uint64_t *nbits;          // n
    uint64_t n, pay_total, segs;
    uint32_t prev0;
    unsigned long long state0;      // a stream's start state: prev0 << 56, or (prev0, prev0) << 48 (KIND_SHARED2)
    unsigned long long pos_mask;    // the position bits of a state: MH_INDEX_BIT_MASK or MH_INDEX2_BIT_MASK
    uint64_t walk_max_bits;
    unsigned long long tag[TAG_WORDS];   // identifies the batch (kind, n, pay_total, prev0, pointers)
    int *caller_status;             // n or nullptr
    unsigned long long *sym_off;    // states: n + 1 (written); index / emit: nullptr
    // index / emit
    unsigned long long *index;
    uint64_t index_cap;
    uint32_t chunk_shift;
    uint8_t *out;
    uint64_t out_cap;
    // model: the shared model's tables (KIND_SHARED, as the batch decoder loads them; KIND_SHARED2: the order-2 tables in
    // the general form, read from L2) or a set (KIND_SET)
    int kind;
    mhb::DecBatchParams tabs;
    size_t lds;
    mhe::SetDev set;
    // KIND_SHARED2, the warm-up's recovery: rep[b] = the heaviest live context (a, b) or 0xFFFF, live = one bit per context
    const uint16_t *rep;
    const uint32_t *live;
};

// states: checks, speculation, K repair passes, fallback walk, proof, scan -> sym_off and the settled records in d_ws
hipError_t launch_states(const StParams &p, void *d_ws, hipStream_t st);
// the chunk-index slices from the settled records
hipError_t launch_index(const StParams &p, void *d_ws, hipStream_t st);
// the decoded bytes from the settled records
hipError_t launch_emit(const StParams &p, void *d_ws, hipStream_t st);

}  // namespace mhs
