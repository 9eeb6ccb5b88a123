// mh_each.hip — batches of independent order-0/1 streams, each under its own model (include/mh.h, "BATCHES OF STREAMS, ONE
// MODEL EACH"): the reference's default per-file flow (train, write the table, encode) for N messages in a fixed number of
// launches.  Layouts: mh_each.h; shared device code: mh_batch_dev.hpp (units, scans, bit writer), mh_each_dev.hpp (the
// per-stream symbol decoder, shared with mh_range.hip); the trees are built by
// mh_tree.hip's tree_build_kernel over the live (stream, context) pairs, so the reference's tie-breaking has one copy.
//   each_check_kernel       offsets non-decreasing, [0] == 0, [n] == total
//   each_live_kernel        one wave per (stream, 1 KiB sub-step): the contexts the sub-step's symbols are coded in, OR-ed
//                           into the stream's 256-bit mask (order 1: prev0 and every byte but the stream's last)
//   each_nlive_kernel       one thread per stream: its live contexts (scanned next into slot bases)
//   each_slotmap_kernel     one thread per (stream, context): context -> slot map, slot -> (stream, context)
//   each_hist_kernel        one wave per (stream, 1 KiB sub-step): counts into the slot rows (global atomics)
//   tree_build_kernel       (mh_tree.hip, unchanged) one wave per slot: the tree and the codes of one (stream, live context)
//   each_pack_kernel        one wave per slot: first level and walk tree from the tree's nodes
//   each_tab_*              table files: bits per slot (scanned), bytes per stream (scanned), the pre-order traversal of
//                           every tree by one lane (src/huffman.cpp:174-188, src/markov_huffman.cpp:80-88)
//   each_enc_*              mh_batch.hip's encoder with the codes of stream i's slots (L2) instead of one LDS image
//   each_dec_*              mh_batch.hip's two decoders with stream i's first level and walk tree (L2)
// Every loop is bounded by a symbol count, a leaf count, 64 code bits or nbits_i.  The number of launches does not depend on n,
// except for one more tree_build_kernel launch per 4 M live contexts (TREE_SLICE).
#include "mh_each.h"
#include "mh_batch_dev.hpp"
#include "mh_each_dev.hpp"
#include "../../include/mh.h"

namespace mhe {

using mhb::B_SUB;
using mhb::B_THREADS;
using mhb::B_VEC;
using mhb::BATCH_STATUS_ARG;
using mhk::BitCursor;
using mhk::BitSrc;
constexpr uint16_t NONE = 0xFFFF;                // (mh_tree.hip: a node without children)

namespace {

using mhb::byte_of;
using mhb::check_batch;
using mhb::fail;
using mhb::find_stream;
using mhb::grid_for;
using mhb::grid_threads;
using mhb::gtid;
using mhb::load16;
using mhb::scan_exclusive;
using mhb::stopped;
using mhb::stream_fail;
using mhb::SUB_SHIFT;

constexpr uint32_t WAVES = B_THREADS / 64;
constexpr uint64_t TREE_SLICE = 1u << 22;          // slots per tree_build_kernel launch: 2^22 x TB_NODE_STRIDE < 2^32
static_assert((TREE_SLICE - 1) * mhk::TB_NODE_STRIDE + mhk::TB_NODE_STRIDE <= (1ull << 32), "tree_build_kernel's 32-bit node offsets");


__global__ void each_check_kernel(const uint64_t *off, uint64_t n, uint64_t total, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i > n) return;
    const bool bad = (i == 0 && off[0] != 0) || (i == n && off[n] != total) || (i < n && off[i + 1] < off[i]);
    if (bad) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
}

// the lane's bytes of unit u (closed-form numbering of mh_batch.h); false when the unit (wave-uniform) has nothing
struct Unit {
    uint64_t i, a, ni, ub, j0;
    uint32_t cnt, prev;
    uint32_t x[4];
};
__device__ __forceinline__ bool unit_of(const uint8_t *data, const uint64_t *in_off, uint64_t n, uint32_t prev0, uint64_t u, Unit &l) {
    l.i = find_stream(in_off, n, SUB_SHIFT, u);
    if (l.i >= n) return false;
    l.a = in_off[l.i];
    l.ni = in_off[l.i + 1] - l.a;
    l.ub = (l.a >> SUB_SHIFT) + l.i;
    const uint64_t s0 = (u - l.ub) << SUB_SHIFT;
    if (s0 >= l.ni) return false;
    l.j0 = s0 + uint64_t(mhk::lane_id()) * B_VEC;
    l.cnt = l.j0 < l.ni ? uint32_t(l.ni - l.j0 < B_VEC ? l.ni - l.j0 : B_VEC) : 0u;
    l.x[0] = l.x[1] = l.x[2] = l.x[3] = 0;
    l.prev = prev0;
    if (l.cnt) {
        load16(data + l.a + l.j0, l.cnt, l.x);
        if (l.j0) l.prev = data[l.a + l.j0 - 1];
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ train

__device__ __forceinline__ void mark(unsigned long long (&m)[4], uint32_t c) {
    const unsigned long long b = 1ull << (c & 63u);
    m[0] |= (c >> 6) == 0 ? b : 0ull;
    m[1] |= (c >> 6) == 1 ? b : 0ull;
    m[2] |= (c >> 6) == 2 ? b : 0ull;
    m[3] |= (c >> 6) == 3 ? b : 0ull;
}

__global__ __launch_bounds__(B_THREADS) void each_live_kernel(const uint8_t *data, const uint64_t *in_off, uint64_t n, uint64_t nunits,
                                                              uint32_t prev0, unsigned long long *masks, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t nw = uint64_t(gridDim.x) * WAVES;
    for (uint64_t u = uint64_t(blockIdx.x) * WAVES + threadIdx.x / 64; u < nunits; u += nw) {
        Unit l;
        if (!unit_of(data, in_off, n, prev0, u, l)) continue;             // wave-uniform
        unsigned long long m[4] = {0, 0, 0, 0};
        if (l.cnt) mark(m, l.prev);                                        // the context of the lane's first symbol
#pragma unroll
        for (uint32_t t = 0; t + 1 < B_VEC; ++t)                          // ... and of the following ones
            if (t + 1 < l.cnt) mark(m, byte_of(l.x, t));
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (int d = 32; d >= 1; d >>= 1) m[k] |= __shfl_xor(m[k], d);
        const uint32_t lane = mhk::lane_id();
        if (lane < 4) {
            const unsigned long long v = lane == 0 ? m[0] : lane == 1 ? m[1] : lane == 2 ? m[2] : m[3];
            if (v) atomicOr(&masks[l.i * 4 + lane], v);
        }
    }
}

__global__ void each_nlive_kernel(const uint64_t *in_off, uint64_t n, int order, const unsigned long long *masks, unsigned long long *counts,
                                  const int *stop) {
    if (stopped(stop)) return;
    const uint64_t i = gtid();
    if (i > n) return;
    if (i == n) { counts[n] = 0; return; }
    if (order == 0) { counts[i] = in_off[i + 1] > in_off[i] ? 1u : 0u; return; }
    const unsigned long long *m = masks + i * 4;
    counts[i] = uint64_t(__popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]));
}

__global__ void each_slotmap_kernel(SetDev s, const uint64_t *in_off, int order, const unsigned long long *masks, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t t = gtid();
    if (t >= s.n * 256u) return;
    const uint64_t i = t >> 8;
    const uint32_t c = uint32_t(t & 255u);
    if (c == 0) { s.type[i] = uint8_t(order); s.maxlen[i] = 0; }
    bool live;
    uint32_t rank = 0;
    if (order == 0) {
        live = c == 0 && in_off[i + 1] > in_off[i];
    } else {
        const unsigned long long *m = masks + i * 4;
        const uint32_t w = c >> 6, b = c & 63u;
        live = (m[w] >> b) & 1ull;
        for (uint32_t k = 0; k < w; ++k) rank += uint32_t(__popcll(m[k]));
        rank += uint32_t(__popcll(m[w] & ((1ull << b) - 1ull)));
    }
    uint32_t slot = NO_SLOT;
    if (live) {
        const uint64_t sl = s.slot_base[i] + rank;
        if (sl < s.nslots) {
            slot = uint32_t(sl);
            s.slot_stream[sl] = uint32_t(i);
            s.slot_ctx[sl] = uint8_t(c);
        }
    }
    s.ctx_slot[t] = slot;
}

// counts into code64 of the pair's slot (zeroed by the host); order 0 counts every symbol in context 0
__global__ __launch_bounds__(B_THREADS) void each_hist_kernel(const uint8_t *data, const uint64_t *in_off, uint64_t nunits, uint32_t prev0,
                                                              int order, SetDev s, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t nw = uint64_t(gridDim.x) * WAVES;
    for (uint64_t u = uint64_t(blockIdx.x) * WAVES + threadIdx.x / 64; u < nunits; u += nw) {
        Unit l;
        if (!unit_of(data, in_off, s.n, prev0, u, l)) continue;
        const uint32_t *row = s.ctx_slot + l.i * 256u;
        uint32_t prev = l.prev;
#pragma unroll
        for (uint32_t t = 0; t < B_VEC; ++t) {
            const uint32_t sym = byte_of(l.x, t);
            if (t < l.cnt) {
                const uint32_t slot = row[order ? prev : 0u];
                if (slot != NO_SLOT) atomicAdd(&s.code64[size_t(slot) * 256u + sym], 1ull);
            }
            prev = sym;
        }
    }
}

// One wave per slot, after tree_build_kernel (mh_tree.hip, launched over the slots: the reference's tie-breaking, one copy)
// has written the slot's codes and node arrays: the first level and the walk tree from the nodes, the leaf count, and the
// code lengths into the stream's and the set's records.  wsmeta: [TRAIN_MAXLEN] max, [TRAIN_MINLEN] min over the set.
__global__ __launch_bounds__(64) void each_pack_kernel(SetDev s, TreeNodes t, uint32_t *wsmeta) {
    const uint32_t lane = threadIdx.x;
    const uint64_t slot = blockIdx.x;
    __shared__ uint16_t left[mhk::TB_NODE_STRIDE], right[mhk::TB_NODE_STRIDE], nid[mhk::TB_NODE_STRIDE];
    __shared__ uint8_t sym[mhk::TB_NODE_STRIDE];
    __shared__ uint32_t tr[256];
    __shared__ uint32_t s_leaves;
    const uint32_t *meta = t.meta + slot * mhk::TB_META_STRIDE;
    const uint32_t nn = meta[0], root = meta[1], maxlen = meta[2], lenmask = meta[15];
    const size_t nb = size_t(slot) * mhk::TB_NODE_STRIDE;
    for (uint32_t k = lane; k < mhk::TB_NODE_STRIDE; k += 64) {
        left[k] = t.left[nb + k]; right[k] = t.right[nb + k]; sym[k] = t.sym[nb + k];
    }
    for (uint32_t k = lane; k < 256; k += 64) tr[k] = 0;
    __syncthreads();
    if (root == 0xFFFFFFFFu) {                       // (a live context has counts: not reached)
        for (uint32_t k = lane; k < 256; k += 64) { s.prim[slot * 256u + k] = mh::DEC16_NULL; s.tree[slot * 256u + k] = 0; }
        if (lane == 0) s.slot_leaves[slot] = 0;
        return;
    }
    if (lane == 0) {                                 // walk-tree ids: root 0, the other inner nodes in node order
        uint32_t next = 1, leaves = 0;
        for (uint32_t k = 0; k < nn; ++k) {
            if (left[k] == NONE) { nid[k] = NONE; ++leaves; }
            else nid[k] = k == root ? 0 : uint16_t(next++);
        }
        s_leaves = leaves;                           // (a one-symbol tree: its two leaves; the first leaf became the root)
    }
    __syncthreads();
    auto enc_child = [&](uint32_t ch) -> uint32_t { return left[ch] == NONE ? (mh::TREE_LEAF | sym[ch]) : uint32_t(nid[ch]); };
    for (uint32_t k = lane; k < nn; k += 64)
        if (left[k] != NONE) tr[nid[k]] = (enc_child(right[k]) << 16) | enc_child(left[k]);
    for (uint32_t w = lane; w < 256; w += 64) {      // first level: the 8 bits of w, MSB first, from the root
        uint32_t node = root, depth = 0;
        while (depth < 8 && left[node] != NONE) {
            node = ((w >> (7 - depth)) & 1u) ? right[node] : left[node];
            ++depth;
        }
        s.prim[slot * 256u + w] = left[node] == NONE ? uint16_t(mh::DEC16_LEAF | (depth << 8) | sym[node]) : nid[node];
    }
    __syncthreads();
    for (uint32_t k = lane; k < 256; k += 64) s.tree[slot * 256u + k] = tr[k];
    if (lane == 0) {
        s.slot_leaves[slot] = uint16_t(s_leaves);
        // shortest code: meta[15] has bit l - 1 for every length l in use, 0 for a one-symbol context (one 1-bit code)
        const uint32_t minlen = lenmask ? uint32_t(__builtin_ctz(lenmask)) + 1u : 1u;
        atomicMax(&s.maxlen[s.slot_stream[slot]], maxlen);
        atomicMax(&wsmeta[TRAIN_MAXLEN], maxlen);
        atomicMin(&wsmeta[TRAIN_MINLEN], minlen);
    }
}

// ------------------------------------------------------------------------------------------------ table files

__global__ void each_tab_bits_kernel(SetDev s, unsigned long long *bits, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t k = gtid();
    if (k > s.nslots) return;
    bits[k] = k < s.nslots ? 10ull * s.slot_leaves[k] - 1ull : 0ull;   // leaves 9 bits each, inner nodes 1 (src/huffman.cpp:174-188)
}

// order 1: the type bit, one bit per context, and the trees; order 0: the tree alone (an empty order-0 model writes nothing)
__global__ void each_tab_size_kernel(SetDev s, const unsigned long long *pbits, unsigned long long *tab_off, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t i = gtid();
    if (i > s.n) return;
    if (i == s.n) { tab_off[i] = 0; return; }
    const unsigned long long b = pbits[s.slot_base[i + 1]] - pbits[s.slot_base[i]] + (s.type[i] ? 257ull : 0ull);
    tab_off[i] = (b + 7) >> 3;
}

// zeroes the output bytes [0, *off_end) (bits are OR-ed into shared edge words) or reports that they do not fit
__global__ void each_zero_kernel(const unsigned long long *off_end, uint8_t *out, uint64_t cap, int *status, int *stop, uint32_t *tail) {
    if (stopped(stop)) return;
    const uint64_t bytes = *off_end;
    if (bytes > cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
        return;
    }
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
    for (uint64_t k = gtid(); k < (bytes >> 2); k += uint64_t(gridDim.x) * blockDim.x) o[k] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *tail = 0u;
}

// Threads 0 .. n-1: the leading 1 of an order-1 table.  Threads n .. n+nslots-1: one context each, its present bit (order 1)
// and its tree in pre-order: 0 for an inner node, 1 + the symbol for a leaf, left before right.  The traversal keeps the
// path from the root as bits (depth <= 64: a code's length) and walks down again from the root after each leaf to the
// next right branch: at most 64 steps per leaf, no stack.
__global__ void each_tab_write_kernel(SetDev s, const unsigned long long *pbits, const unsigned long long *tab_off, uint8_t *out,
                                      uint32_t *tail, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t t = gtid();
    if (t >= s.n + s.nslots) return;
    const uint64_t bytes = tab_off[s.n];
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    mhb::BitWriter bw;
    if (t < s.n) {
        if (!s.type[t]) return;
        bw.init(reinterpret_cast<uint32_t *>(out), tail, tail_w, uint64_t(tab_off[t]) * 8u);
        bw.push(1u, 1u);
        bw.finish();
        return;
    }
    const uint64_t k = t - s.n;
    const uint64_t i = s.slot_stream[k];
    const uint32_t c = s.slot_ctx[k];
    const bool o1 = s.type[i] != 0;
    const uint64_t rel = o1 ? 1u + c + (pbits[k] - pbits[s.slot_base[i]]) : 0u;
    bw.init(reinterpret_cast<uint32_t *>(out), tail, tail_w, uint64_t(tab_off[i]) * 8u + rel);
    if (o1) bw.push(1u, 1u);                                   // the context has a tree
    const uint32_t *tr = s.tree + k * 256u;
    bw.push(0u, 1u);                                           // the root is inner (a one-symbol tree has two leaves)
    uint64_t path = 0;
    uint32_t depth = 0, node = 0;
    const uint32_t leaves = s.slot_leaves[k];
    for (uint32_t emitted = 0; emitted < leaves;) {
        // go left from the inner node `node` until a leaf
        uint32_t ch = tr[node] & 0xFFFFu;
        path <<= 1; ++depth;
        while (!(ch & mh::TREE_LEAF) && depth < 64) {
            bw.push(0u, 1u);
            node = ch & 255u;
            ch = tr[node] & 0xFFFFu;
            path <<= 1; ++depth;
        }
        for (;;) {                                             // ch is a leaf at `path`: emit it, then find the next right branch
            bw.push(0x100u | (ch & 255u), 9u);
            if (++emitted >= leaves) break;
            while (depth > 0 && (path & 1u)) { path >>= 1; --depth; }
            if (depth == 0) { emitted = leaves; break; }       // (a tree with fewer leaves than recorded: not reached)
            path |= 1u;
            uint32_t at = 0;
            for (uint32_t d = 0; d < depth; ++d) {             // walk down again to the right child
                const uint32_t pair = tr[at];
                ch = ((path >> (depth - 1 - d)) & 1u) ? (pair >> 16) : (pair & 0xFFFFu);
                if (d + 1 < depth) at = ch & 255u;
            }
            if (!(ch & mh::TREE_LEAF)) { bw.push(0u, 1u); node = ch & 255u; break; }
        }
    }
    bw.finish();
}

__global__ void each_tail_kernel(const unsigned long long *off_end, uint8_t *out, const uint32_t *tail, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t bytes = *off_end;
    if (!(bytes & 3u)) return;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(tail);
    for (uint64_t b = bytes & ~uint64_t(3); b < bytes; ++b) out[b] = t[b & 3u];
}

// ------------------------------------------------------------------------------------------------ encode

// stream i's code of sym after prev: from the slot of its context (len 0: no code, the symbol is skipped as mh_encode does)
__device__ __forceinline__ void code_of(const SetDev &s, const uint32_t *row, uint32_t ctx, uint32_t sym, uint32_t &len, uint64_t &code) {
    const uint32_t slot = row[ctx];
    if (slot == NO_SLOT) { len = 0; code = 0; return; }
    len = s.len8[size_t(slot) * 256u + sym];
    code = s.code64[size_t(slot) * 256u + sym];
}

__global__ __launch_bounds__(B_THREADS) void each_enc_len_kernel(EncEachParams p, uint64_t nunits, unsigned long long *ubits, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t nw = uint64_t(gridDim.x) * WAVES;
    for (uint64_t u = uint64_t(blockIdx.x) * WAVES + threadIdx.x / 64; u < nunits; u += nw) {
        Unit l;
        uint32_t bits = 0;
        if (unit_of(p.data, p.in_off, p.n, p.prev0, u, l) && l.cnt) {
            const uint32_t *row = p.set.ctx_slot + l.i * 256u;
            const bool o1 = p.set.type[l.i] != 0;
            uint32_t prev = l.prev;
#pragma unroll
            for (uint32_t t = 0; t < B_VEC; ++t) {
                const uint32_t sym = byte_of(l.x, t);
                if (t < l.cnt) {
                    const uint32_t slot = row[o1 ? prev : 0u];
                    if (slot != NO_SLOT) bits += p.set.len8[size_t(slot) * 256u + sym];
                }
                prev = sym;
            }
        }
        bits = mhk::wave_sum(bits);
        if (mhk::lane_id() == 0) ubits[u] = bits;
    }
}

__global__ void each_enc_sizes_kernel(EncEachParams p, const unsigned long long *ubase, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t i = gtid();
    if (i > p.n) return;
    if (i == p.n) { p.out_off[i] = 0; return; }
    const uint64_t u0 = (p.in_off[i] >> SUB_SHIFT) + i, u1 = (p.in_off[i + 1] >> SUB_SHIFT) + i + 1;
    const unsigned long long bits = ubase[u1] - ubase[u0];
    p.nbits[i] = bits;
    p.out_off[i] = (bits + 7) >> 3;
}

__global__ __launch_bounds__(B_THREADS) void each_enc_emit_kernel(EncEachParams p, uint64_t nunits, const unsigned long long *ubase,
                                                                  uint32_t *tail, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t bytes = p.out_off[p.n];
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint64_t nw = uint64_t(gridDim.x) * WAVES;
    for (uint64_t u = uint64_t(blockIdx.x) * WAVES + threadIdx.x / 64; u < nunits; u += nw) {
        Unit l;
        if (!unit_of(p.data, p.in_off, p.n, p.prev0, u, l)) continue;     // wave-uniform
        const uint32_t *row = p.set.ctx_slot + l.i * 256u;
        const bool o1 = p.set.type[l.i] != 0;
        uint32_t bits = 0, prev = l.prev;
        uint32_t lens[B_VEC];
        uint64_t codes[B_VEC];
#pragma unroll
        for (uint32_t t = 0; t < B_VEC; ++t) {
            const uint32_t sym = byte_of(l.x, t);
            lens[t] = 0; codes[t] = 0;
            if (t < l.cnt) code_of(p.set, row, o1 ? prev : 0u, sym, lens[t], codes[t]);
            bits += lens[t];
            prev = sym;
        }
        const uint32_t excl = mhk::wave_inclusive_sum(bits) - bits;
        const uint64_t sbit = (ubase[u] - ubase[l.ub]) + excl;      // stream-relative
        if (p.index && l.cnt && (l.j0 & ((uint64_t(1) << p.chunk_shift) - 1u)) == 0)
            p.index[(l.a >> p.chunk_shift) + l.i + (l.j0 >> p.chunk_shift)] = (uint64_t(l.prev) << 56) | sbit;
        if (!bits) continue;
        mhb::BitWriter bw;
        bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[l.i]) * 8u + sbit);
#pragma unroll
        for (uint32_t t = 0; t < B_VEC; ++t) bw.code(codes[t], lens[t]);
        bw.finish();
    }
}

// ------------------------------------------------------------------------------------------------ decode

__global__ void each_dec_check_kernel(DecEachParams p, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i > p.n) return;
    check_batch(p, i, status, stop);
}

__global__ __launch_bounds__(256) void each_dec_idx_kernel(DecEachParams p, uint64_t nwork, int *status, const int *stop) {
    if (stopped(stop)) return;
    const uint32_t cs = p.chunk_shift;
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t i = find_stream(p.sym_off, p.n, cs, w);
        if (i >= p.n) continue;
        const uint64_t a = p.sym_off[i], ni = p.sym_off[i + 1] - a;
        const uint64_t first = (w - ((a >> cs) + i)) << cs;
        if (first >= ni || p.stream_status[i] == MH_ERR_ARG) continue;
        const uint64_t nb = p.nbits[i];
        const uint64_t e = p.index[w];
        const uint64_t start = e & MH_INDEX_BIT_MASK;
        const bool last = first + (uint64_t(1) << cs) >= ni;
        const uint64_t end = last ? nb : (p.index[w + 1] & MH_INDEX_BIT_MASK);
        const uint32_t nsym = uint32_t(last ? ni - first : (uint64_t(1) << cs));
        if (start > end || end > nb) { stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.payload, p.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + start);
        const uint32_t *row = p.set.ctx_slot + i * 256u;
        const bool o1 = p.set.type[i] != 0;
        uint32_t prev = uint32_t(e >> 56), used = 0;
        bool bad = false;
        mhb::ByteOut bo;
        bo.init(p.out, a + first);
        for (uint32_t t = 0; t < nsym && !bad; ++t) {
            prev = decode_sym(p.set, row, o1 ? prev : 0u, src, bc, used, bad);
            bo.put(prev);
        }
        bo.flush();
        if (bad || used != end - start) stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
    }
}

// EMIT = false: count the stream's symbols into sym_off[i] (scanned next); true: write them at out[sym_off[i] ...)
template <bool EMIT>
__global__ __launch_bounds__(256) void each_dec_walk_kernel(DecEachParams p, int *status, const int *stop) {
    if (stopped(stop)) return;
    for (uint64_t i = gtid(); i <= p.n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (i == p.n) { if (!EMIT) p.sym_off[i] = 0; continue; }
        if (!EMIT) p.sym_off[i] = 0;
        if (p.stream_status[i] != MH_OK) continue;
        const uint64_t nb = p.nbits[i];
        if (!EMIT && nb > p.walk_max_bits) { stream_fail(p, status, i, MH_ERR_ARG, BATCH_STATUS_ARG); continue; }
        uint64_t count = 0;
        if (EMIT) {
            const uint64_t a = p.sym_off[i];
            count = p.sym_off[i + 1] - a;
            if (a + count > p.out_cap) { stream_fail(p, status, i, MH_ERR_CAPACITY, mhk::MHK_STATUS_CAPACITY); continue; }
        }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.payload, p.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0);
        const uint32_t *row = p.set.ctx_slot + i * 256u;
        const bool o1 = p.set.type[i] != 0;
        uint32_t prev = p.prev0, used = 0;
        bool bad = false;
        mhb::ByteOut bo;
        bo.init(p.out, EMIT ? p.sym_off[i] : 0);
        uint64_t k = 0;
        // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
        while (used < nb && !bad && (!EMIT || k < count)) {
            prev = decode_sym(p.set, row, o1 ? prev : 0u, src, bc, used, bad);
            if (EMIT && !bad) bo.put(prev);
            ++k;
        }
        if (EMIT) bo.flush();
        if (bad || used != nb || (EMIT && k != count)) { stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        if (!EMIT) p.sym_off[i] = k;                               // src/coding.cpp:158: the stream ends exactly at nbits
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ launchers

hipError_t launch_train_count(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total, int order, uint32_t prev0,
                              void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const TrainLayout L = train_layout(n);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    auto *masks = reinterpret_cast<unsigned long long *>(ws + L.off_masks);
    auto *counts = reinterpret_cast<unsigned long long *>(ws + L.off_counts);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, L.off_counts, st);        // status block and masks
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(each_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, d_in_off, n, total, status, stop);
    if (order && total) {
        const uint64_t U = mhb::units_of(total, n);
        hipLaunchKernelGGL(each_live_kernel, dim3(grid_for(U, WAVES, 2)), dim3(B_THREADS), 0, st, d_data, d_in_off, n, U, prev0, masks, stop);
    }
    hipLaunchKernelGGL(each_nlive_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, d_in_off, n, order, masks, counts, stop);
    if ((e = scan_exclusive(counts, n + 1, sums, stop, st)) != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t launch_train_build(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t total, int order, uint32_t prev0, const SetDev &s,
                              const TreeNodes &t, void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const TrainLayout L = train_layout(s.n);
    int *stop = reinterpret_cast<int *>(ws) + TRAIN_STOP;
    auto *masks = reinterpret_cast<unsigned long long *>(ws + L.off_masks);
    if (s.n) hipLaunchKernelGGL(each_slotmap_kernel, grid_threads(s.n * 256u, 256), dim3(256), 0, st, s, d_in_off, order, masks, stop);
    if (total) {
        const uint64_t U = mhb::units_of(total, s.n);
        hipLaunchKernelGGL(each_hist_kernel, dim3(grid_for(U, WAVES, 2)), dim3(B_THREADS), 0, st, d_data, d_in_off, U, prev0, order, s, stop);
    }
    hipError_t e = hipMemsetAsync(ws + 4 * TRAIN_MINLEN, 0xFF, 4, st);   // (the max starts at 0 from launch_train_count)
    if (e != hipSuccess) return e;
    if (!s.nslots) return hipGetLastError();
    // The counts sit in code64: block c of tree_build_kernel reads its row into LDS before it writes the row's codes.  The
    // kernel indexes its node arrays with 32-bit products (context x TB_NODE_STRIDE), so it runs over slices of TREE_SLICE
    // slots: one launch per 4 M live contexts (1 GiB of counts).
    for (uint64_t s0 = 0; s0 < s.nslots; s0 += TREE_SLICE) {
        const uint64_t k = s.nslots - s0 < TREE_SLICE ? s.nslots - s0 : TREE_SLICE;
        const size_t nb = size_t(s0) * mhk::TB_NODE_STRIDE;
        mhk::TreeBuildOut o{};
        o.len8 = s.len8 + s0 * 256u; o.code64 = s.code64 + s0 * 256u;
        o.node_left = t.left + nb; o.node_right = t.right + nb; o.node_sym = t.sym + nb; o.node_height = t.height + nb;
        o.ctx_meta = t.meta + s0 * mhk::TB_META_STRIDE;
        o.hcap = 8;
        if ((e = mhk::launch_tree_build(s.code64 + s0 * 256u, int(k), o, st)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(each_pack_kernel, dim3(uint32_t(s.nslots)), dim3(64), 0, st, s, t, reinterpret_cast<uint32_t *>(ws));
    return hipGetLastError();
}

hipError_t launch_tables(const SetDev &s, uint8_t *d_out, uint64_t cap, unsigned long long *d_tab_off, void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const TabLayout L = tab_layout(s.n, s.nslots);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    auto *bits = reinterpret_cast<unsigned long long *>(ws + L.off_bits);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    auto *tail = reinterpret_cast<uint32_t *>(ws + L.off_tail);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(each_tab_bits_kernel, grid_threads(s.nslots + 1, 256), dim3(256), 0, st, s, bits, stop);
    if ((e = scan_exclusive(bits, s.nslots + 1, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(each_tab_size_kernel, grid_threads(s.n + 1, 256), dim3(256), 0, st, s, bits, d_tab_off, stop);
    if ((e = scan_exclusive(d_tab_off, s.n + 1, sums, stop, st)) != hipSuccess) return e;
    const uint64_t bound_words = (s.n * 33u + s.nslots * 320u + 4) / 4;
    hipLaunchKernelGGL(each_zero_kernel, dim3(grid_for(bound_words, 256, 8)), dim3(256), 0, st, d_tab_off + s.n, d_out, cap, status, stop, tail);
    if (s.n + s.nslots)
        hipLaunchKernelGGL(each_tab_write_kernel, grid_threads(s.n + s.nslots, 256), dim3(256), 0, st, s, bits, d_tab_off, d_out, tail, stop);
    hipLaunchKernelGGL(each_tail_kernel, dim3(1), dim3(1), 0, st, d_tab_off + s.n, d_out, tail, stop);
    return hipGetLastError();
}

hipError_t launch_encode_each(const EncEachParams &p, void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const mhb::EncLayout L = mhb::enc_layout(p.n, p.total);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    auto *ubits = reinterpret_cast<unsigned long long *>(ws + L.off_units);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    auto *tail = reinterpret_cast<uint32_t *>(ws + L.off_tail);
    const uint64_t U = mhb::units_of(p.total, p.n);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(each_check_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p.in_off, p.n, p.total, status, stop);
    hipLaunchKernelGGL(each_enc_len_kernel, dim3(grid_for(U, WAVES, 2)), dim3(B_THREADS), 0, st, p, U, ubits, stop);
    if ((e = scan_exclusive(ubits, U, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(each_enc_sizes_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p, ubits, stop);
    if ((e = scan_exclusive(p.out_off, p.n + 1, sums, stop, st)) != hipSuccess) return e;
    const uint64_t bound_words = (p.total * 8u + p.n + 4) / 4;
    hipLaunchKernelGGL(each_zero_kernel, dim3(grid_for(bound_words, 256, 8)), dim3(256), 0, st, p.out_off + p.n, p.out, p.cap, status, stop, tail);
    hipLaunchKernelGGL(each_enc_emit_kernel, dim3(grid_for(U, WAVES, 2)), dim3(B_THREADS), 0, st, p, U, ubits, tail, stop);
    hipLaunchKernelGGL(each_tail_kernel, dim3(1), dim3(1), 0, st, p.out_off + p.n, p.out, tail, stop);
    return hipGetLastError();
}

hipError_t launch_decode_each(const DecEachParams &p, void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const mhb::DecLayout L = mhb::dec_layout(p.n);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(each_dec_check_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p, status, stop);
    if (p.index) {
        const uint64_t W = p.sym_total / (uint64_t(1) << p.chunk_shift) + p.n + 1;
        hipLaunchKernelGGL(each_dec_idx_kernel, dim3(grid_for(W, 256, 8)), dim3(256), 0, st, p, W, status, stop);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(each_dec_walk_kernel<false>, dim3(grid_for(p.n + 1, 256, 8)), dim3(256), 0, st, p, status, stop);
    if ((e = scan_exclusive(p.sym_off, p.n + 1, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(each_dec_walk_kernel<true>, dim3(grid_for(p.n + 1, 256, 8)), dim3(256), 0, st, p, status, stop);
    return hipGetLastError();
}

}  // namespace mhe
