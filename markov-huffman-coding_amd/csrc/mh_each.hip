// mh_each.hip — batches of independent order-0/1 streams, each under its own model (include/mh.h, "BATCHES OF STREAMS, ONE
// MODEL EACH"): the reference's default per-file flow (train, write the table, encode) for N messages in a fixed number of
// launches.  Layouts: mh_each.h; shared device code: mh_batch_dev.hpp (units and their finder, scans, the model-free encode
// stages, bit writer); the trees are built by mh_tree.hip's tree_build_kernel over the live (stream, context) pairs, so the
// reference's tie-breaking has one copy.
//   batch_check_kernel      (mh_batch_dev.hpp) offsets non-decreasing, [0] == 0, [n] == total
//   each_live_kernel        one wave per (stream, 1 KiB sub-step): the contexts the sub-step's symbols are coded in, OR-ed
//                           into the stream's 256-bit mask (order 1: prev0 and every byte but the stream's last)
//   each_nlive_kernel       one thread per stream: its live contexts (scanned next into slot bases)
//   each_slotmap_kernel     one thread per (stream, context): context -> slot map, slot -> (stream, context)
//   each_hist_kernel        one wave per (stream, 1 KiB sub-step): counts into the slot rows (global atomics)
//   tree_build_kernel       (mh_tree.hip, unchanged) one wave per slot: the tree and the codes of one (stream, live context)
//   each_pack_kernel        one wave per slot: first level and walk tree from the tree's nodes
//   each_tab_*              table files: bits per slot (scanned), bytes per stream (scanned), the pre-order traversal of
//                           every tree by one lane (src/huffman.cpp:174-188, src/markov_huffman.cpp:80-88)
//                           batch_zero_kernel and batch_tail_kernel (mh_batch_dev.hpp) around the writer, as in the encoder
//   each_enc_*              mh_batch.hip's len and emit kernels with the codes of stream i's slots (L2) instead of one LDS
//                           image, between the same model-free stages (mh_batch_dev.hpp)
// The decoder is mh_batch.hip's dec_*_kernel<Model::Set> (mhb::launch_decode): stream i's first level and walk tree from L2.
// Every loop is bounded by a symbol count, a leaf count, 64 code bits or nbits_i.  The number of launches does not depend on n,
// except for one more tree_build_kernel launch per 4 M live contexts (TREE_SLICE).
#include "mh_each.h"
#include "mh_batch_dev.hpp"
#include "../../include/mh.h"

namespace mhe {

using mhb::B_THREADS;
using mhb::B_VEC;
constexpr uint16_t NONE = 0xFFFF;                // (mh_tree.hip: a node without children)

namespace {

using mhb::batch_check_kernel;
using mhb::batch_enc_sizes_kernel;
using mhb::batch_tail_kernel;
using mhb::batch_zero_kernel;
using mhb::byte_of;
using mhb::grid_for;
using mhb::grid_threads;
using mhb::gtid;
using mhb::scan_exclusive;
using mhb::stopped;
using mhb::Unit;

constexpr uint32_t WAVES = B_THREADS / 64;
constexpr uint64_t TREE_SLICE = 1u << 22;          // slots per tree_build_kernel launch: 2^22 x TB_NODE_STRIDE < 2^32
static_assert((TREE_SLICE - 1) * mhk::TB_NODE_STRIDE + mhk::TB_NODE_STRIDE <= (1ull << 32), "tree_build_kernel's 32-bit node offsets");

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
        if (!mhb::unit_of<1>(data, in_off, n, prev0, u, l)) continue;             // wave-uniform
        unsigned long long m[4] = {0, 0, 0, 0};
        if (l.cnt) mark(m, l.ctx);                                        // the context of the lane's first symbol
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
        if (!mhb::unit_of<1>(data, in_off, s.n, prev0, u, l)) continue;
        const uint32_t *row = s.ctx_slot + l.i * 256u;
        uint32_t prev = l.ctx;
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
        if (mhb::unit_of<1>(p.data, p.in_off, p.n, p.prev0, u, l) && l.cnt) {
            const uint32_t *row = p.set.ctx_slot + l.i * 256u;
            const bool o1 = p.set.type[l.i] != 0;
            uint32_t prev = l.ctx;
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

__global__ __launch_bounds__(B_THREADS) void each_enc_emit_kernel(EncEachParams p, uint64_t nunits, const unsigned long long *ubase,
                                                                  uint32_t *tail, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t bytes = p.out_off[p.n];
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint64_t nw = uint64_t(gridDim.x) * WAVES;
    for (uint64_t u = uint64_t(blockIdx.x) * WAVES + threadIdx.x / 64; u < nunits; u += nw) {
        Unit l;
        if (!mhb::unit_of<1>(p.data, p.in_off, p.n, p.prev0, u, l)) continue;     // wave-uniform
        const uint32_t *row = p.set.ctx_slot + l.i * 256u;
        const bool o1 = p.set.type[l.i] != 0;
        uint32_t bits = 0, prev = l.ctx;
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
            p.index[(l.a >> p.chunk_shift) + l.i + (l.j0 >> p.chunk_shift)] = (uint64_t(l.ctx) << 56) | sbit;
        if (!bits) continue;
        mhb::BitWriter bw;
        bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[l.i]) * 8u + sbit);
#pragma unroll
        for (uint32_t t = 0; t < B_VEC; ++t) bw.code(codes[t], lens[t]);
        bw.finish();
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
    hipLaunchKernelGGL(batch_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, d_in_off, n, total, status, stop);
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
    hipLaunchKernelGGL(batch_zero_kernel, dim3(grid_for(bound_words, 256, 8)), dim3(256), 0, st, d_tab_off + s.n, d_out, cap, status, stop, tail);
    if (s.n + s.nslots)
        hipLaunchKernelGGL(each_tab_write_kernel, grid_threads(s.n + s.nslots, 256), dim3(256), 0, st, s, bits, d_tab_off, d_out, tail, stop);
    hipLaunchKernelGGL(batch_tail_kernel, dim3(1), dim3(1), 0, st, d_tab_off + s.n, d_out, tail, stop);
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
    hipLaunchKernelGGL(batch_check_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p.in_off, p.n, p.total, status, stop);
    hipLaunchKernelGGL(each_enc_len_kernel, dim3(grid_for(U, WAVES, 2)), dim3(B_THREADS), 0, st, p, U, ubits, stop);
    if ((e = scan_exclusive(ubits, U, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(batch_enc_sizes_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p.in_off, p.n, ubits, p.nbits, p.out_off, stop);
    if ((e = scan_exclusive(p.out_off, p.n + 1, sums, stop, st)) != hipSuccess) return e;
    const uint64_t bound_words = (p.total * 8u + p.n + 4) / 4;
    hipLaunchKernelGGL(batch_zero_kernel, dim3(grid_for(bound_words, 256, 8)), dim3(256), 0, st, p.out_off + p.n, p.out, p.cap, status, stop, tail);
    hipLaunchKernelGGL(each_enc_emit_kernel, dim3(grid_for(U, WAVES, 2)), dim3(B_THREADS), 0, st, p, U, ubits, tail, stop);
    hipLaunchKernelGGL(batch_tail_kernel, dim3(1), dim3(1), 0, st, p.out_off + p.n, p.out, tail, stop);
    return hipGetLastError();
}

}  // namespace mhe
