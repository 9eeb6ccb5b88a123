// mh_tree.hip — per-context Huffman tree build and table packing on the device.
//
//   tree_build_kernel   one wave per context: exact emulation of the reference's heap
//                       (src/min_pq.tpp:4-52) and merge rule (src/huffman.cpp:131-164), the heap held in
//                       LDS and every sift done lane-parallel, lane = heap level (LdsHeap); then all lanes derive
//                       depths, codewords (src/huffman.cpp:97-123) and the encode tables, and size the
//                       decode tables for every primary width.
//   tree_pack_kernel    one workgroup per context: fills the two decode-table levels and the walk tree
//                       for the layout the host picked from those sizes (same rule as Model::pack()).
//
// The result is bit-identical to the host build in mh_model.cpp (tests/test_gpu_parity.py compares the
// images); it exists so that histogram -> tables -> encode runs without the 512 KiB of counts going to
// the host and ~5 ms of host work in the middle of the pipeline.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mh_kernels.h"
#include "mh_model.hpp"

namespace mhk {

using mh::DEC16_LEAF;
using mh::DEC16_NULL;
using mh::TREE_LEAF;
using mh::TREE_STRIDE;

constexpr uint16_t NONE = 0xFFFF;

// ------------------------------------------------------------------------------------------------
// The reference's binary heap (src/min_pq.tpp:4-52), reproduced entry for entry with each sift done lane-parallel
// (lane = heap level) instead of comparison by comparison.  The heap lives in LDS, 1-based (root e[1], children of
// n at 2n and 2n + 1), one entry = key (32 bits when the context's total fits, else 64) + `item` = node id |
// subtree height << 16, so the merge loop (src/huffman.cpp:143-151) needs nothing back from memory.
// Why this gives the reference's array exactly: the comparisons never look at items, and along any root path the
// keys never decrease, so
//   * swim (:29-36, "parent STRICTLY greater"): the ancestors that move down are the bottom run of the root path
//     whose keys are > the new key — one compare per level, a ballot, and every level written at once;
//   * sink (:38-52): the path the hole takes is the chain of preferred children (right iff it exists and its key is
//     STRICTLY smaller than the left's), which depends on the heap before the sink only; the children that move up
//     are the top run of that path whose keys are < the sinking key.  The preferred-child bits of nodes 1..127 are
//     two ballots (nodes 128.. never have a right child), the path is a chase of those bits in scalar registers
//     (four instructions a level), and the rest is again one compare per level, a ballot and one write per level.
// Per heap operation: one LDS round trip for a swim, two for a sink, and no data-dependent branch.
// entries 1..256; a lane with no level to work on reads and writes back its own spare slot HEAP_SPARE + lane (> 256)
constexpr uint32_t HEAP_SPARE = 256, HEAP_SLOTS = 320;

template <bool K64>
struct LdsHeap {
    using Key = typename std::conditional<K64, unsigned long long, uint32_t>::type;
    struct alignas(K64 ? 16 : 8) Ent {
        Key key;
        uint32_t item;
    };
    Ent *e;
    uint32_t lane;
    uint32_t hn = 0;

    static __device__ __forceinline__ uint32_t uni(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
    static __device__ __forceinline__ Key uni_key(Key k) {
        if constexpr (K64) return (Key(uni(uint32_t(k >> 32))) << 32) | uni(uint32_t(k));
        else return uni(k);
    }

    // src/min_pq.tpp:4-7 + 29-36: append at n = hn, then the ancestors (lane l = level l, n >> (L - l)) whose keys
    // are STRICTLY greater move down one level each and the new entry takes the highest of their places
    __device__ __forceinline__ void push(Key k, uint32_t it) {
        const uint32_t n = ++hn;
        const uint32_t L = 31u - uint32_t(__builtin_clz(n));
        const uint32_t an = lane <= L ? n >> (L - lane) : HEAP_SPARE + lane;
        const Ent a = e[an];
        const Ent p = e[an >> 1];                                  // the entry above it (lane 0: e[0], unused)
        const uint32_t f = L - uint32_t(__popcll(__ballot(lane < L && a.key > k)));   // level where the entry rests
        // every lane writes, the lanes that keep their entry write it back: with a conditional write the compiler moves
        // the read of p behind the ballot (a second LDS round trip); selects field by field (of whole structs: scratch)
        const bool self = lane == f, down = lane > f && lane <= L;
        e[an] = Ent{self ? k : down ? p.key : a.key, self ? it : down ? p.item : a.item};
    }

    // src/min_pq.tpp:9-15 + 38-52: returns the minimum's item and key; the last entry sinks from the root
    __device__ __forceinline__ uint32_t pop(Key &mkey) {
        const Ent top = e[1];
        const Ent last = e[hn];
        --hn;
        // preferred-child bits of nodes n = lane and n = 64 + lane, for the heap without its last entry
        const Ent l0 = e[2u * lane], r0 = e[2u * lane + 1u], l1 = e[128u + 2u * lane], r1 = e[129u + 2u * lane];
        const unsigned long long pa = __ballot(2u * lane + 1u <= hn && r0.key < l0.key);
        const unsigned long long pb = __ballot(129u + 2u * lane <= hn && r1.key < l1.key);
        mkey = uni_key(top.key);
        const uint32_t titem = uni(top.item);
        if (hn == 0) return titem;
        // the path of the hole, chased to level 7 whatever the heap's depth: levels past the last occupied one are
        // never used (their nodes are > hn) and do not change the path above them
        uint32_t n = 1;
#pragma unroll
        for (int l = 0; l < 7; ++l) n = 2u * n + uint32_t(((l < 6 ? pa : pb) >> (n & 63u)) & 1u);
        // lane l = level l of the path: its entry, and (lanes 0..6) its child's on the path
        const uint32_t pn = lane < 8u ? n >> (7u - lane) : HEAP_SPARE + lane;
        const uint32_t cn = lane < 7u ? n >> (6u - lane) : pn;
        const Ent pe = e[pn];
        const Ent ce = e[cn];
        const uint32_t moves = uint32_t(__popcll(__ballot(lane >= 1u && pn <= hn && pe.key < last.key)));
        const bool up = lane < moves, here = lane == moves;        // (every lane writes: see push)
        e[pn] = Ent{up ? ce.key : here ? last.key : pe.key, up ? ce.item : here ? last.item : pe.item};
        return titem;
    }
};

struct TreeLds {
    uint16_t *left, *right, *parent, *height;
    uint8_t *sym;
    unsigned long long *weight;
    uint4 *heap;                                                       // HEAP_SLOTS entries of LdsHeap
};

// src/huffman.cpp:131-164 for one context: nleaf leaves are already laid out (ascending symbol order) in
// the node arrays.  Returns nn and the root through the two references; all lanes run the same scalar code
// and lane 0 writes the node arrays.
template <bool K64>
__device__ __forceinline__ void merge_context(const TreeLds &t, uint32_t nleaf, uint32_t lane, uint32_t &nn_out, uint32_t &root_out,
                                              uint32_t &single_out) {
    using Heap = LdsHeap<K64>;
    using Key = typename Heap::Key;
    Heap h{reinterpret_cast<typename Heap::Ent *>(t.heap), lane};
    for (uint32_t i = 0; i < nleaf; ++i) {                            // :134-138 ascending symbol order
        const unsigned long long w = t.weight[i];
        h.push(Key(w), i);                                             // height 0
    }
    uint32_t nn = nleaf;
    while (h.hn > 1) {                                                 // :143-151
        Key ka, kb;
        uint32_t a = h.pop(ka), b = h.pop(kb);
        if ((a >> 16) > (b >> 16)) {                                   // :147-149 the lower subtree goes left
            uint32_t x = a; a = b; b = x;
        }
        const unsigned long long w = (unsigned long long)(ka) + (unsigned long long)(kb);
        const uint32_t ha = a >> 16, hb = b >> 16, hnew = (ha > hb ? ha : hb) + 1u;
        const uint32_t ia = a & 0xFFFFu, ib = b & 0xFFFFu;
        if (lane == 0) {
            t.left[nn] = uint16_t(ia); t.right[nn] = uint16_t(ib); t.parent[nn] = NONE; t.sym[nn] = 0;
            t.weight[nn] = w; t.height[nn] = uint16_t(hnew);
            t.parent[ia] = t.parent[ib] = uint16_t(nn);
        }
        h.push(Key(w), nn | (hnew << 16));
        ++nn;
    }
    Key kr;
    const uint32_t root = h.pop(kr) & 0xFFFFu;                         // :152
    single_out = 0;
    if (nleaf == 1) {                                                  // :154-162 one-symbol context
        if (lane == 0) {
            const uint8_t s = t.sym[root];
            for (int k = 0; k < 2; ++k) {
                t.left[nn + k] = t.right[nn + k] = NONE; t.parent[nn + k] = uint16_t(root); t.height[nn + k] = 0; t.sym[nn + k] = s;
                t.weight[nn + k] = t.weight[root];
            }
            t.left[root] = uint16_t(nn); t.right[root] = uint16_t(nn + 1);
            t.height[root] = 1;
        }
        nn += 2;
        single_out = 1;
    }
    nn_out = nn;
    root_out = root;
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tree_build_kernel(const unsigned long long *__restrict__ counts, TreeBuildOut o) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    __shared__ unsigned long long cnt[256];
    __shared__ uint16_t left[TB_NODE_STRIDE], right[TB_NODE_STRIDE], parent[TB_NODE_STRIDE], height[TB_NODE_STRIDE];
    __shared__ uint8_t sym[TB_NODE_STRIDE];
    __shared__ unsigned long long weight[TB_NODE_STRIDE];
    __shared__ uint4 heap[HEAP_SLOTS];
    __shared__ uint8_t olen[256];
    __shared__ unsigned long long ocode[256];
    __shared__ uint32_t prof[9];
    __shared__ uint32_t s_nn, s_root, s_single, s_ntab8, s_maxlen;

    unsigned long long wsum = 0;
    for (uint32_t i = lane; i < 256; i += 64) {
        cnt[i] = counts[size_t(c) * 256 + i];
        wsum += cnt[i];
        olen[i] = 0;
        ocode[i] = 0;
    }
    for (int d = 32; d >= 1; d >>= 1) wsum += __shfl_xor(wsum, d);
    if (lane < 9) prof[lane] = 0;
    if (lane == 0) { s_ntab8 = 0; s_maxlen = 0; s_single = 0; }
    __syncthreads();

    // ---- leaves, in ascending symbol order (src/huffman.cpp:134-138): node id = rank among the non-zero counts
    uint32_t nleaf = 0;
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t s = i * 64 + lane;
        const bool nz = cnt[s] != 0;
        const unsigned long long m = __ballot(nz);
        const uint32_t pos = nleaf + __popcll(m & ((1ull << lane) - 1ull));
        if (nz) {
            left[pos] = right[pos] = NONE; parent[pos] = NONE; height[pos] = 0; sym[pos] = uint8_t(s); weight[pos] = cnt[s];
        }
        nleaf += __popcll(m);
    }
    __syncthreads();
    {
        const TreeLds t{left, right, parent, height, sym, weight, heap};
        uint32_t nn = 0, root = 0xFFFFFFFFu, single = 0;
        if (nleaf > 0) {
            // 32-bit keys when every weight that can appear (the root's is the context total) fits
            const bool wide = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(wsum >> 32)))) != 0;
            if (wide) merge_context<true>(t, nleaf, lane, nn, root, single);
            else merge_context<false>(t, nleaf, lane, nn, root, single);
        }
        if (lane == 0) { s_nn = nn; s_root = root; s_single = single; }
    }
    __syncthreads();

    const uint32_t nn = s_nn, root = s_root;
    if (root != 0xFFFFFFFFu) {
        for (uint32_t node = lane; node < nn; node += 64) {
            // walk up: depth, and for a leaf its codeword (last bit first)
            uint32_t d = 0;
            unsigned long long code = 0;
            uint32_t cur = node;
            while (cur != root) {
                const uint32_t p = parent[cur];
                if (right[p] == cur && d < 64) code |= 1ull << d;
                ++d;
                cur = p;
            }
            if (left[node] == NONE) {
                // in the one-symbol case the right leaf is visited last and wins (src/huffman.cpp:115)
                if (!(s_single && node == left[root])) {
                    olen[sym[node]] = uint8_t(d > 255 ? 255 : d);
                    ocode[sym[node]] = d <= 64 ? code : 0;
                    atomicMax(&s_maxlen, d);
                }
            } else if (d <= 8) {
                const uint32_t h = height[node] < o.hcap ? height[node] : o.hcap;
                atomicAdd(&prof[d], 1u << h);
                if (d == 8) atomicAdd(&s_ntab8, 1u);
            }
        }
    }
    __syncthreads();

    // ---- outputs
    uint32_t lenmask = 0;                    // bit l-1 for every code length l < 32 in use, bit 31 for longer ones
    for (uint32_t s = lane; s < 256; s += 64) {
        const uint32_t l = olen[s];
        if (l) lenmask |= 1u << (l < 32u ? l - 1u : 31u);
        const unsigned long long cd = ocode[s];
        o.len8[c * 256 + s] = uint8_t(l);
        o.code64[c * 256 + s] = cd;
        if (o.enc16) {                                       // order 0/1: the encoder's LDS images
            const uint32_t slot = mh::enc_slot((s << 8) | c);
            uint16_t e = 0;
            if (l > uint32_t(mh::ENC16_MAX_LEN)) e = mh::ENC16_ESCAPE;
            else if (l > 0) e = uint16_t((l << 12) | uint32_t(cd));
            o.enc16[slot] = e;
            o.len_slot[slot] = uint8_t(l);
        }
    }
    for (uint32_t i = lane; i < TB_NODE_STRIDE; i += 64) {
        const bool live = i < nn;
        o.node_left[c * TB_NODE_STRIDE + i] = live ? left[i] : NONE;
        o.node_right[c * TB_NODE_STRIDE + i] = live ? right[i] : NONE;
        o.node_sym[c * TB_NODE_STRIDE + i] = live ? sym[i] : 0;
        o.node_height[c * TB_NODE_STRIDE + i] = live ? uint8_t(height[i] > 255 ? 255 : height[i]) : 0;
    }
    for (int d = 32; d >= 1; d >>= 1) lenmask |= __shfl_xor(lenmask, d);
    if (lane == 0) {
        uint32_t *m = o.ctx_meta + c * TB_META_STRIDE;
        m[0] = nn; m[1] = root; m[2] = s_maxlen; m[3] = s_ntab8;
        for (int d = 0; d < 9; ++d) m[4 + d] = prof[d];
        m[13] = uint32_t(wsum); m[14] = uint32_t(wsum >> 32);
        m[15] = nleaf < 2 ? 0u : lenmask;                       // the 1-bit code of a one-symbol context does not count
    }
}

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tree_pack_body(const TreePackArgs &a, const uint32_t c) {
    const uint32_t tid = threadIdx.x;
    __shared__ uint16_t left[TB_NODE_STRIDE], right[TB_NODE_STRIDE], nid[TB_NODE_STRIDE];
    __shared__ uint8_t sym[TB_NODE_STRIDE], height[TB_NODE_STRIDE];
    __shared__ uint32_t tr[TREE_STRIDE];
    __shared__ uint32_t scan[256];
    const uint32_t *meta = a.ctx_meta + c * TB_META_STRIDE;
    const uint32_t nn = meta[0], root = meta[1];
    for (uint32_t i = tid; i < TB_NODE_STRIDE; i += 256) {
        left[i] = a.node_left[c * TB_NODE_STRIDE + i];
        right[i] = a.node_right[c * TB_NODE_STRIDE + i];
        sym[i] = a.node_sym[c * TB_NODE_STRIDE + i];
        height[i] = a.node_height[c * TB_NODE_STRIDE + i];
    }
    tr[tid] = 0;
    __syncthreads();
    const uint32_t P = a.P, nprim = 1u << P;
    const uint32_t my_base = a.sec_base_in ? a.sec_base_in[c] : a.sec_base_val[c];
    if (tid == 0 && !a.sec_base_in && a.sec_base) a.sec_base[c] = my_base;
    if (root == 0xFFFFFFFFu) {                       // empty context: null tables
        if (tid < nprim) a.prim[(c << P) | tid] = DEC16_NULL;
        if (a.tree) a.tree[c * TREE_STRIDE + tid] = 0;
        return;
    }
    if (tid == 0) {                                   // inner-node ids for the walk: root = 0, the rest in node order
        uint32_t next = 1;
        for (uint32_t i = 0; i < nn; ++i) nid[i] = (left[i] == NONE) ? NONE : (i == root ? 0 : uint16_t(next++));
    }
    __syncthreads();
    auto enc_child = [&](uint32_t ch) -> uint32_t { return left[ch] == NONE ? (TREE_LEAF | sym[ch]) : uint32_t(nid[ch]); };
    for (uint32_t i = tid; i < nn; i += 256)
        if (left[i] != NONE) tr[nid[i]] = (enc_child(right[i]) << 16) | enc_child(left[i]);

    // first level: thread w follows the P bits of w from the root
    uint32_t node = root, depth = 0, tabsize = 0, h = 0;
    if (tid < nprim) {
        while (depth < P && left[node] != NONE) {
            const uint32_t bit = a.lsb ? (tid >> depth) & 1u : (tid >> (P - 1 - depth)) & 1u;
            node = bit ? right[node] : left[node];
            ++depth;
        }
        if (left[node] != NONE) {                     // internal node at depth P
            h = a.direct ? a.H : (height[node] < a.hcap ? height[node] : a.hcap);
            tabsize = 1u << h;
        }
    }
    // exclusive prefix of the table sizes in w order (tables are laid out by increasing w)
    scan[tid] = tabsize;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        uint32_t v = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const uint32_t off = scan[tid] - tabsize;
    const uint32_t base = my_base;
    if (tid < nprim) {
        uint16_t e;
        if (left[node] == NONE) e = uint16_t(DEC16_LEAF | (depth << 8) | sym[node]);      // a leaf reached at depth <= P fills its whole range
        else if (a.direct) e = uint16_t((base >> a.H) + (off >> a.H));
        else e = uint16_t(((h - 1) << 12) | off);
        a.prim[(c << P) | tid] = e;
        // second level: this thread fills its own table
        for (uint32_t x = 0; x < tabsize; ++x) {
            uint32_t n2 = node, d2 = 0;
            while (d2 < h && left[n2] != NONE) {
                const uint32_t bit = a.lsb ? (x >> d2) & 1u : (x >> (h - 1 - d2)) & 1u;
                n2 = bit ? right[n2] : left[n2];
                ++d2;
            }
            a.sec[base + off + x] = left[n2] == NONE ? uint16_t(DEC16_LEAF | ((P + d2) << 8) | sym[n2]) : uint16_t(nid[n2]);
        }
    }
    __syncthreads();
    if (a.tree) a.tree[c * TREE_STRIDE + tid] = tr[tid];      // (a second packing of the same trees leaves the walk tree alone)
}

__global__ __launch_bounds__(256) void tree_pack_kernel(TreePackArgs a) { tree_pack_body(a, blockIdx.x); }
// [r4] two packings of the same trees in ONE launch (the chunk decoder's tables and the tile decoder's: blocks 0 .. nctx - 1
// and nctx .. 2 nctx - 1): they ran one after the other, 0.04 ms each, with nothing between them but a launch gap
__global__ __launch_bounds__(256) void tree_pack2_kernel(TreePackArgs a, TreePackArgs b, uint32_t nctx) {
    if (blockIdx.x < nctx) tree_pack_body(a, blockIdx.x);
    else tree_pack_body(b, blockIdx.x - nctx);
}

// ---- order 2: the live contexts' tables ("LDS codeword-table staging") --------------------------
// one wave per slot; the last block (slot == nslots) writes the encoder's all-escape row
__global__ __launch_bounds__(64) void o2_hot_pack_kernel(O2HotArgs a) {
    const uint32_t slot = blockIdx.x, lane = threadIdx.x;
    if (slot == a.nslots) { a.hot[slot * 64u + lane] = mh::ENC16_ESCAPE; return; }
    const uint32_t ctx = a.slot_ctx[slot];
    {   // encoder row: id of the symbol -> len << 12 | code, ENC16_ESCAPE for codes over 12 bits, id 63 and unused ids
        uint16_t e = mh::ENC16_ESCAPE;
        if (lane < 63 && a.id_used[lane]) {
            const uint32_t k = ctx * 256u + a.id_sym[lane];
            const uint32_t l = a.len8[k];
            e = l == 0 ? uint16_t(0) : (l > uint32_t(mh::ENC16_MAX_LEN) ? mh::ENC16_ESCAPE : uint16_t((l << 12) | uint32_t(a.code64[k])));
        }
        // stored at column id ^ (id of the context's second byte): the encoders read it there (bank spreading)
        a.hot[slot * 64u + (lane ^ a.slot_id1[slot])] = e;
    }
    if (!a.tprim) return;
    // tile decoder: first level of P bits (lane = window value, LSB-first), uniform second-level tables of 2^H entries;
    // entry = next slot << 16 | 0x8000 | length << 8 | symbol (leaf) or the table id (inner node at depth P)
    const uint32_t P = a.P, H = a.H;
    const uint16_t *left = a.node_left + size_t(ctx) * TB_NODE_STRIDE, *right = a.node_right + size_t(ctx) * TB_NODE_STRIDE;
    const uint8_t *sym = a.node_sym + size_t(ctx) * TB_NODE_STRIDE;
    const uint32_t root = a.ctx_meta[size_t(ctx) * TB_META_STRIDE + 1];
    auto leaf_entry = [&](uint32_t node, uint32_t len) -> uint32_t {
        const uint32_t s = sym[node];
        uint32_t nxt = a.ctx2slot[((ctx & 255u) << 8) | s];
        if (nxt == 0xFFFFu) nxt = 0;                              // no live context follows: only at the very end of a stream
        return (nxt << 16) | DEC16_LEAF | (len << 8) | s;
    };
    for (uint32_t w = lane; w < (1u << P); w += 64u) {            // (P <= 6: one pass)
        uint32_t node = root, depth = 0;
        if (root != 0xFFFFFFFFu)
            while (depth < P && left[node] != NONE) { node = ((w >> depth) & 1u) ? right[node] : left[node]; ++depth; }
        const bool inner = root != 0xFFFFFFFFu && left[node] != NONE;
        const unsigned long long m = __ballot(inner);
        const uint32_t rank = uint32_t(__popcll(m & ((1ull << lane) - 1ull)));
        const uint32_t id = (slot << P) + rank;                   // sparse ids: at most 2^P tables per slot
        uint32_t e = DEC16_NULL;
        if (root != 0xFFFFFFFFu) e = inner ? id : leaf_entry(node, depth);
        a.tprim[(slot << P) + (w ^ (slot & ((1u << P) - 1u)))] = e;       // stored at column w ^ slot: the decoder reads it there (bank spreading)
        if (inner) {
            for (uint32_t x = 0; x < (1u << H); ++x) {
                uint32_t n2 = node, d2 = 0;
                while (d2 < H && left[n2] != NONE) { n2 = ((x >> d2) & 1u) ? right[n2] : left[n2]; ++d2; }
                a.tsec[(size_t(id) << H) + x] = left[n2] == NONE ? leaf_entry(n2, P + d2) : 0u;   // deeper than P + H: unresolved (redo pass)
            }
        }
    }
}

hipError_t launch_o2_hot_pack(const O2HotArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(o2_hot_pack_kernel, dim3(a.nslots + 1), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_tree_build(const unsigned long long *d_counts, int nctx, const TreeBuildOut &o, hipStream_t st) {
    hipLaunchKernelGGL(tree_build_kernel, dim3(nctx), dim3(64), 0, st, d_counts, o);
    return hipGetLastError();
}

hipError_t launch_tree_pack(const TreePackArgs &a, int nctx, hipStream_t st) {
    hipLaunchKernelGGL(tree_pack_kernel, dim3(nctx), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_tree_pack2(const TreePackArgs &a, const TreePackArgs &b, int nctx, hipStream_t st) {
    hipLaunchKernelGGL(tree_pack2_kernel, dim3(2 * nctx), dim3(256), 0, st, a, b, uint32_t(nctx));
    return hipGetLastError();
}

}  // namespace mhk
