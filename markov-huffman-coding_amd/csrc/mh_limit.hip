// mh_limit.hip — length-limited models on the device (mh_limit.hpp).
//
//   limit_recode_kernel   one wave per context, launched behind tree_build_kernel on the same stream: a context whose
//                         reference tree is deeper than the limit is re-coded by package-merge with canonical codewords and
//                         its part of tree_build_kernel's outputs is rewritten in place; every other wave exits at once.
//
// The result is bit-identical to the host build in mh_limit_host.cpp (tests/test_gpu_limit.py compares the images).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_limit.hpp"

namespace mhk {

constexpr uint16_t NONE = 0xFFFF;

// What tree_build_kernel (mh_tree.hip) does once a context's tree stands in the LDS node arrays, restated here statement for
// statement (that file's bytes are pinned by the committed counter figures): every lane derives depths and codewords
// (src/huffman.cpp:97-123) for its nodes, then the wave writes the context's part of every image and its sizes.
// olen, ocode, prof and the three scalars are zero on entry.  tests/test_gpu_limit.py compares every image with the host's.
struct TreeLds {
    uint16_t *left, *right, *parent, *height;
    uint8_t *sym;
};
struct TreeDerived {
    uint8_t *olen;
    unsigned long long *ocode;
    uint32_t *prof, *single, *ntab8, *maxlen;
};
__device__ __forceinline__ void derive_and_store(const TreeLds &t, const TreeDerived &x, const TreeBuildOut &o, uint32_t c, uint32_t lane,
                                                 uint32_t nn, uint32_t root, uint32_t nleaf, unsigned long long wsum) {
    if (root != 0xFFFFFFFFu) {
        for (uint32_t node = lane; node < nn; node += 64) {
            // walk up: depth, and for a leaf its codeword (last bit first)
            uint32_t d = 0;
            unsigned long long code = 0;
            uint32_t cur = node;
            while (cur != root) {
                const uint32_t p = t.parent[cur];
                if (t.right[p] == cur && d < 64) code |= 1ull << d;
                ++d;
                cur = p;
            }
            if (t.left[node] == NONE) {
                // in the one-symbol case the right leaf is visited last and wins (src/huffman.cpp:115)
                if (!(*x.single && node == t.left[root])) {
                    x.olen[t.sym[node]] = uint8_t(d > 255 ? 255 : d);
                    x.ocode[t.sym[node]] = d <= 64 ? code : 0;
                    atomicMax(x.maxlen, d);
                }
            } else if (d <= 8) {
                const uint32_t h = t.height[node] < o.hcap ? t.height[node] : o.hcap;
                atomicAdd(&x.prof[d], 1u << h);
                if (d == 8) atomicAdd(x.ntab8, 1u);
            }
        }
    }
    __syncthreads();

    // ---- outputs
    uint32_t lenmask = 0;                    // bit l-1 for every code length l < 32 in use, bit 31 for longer ones
    for (uint32_t s = lane; s < 256; s += 64) {
        const uint32_t l = x.olen[s];
        if (l) lenmask |= 1u << (l < 32u ? l - 1u : 31u);
        const unsigned long long cd = x.ocode[s];
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
        o.node_left[c * TB_NODE_STRIDE + i] = live ? t.left[i] : NONE;
        o.node_right[c * TB_NODE_STRIDE + i] = live ? t.right[i] : NONE;
        o.node_sym[c * TB_NODE_STRIDE + i] = live ? t.sym[i] : 0;
        o.node_height[c * TB_NODE_STRIDE + i] = live ? uint8_t(t.height[i] > 255 ? 255 : t.height[i]) : 0;
    }
    for (int d = 32; d >= 1; d >>= 1) lenmask |= __shfl_xor(lenmask, d);
    if (lane == 0) {
        uint32_t *m = o.ctx_meta + c * TB_META_STRIDE;
        m[0] = nn; m[1] = root; m[2] = *x.maxlen; m[3] = *x.ntab8;
        for (int d = 0; d < 9; ++d) m[4 + d] = x.prof[d];
        m[13] = uint32_t(wsum); m[14] = uint32_t(wsum >> 32);
        m[15] = nleaf < 2 ? 0u : lenmask;                       // the 1-bit code of a one-symbol context does not count
    }
}

// ------------------------------------------------------------------------------------------------
// Length-limited models: one wave per context; a context whose reference tree (tree_build_kernel ran
// before on the same stream) has no code over `maxbits` exits at once.  The others are re-coded as a whole, all state in
// LDS and registers:
//   1. the live symbols sorted by (count, symbol): every lane ranks its (at most 4) leaves against all others, in one pass
//      over the leaves (each a broadcast LDS read);
//   2. package-merge, level by level: level 1 = the leaves; level j + 1 = the leaves merged with the packages (pairs of
//      consecutive items) of level j.  Both lists are sorted, so an item's place is its own index plus its rank in the other
//      list, a binary search: packages of strictly smaller weight for a leaf, leaves of smaller OR EQUAL weight for a
//      package (on equal weight a leaf goes first).  Only the first 2n - 2 items of a level can ever be selected: the rest
//      is dropped, and what is kept per level is one flag bit per item (1 = package), 512 bits;
//   3. the walk back from level `maxbits`: of the first `take` items the leaves give one bit to the symbols of the lowest
//      ranks and the p packages select the first 2p items of the level below (a masked popcount of the level's flags);
//   4. canonical codewords by (length, symbol), as the trie they form: at depth d the nodes are, in codeword order, the
//      leaves of length d and then the inner nodes, and inner node k has the nodes 2k and 2k + 1 of depth d + 1 as children.
//      Node ids: leaves in symbol order, then the inner nodes from the deepest level up, the root last (the order of
//      mh::build_context_limited: tree_pack_kernel numbers the walk tree by node id);
//   5. the same derivation and stores as the reference build (derive_and_store), over that context's part of every image.
// A context whose counts add up to 2^56 or more (package weights would not fit 64 bits) is left as it is: the host sees
// its length over the limit in ctx_meta and refuses the model.
constexpr uint32_t LIM_ITEMS = 512;                      // 2n - 2 <= 510 items of a level
__global__ __launch_bounds__(64) void limit_recode_kernel(const unsigned long long *__restrict__ counts, TreeBuildOut o, uint32_t maxbits) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    if (o.ctx_meta[c * TB_META_STRIDE + 2] <= maxbits) return;
    __shared__ unsigned long long cnt[256];
    __shared__ uint16_t left[TB_NODE_STRIDE], right[TB_NODE_STRIDE], parent[TB_NODE_STRIDE], height[TB_NODE_STRIDE];
    __shared__ uint8_t sym[TB_NODE_STRIDE];
    __shared__ uint8_t olen[256];
    __shared__ unsigned long long ocode[256];
    __shared__ uint32_t prof[9];
    __shared__ uint32_t s_single, s_ntab8, s_maxlen;
    __shared__ unsigned long long lw[256];               // leaf weights in sorted order
    __shared__ unsigned long long item[2][LIM_ITEMS];    // the weights of two consecutive levels
    __shared__ uint32_t flag[mh::LIMIT_MAX_LEN][LIM_ITEMS / 32];
    __shared__ uint16_t level_items[mh::LIMIT_MAX_LEN];
    __shared__ uint8_t leaf_of_rank[256], leaf_len[256];
    __shared__ uint32_t nlen[mh::LIMIT_MAX_LEN + 2], ninner[mh::LIMIT_MAX_LEN + 2], ibase[mh::LIMIT_MAX_LEN + 2];
    __shared__ uint32_t s_complete;

    unsigned long long wsum = 0;
    bool big = false;
    for (uint32_t i = lane; i < 256; i += 64) {
        cnt[i] = counts[size_t(c) * 256 + i];
        big |= cnt[i] >= mh::LIMIT_MAX_TOTAL;
        wsum += cnt[i];
        olen[i] = 0;
        ocode[i] = 0;
    }
    for (int d = 32; d >= 1; d >>= 1) wsum += __shfl_xor(wsum, d);
    if (__ballot(big) != 0ull || wsum >= mh::LIMIT_MAX_TOTAL) return;       // (wave-uniform)
    if (lane < 9) prof[lane] = 0;
    if (lane == 0) { s_ntab8 = 0; s_maxlen = 0; s_single = 0; }
    for (uint32_t i = lane; i < mh::LIMIT_MAX_LEN * (LIM_ITEMS / 32); i += 64) (&flag[0][0])[i] = 0;
    for (uint32_t i = lane; i < mh::LIMIT_MAX_LEN + 2; i += 64) nlen[i] = 0;
    __syncthreads();

    // ---- leaves: node id = rank among the non-zero counts (ascending symbol order, as in tree_build_kernel)
    uint32_t n = 0;
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t s = i * 64 + lane;
        const bool nz = cnt[s] != 0;
        const unsigned long long m = __ballot(nz);
        const uint32_t pos = n + __popcll(m & ((1ull << lane) - 1ull));
        if (nz) { left[pos] = right[pos] = NONE; height[pos] = 0; sym[pos] = uint8_t(s); item[1][pos] = cnt[s]; }   // (item[1]: free until level 2)
        n += __popcll(m);
    }
    __syncthreads();
    // (a tree deeper than 8 has at least 10 leaves: n >= 2 from here on)
    const uint32_t cap = 2u * n - 2u;

    // ---- 1. sort by (count, symbol): one pass over the leaves, each read once (a broadcast) and ranked against this lane's four
    {
        unsigned long long w4[4];
        uint32_t r4[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) w4[k] = lane + 64u * k < n ? item[1][lane + 64u * k] : 0ull;
        for (uint32_t j = 0; j < n; ++j) {
            const unsigned long long wj = item[1][j];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) r4[k] += (wj < w4[k] || (wj == w4[k] && j < lane + 64u * k)) ? 1u : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (lane + 64u * k < n) {
                lw[r4[k]] = w4[k];
                item[0][r4[k]] = w4[k];
                leaf_of_rank[r4[k]] = uint8_t(lane + 64u * k);
            }
    }
    if (lane == 0) level_items[0] = uint16_t(n);
    __syncthreads();

    // ---- 2. levels 2 .. maxbits
    uint32_t have = n;                                   // items of the level below
    for (uint32_t j = 1; j < maxbits; ++j) {
        const unsigned long long *prev = item[(j - 1) & 1];
        unsigned long long *cur = item[j & 1];
        const uint32_t npk = have >> 1;                  // an odd last item pairs with nothing
        for (uint32_t a = lane; a < n; a += 64) {
            const unsigned long long w = lw[a];
            uint32_t lo = 0, hi = npk;                   // packages of strictly smaller weight
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (prev[2 * mid] + prev[2 * mid + 1] < w) lo = mid + 1; else hi = mid;
            }
            if (a + lo < cap) cur[a + lo] = w;
        }
        for (uint32_t b = lane; b < npk; b += 64) {
            const unsigned long long w = prev[2 * b] + prev[2 * b + 1];
            uint32_t lo = 0, hi = n;                     // leaves of smaller or equal weight
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (lw[mid] <= w) lo = mid + 1; else hi = mid;
            }
            const uint32_t pos = b + lo;
            if (pos < cap) {
                cur[pos] = w;
                atomicOr(&flag[j][pos >> 5], 1u << (pos & 31u));
            }
        }
        have = n + npk < cap ? n + npk : cap;
        if (lane == 0) level_items[j] = uint16_t(have);
        __syncthreads();
    }

    // ---- 3. the walk back; this lane holds the lengths of the ranks lane, lane + 64, lane + 128, lane + 192
    uint32_t len_r[4] = {0, 0, 0, 0};
    uint32_t take = cap;
    for (int j = int(maxbits) - 1; j >= 0; --j) {
        const uint32_t lv = level_items[j];
        const uint32_t t = take < lv ? take : lv;
        uint32_t pc = 0;
        if (lane < LIM_ITEMS / 32) {
            const uint32_t first = lane * 32u;
            const uint32_t mask = t >= first + 32u ? 0xFFFFFFFFu : (t > first ? (1u << (t - first)) - 1u : 0u);
            pc = uint32_t(__popc(flag[j][lane] & mask));
        }
        for (int d = 8; d >= 1; d >>= 1) pc += __shfl_xor(pc, d);
        const uint32_t p = uint32_t(__builtin_amdgcn_readfirstlane(int(pc)));
        const uint32_t a = t - p;                        // leaves among the items taken
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) len_r[k] += (lane + 64u * k < a) ? 1u : 0u;
        take = 2u * p;
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t r = lane + 64u * k;
        if (r < n) {
            leaf_len[leaf_of_rank[r]] = uint8_t(len_r[k]);
            atomicAdd(&nlen[len_r[k]], 1u);
        }
    }
    __syncthreads();

    // ---- 4. the canonical trie
    if (lane == 0) {
        ninner[0] = 1;
        for (uint32_t d = 1; d <= maxbits; ++d) ninner[d] = 2u * ninner[d - 1] - nlen[d];
        ibase[maxbits] = n;
        for (uint32_t d = maxbits; d-- > 0;) ibase[d] = ibase[d + 1] + ninner[d + 1];
        // a complete code has n - 1 inner nodes, none at the last level; anything else would index past the node arrays
        uint32_t total = 0, bad = nlen[0] | ninner[maxbits];
        for (uint32_t d = 0; d < maxbits; ++d) { bad |= ninner[d] > 255u ? 1u : 0u; total += ninner[d] <= 255u ? ninner[d] : 0u; }
        s_complete = (bad == 0 && total == n - 1u) ? 1u : 0u;
    }
    __syncthreads();
    if (!s_complete) return;                             // (never: the lengths' Kraft sum is 1) the context stays as it was, which the host refuses
    const uint32_t root = 2u * n - 2u, nn = 2u * n - 1u;
    // node x of depth d hangs under inner node x / 2 of depth d - 1
    auto hang = [&](uint32_t id, uint32_t d, uint32_t x) {
        const uint32_t p = ibase[d - 1] + (x >> 1);
        parent[id] = uint16_t(p);
        if (x & 1u) right[p] = uint16_t(id); else left[p] = uint16_t(id);
    };
    {   // a leaf's place among the leaves of its length (symbols ascending): again one pass, this lane's four against each
        uint32_t l4[4], x4[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) l4[k] = lane + 64u * k < n ? leaf_len[lane + 64u * k] : 0xFFFFu;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t lj = leaf_len[j];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) x4[k] += (j < lane + 64u * k && lj == l4[k]) ? 1u : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (lane + 64u * k < n) hang(lane + 64u * k, l4[k], x4[k]);
    }
    for (uint32_t d = 0; d < maxbits; ++d)
        for (uint32_t k = lane; k < ninner[d]; k += 64) {
            const uint32_t id = ibase[d] + k;
            sym[id] = 0;
            if (d == 0) parent[id] = NONE; else hang(id, d, nlen[d] + k);
        }
    __syncthreads();
    // lengths never shrink along the codeword order: the deepest leaf under a node is its rightmost
    for (uint32_t id = n + lane; id < nn; id += 64) {
        uint32_t h = 0;
        for (uint32_t cur = id; right[cur] != NONE; cur = right[cur]) ++h;
        height[id] = uint16_t(h);
    }
    __syncthreads();

    // ---- 5.
    const TreeLds t{left, right, parent, height, sym};
    derive_and_store(t, TreeDerived{olen, ocode, prof, &s_single, &s_ntab8, &s_maxlen}, o, c, lane, nn, root, n, wsum);
}

hipError_t launch_tree_limit(const unsigned long long *d_counts, int nctx, uint32_t max_len, const TreeBuildOut &o, hipStream_t st) {
    hipLaunchKernelGGL(limit_recode_kernel, dim3(nctx), dim3(64), 0, st, d_counts, o, max_len);
    return hipGetLastError();
}

}  // namespace mhk
