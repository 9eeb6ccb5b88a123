// mh_limit_host.cpp — see mh_limit.hpp.  Host-side, integer-only, deterministic.
#include "mh_limit.hpp"

#include <algorithm>
#include <vector>

namespace mh {

namespace {

// Replaces the context's tree by the trie of the canonical code whose lengths package-merge gives for a limit of L bits.
// Same arithmetic, tie rule and node order as limit_recode_kernel (mh_limit.hip): the images of both builds are equal.
void recode_context(ContextCoder &c, const uint64_t *counts, int L) {
    // leaves in the order (count ascending, symbol ascending)
    int order[256], n = 0;
    for (int s = 0; s < 256; ++s)
        if (counts[s]) order[n++] = s;
    std::stable_sort(order, order + n, [&](int a, int b) { return counts[a] < counts[b]; });
    const int cap = 2 * n - 2;                       // only the first 2n - 2 items of a level can ever be selected
    // level 1 = the leaves; level j + 1 = leaves merged with the packages of level j, on equal weight a leaf first.
    // Kept per level: one flag per item (1 = package).
    std::vector<std::vector<uint8_t>> flag{size_t(L)};
    std::vector<uint64_t> prev, cur;
    prev.resize(size_t(n));
    for (int i = 0; i < n; ++i) prev[size_t(i)] = counts[order[i]];
    flag[0].assign(size_t(n), 0);
    for (int j = 1; j < L; ++j) {
        const size_t npk = prev.size() / 2;          // an odd last item pairs with nothing
        cur.clear();
        size_t a = 0, b = 0;
        while (int(cur.size()) < cap && (a < size_t(n) || b < npk)) {
            const uint64_t pw = b < npk ? prev[2 * b] + prev[2 * b + 1] : 0;
            const bool leaf = a < size_t(n) && (b >= npk || counts[order[a]] <= pw);
            cur.push_back(leaf ? counts[order[a]] : pw);
            flag[size_t(j)].push_back(leaf ? 0 : 1);
            if (leaf) ++a; else ++b;
        }
        prev.swap(cur);
    }
    // walk back: of the `take` first items of a level, the leaves give one bit to the symbols of the lowest ranks and the
    // p packages select the first 2p items of the level below
    int len_of_rank[256] = {0};
    size_t take = size_t(cap);
    for (int j = L - 1; j >= 0; --j) {
        const std::vector<uint8_t> &f = flag[size_t(j)];
        const size_t t = std::min(take, f.size());
        size_t p = 0;
        for (size_t i = 0; i < t; ++i) p += f[i];
        for (size_t r = 0; r < t - p; ++r) ++len_of_rank[r];
        take = 2 * p;
    }
    int len[256] = {0}, nlen[LIMIT_MAX_LEN + 2] = {0};
    for (int r = 0; r < n; ++r) { len[order[r]] = len_of_rank[r]; ++nlen[len_of_rank[r]]; }
    // the canonical trie.  At depth d the nodes are, in codeword order, nlen[d] leaves (symbols ascending) and then
    // inner[d] inner nodes; inner node k of depth d has the nodes 2k and 2k + 1 of depth d + 1 as children.
    // Node ids: leaves 0..n-1 in symbol order, then the inner nodes from the deepest level up, the root last.
    int inner[LIMIT_MAX_LEN + 2] = {0}, ibase[LIMIT_MAX_LEN + 2] = {0};
    inner[0] = 1;
    for (int d = 1; d <= L; ++d) inner[d] = 2 * inner[d - 1] - nlen[d];
    ibase[L] = n;
    for (int d = L - 1; d >= 0; --d) ibase[d] = ibase[d + 1] + inner[d + 1];
    const int nn = 2 * n - 1;
    std::vector<uint16_t> left(size_t(nn), 0xFFFF), right(size_t(nn), 0xFFFF);   // 0xFFFF on a leaf (ContextCoder::adopt)
    std::vector<uint8_t> sym(size_t(nn), 0);
    auto hang = [&](int id, int d, int x) {           // node x of depth d goes under inner node x / 2 of depth d - 1
        (x & 1 ? right : left)[size_t(ibase[d - 1] + (x >> 1))] = uint16_t(id);
    };
    int seen[LIMIT_MAX_LEN + 2] = {0}, id = 0;
    for (int s = 0; s < 256; ++s) {
        if (!counts[s]) continue;
        sym[size_t(id)] = uint8_t(s);
        hang(id++, len[s], seen[len[s]]++);
    }
    for (int d = L - 1; d >= 1; --d)
        for (int k = 0; k < inner[d]; ++k) hang(ibase[d] + k, d, nlen[d] + k);
    c.adopt(nn, nn - 1, left.data(), right.data(), sym.data());
}

}  // namespace

bool build_context_limited(ContextCoder &c, const uint64_t *counts, int max_len) {
    c.build_from_counts(counts);
    if (max_len <= 0 || c.max_len() <= max_len) return true;       // (a one-symbol context has depth 1)
    uint64_t total = 0;
    for (int s = 0; s < 256; ++s)
        if (counts[s] >= LIMIT_MAX_TOTAL || (total += counts[s]) >= LIMIT_MAX_TOTAL) { c.clear(); return false; }
    recode_context(c, counts, max_len);
    return true;
}

bool build_model_limited(Model &m, const uint64_t *counts, int order, int max_len) {
    m.build_from_counts(counts, order);                              // context weights, and every context's reference tree
    if (max_len <= 0) return true;
    bool ok = true;
    for (size_t i = 0; i < m.ctx.size(); ++i)
        if (m.ctx[i].max_len() > max_len) ok = build_context_limited(m.ctx[i], counts + 256 * i, max_len) && ok;
    return ok;
}

}  // namespace mh
