// mh_dict_host.cpp — the dictionary object of the C ABI (include/mh.h, "DICTIONARY SEARCH IN BATCHES"): Aho-Corasick over
// byte classes, turned into a full DFA with breadth-first state numbers, and the host matcher over it.  Host code only, no
// HIP: the device image is uploaded through mhd::g_upload (mh_api_find.cpp), and sanitize/fuzz_dict.cpp links this file alone.
#include "mh_dict.h"

#include <algorithm>
#include <new>

#include "../../include/mh.h"

namespace mhd {
int (*g_upload)(mh_dict *d) = nullptr;
void (*g_release)(mh_dict *d) = nullptr;
}  // namespace mhd

namespace {

inline uint8_t lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? uint8_t(c + 32) : c; }

// MH_OK, MH_ERR_ARG (a limit of the automaton) or MH_ERR_NOMEM (std::bad_alloc is the caller's)
int build(mh_dict &d, const uint8_t *bytes, const uint32_t *pat_off, size_t np, bool fold) {
    // classes: 0 for the bytes of no pattern, then the bytes in use in ascending order; folded, 'A'..'Z' take their twin's
    bool used[256] = {};
    for (uint32_t k = 0; k < pat_off[np]; ++k) used[fold ? lower(bytes[k]) : bytes[k]] = true;
    uint32_t ncls = 1;
    for (uint32_t c = 0; c < 256; ++c) d.cls[c] = used[c] ? uint8_t(ncls++) : 0;     // (at most 256 in use: class 256 cannot happen
    if (ncls > 256) {                                                                //  unless all are; then class 0 stays empty)
        ncls = 256;
        for (uint32_t c = 0; c < 256; ++c) d.cls[c] = uint8_t(c);                    // every byte its own class, none spare
    }
    if (fold)
        for (uint32_t c = 'A'; c <= 'Z'; ++c) d.cls[c] = d.cls[c + 32];
    // the trie, nodes in insertion order; child[node x ncls + cls], 0: none (the root is nobody's child)
    std::vector<uint32_t> child(ncls, 0), node_depth(1, 0);
    std::vector<std::vector<uint32_t>> ends(1);                  // the patterns that end in a node, ascending
    for (size_t j = 0; j < np; ++j) {
        uint32_t s = 0;
        for (uint32_t k = pat_off[j]; k < pat_off[j + 1]; ++k) {
            const uint32_t c = d.cls[fold ? lower(bytes[k]) : bytes[k]];
            uint32_t t = child[size_t(s) * ncls + c];
            if (!t) {
                t = uint32_t(node_depth.size());
                if (t >= MH_DICT_MAX_STATES) return MH_ERR_ARG;
                child.resize(child.size() + ncls, 0);
                child[size_t(s) * ncls + c] = t;
                node_depth.push_back(node_depth[s] + 1);
                ends.emplace_back();
            }
            s = t;
        }
        ends[s].push_back(uint32_t(j));
    }
    const uint32_t S = uint32_t(node_depth.size());
    // breadth-first numbers: order[new] = old, children in class order
    std::vector<uint32_t> order(1, 0), number(S, 0);
    order.reserve(S);
    for (uint32_t q = 0; q < order.size(); ++q)
        for (uint32_t c = 0; c < ncls; ++c)
            if (const uint32_t t = child[size_t(order[q]) * ncls + c]) { number[t] = uint32_t(order.size()); order.push_back(t); }
    // the DFA in that order: a state's fail state is shallower, so its row and its outputs are complete
    std::vector<uint32_t> go(size_t(S) * ncls, 0), fail(S, 0);
    std::vector<std::vector<uint32_t>> outs(S);
    size_t n_out = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t old = order[s], f = fail[s];
        for (uint32_t c = 0; c < ncls; ++c) {
            const uint32_t t = child[size_t(old) * ncls + c];
            if (t) {
                go[size_t(s) * ncls + c] = number[t];
                fail[number[t]] = s ? go[size_t(f) * ncls + c] : 0;
            } else {
                go[size_t(s) * ncls + c] = s ? go[size_t(f) * ncls + c] : 0;
            }
        }
        outs[s] = ends[old];
        if (s && !outs[f].empty()) {                             // the dictionary-suffix chain, merged by pattern number
            std::vector<uint32_t> merged(outs[s].size() + outs[f].size());
            std::merge(outs[s].begin(), outs[s].end(), outs[f].begin(), outs[f].end(), merged.begin());
            outs[s].swap(merged);
        }
        n_out += outs[s].size();
        if (n_out > MH_DICT_MAX_OUTPUTS) return MH_ERR_ARG;
    }
    d.ncls = ncls;
    d.states = S;
    d.trans.resize(size_t(S) * ncls);
    for (size_t k = 0; k < d.trans.size(); ++k) d.trans[k] = uint16_t(go[k] | (outs[go[k]].empty() ? 0u : 0x8000u));
    d.depth.resize(S);
    d.out_off.resize(size_t(S) + 1);
    d.out_pat.reserve(n_out);
    d.out_len.reserve(n_out);
    for (uint32_t s = 0; s < S; ++s) {
        d.depth[s] = uint8_t(node_depth[order[s]]);
        d.out_off[s] = uint32_t(d.out_pat.size());
        for (const uint32_t j : outs[s]) {
            d.out_pat.push_back(j);
            d.out_len.push_back(uint8_t(pat_off[j + 1] - pat_off[j]));
        }
    }
    d.out_off[S] = uint32_t(d.out_pat.size());
    return MH_OK;
}

}  // namespace

extern "C" {

int mh_dict_create(const uint8_t *bytes, const uint32_t *pat_off, size_t n_patterns, uint32_t flags, mh_dict **out) {
    if (out) *out = nullptr;
    if (!bytes || !pat_off || !out || n_patterns == 0 || n_patterns > MH_DICT_MAX_PATTERNS || (flags & ~MH_FIND_FOLD_ASCII)) return MH_ERR_ARG;
    if (pat_off[0] != 0) return MH_ERR_ARG;
    uint32_t max_len = 0;
    for (size_t j = 0; j < n_patterns; ++j) {
        if (pat_off[j + 1] <= pat_off[j] || pat_off[j + 1] - pat_off[j] > MH_DICT_MAX_LEN) return MH_ERR_ARG;   // empty, decreasing, too long
        max_len = std::max(max_len, pat_off[j + 1] - pat_off[j]);
    }
    mh_dict *d = new (std::nothrow) mh_dict;
    if (!d) return MH_ERR_NOMEM;
    d->n = uint32_t(n_patterns);
    d->max_len = max_len;
    d->flags = flags;
    int rc;
    try {
        rc = build(*d, bytes, pat_off, n_patterns, (flags & MH_FIND_FOLD_ASCII) != 0);
    } catch (const std::bad_alloc &) {
        rc = MH_ERR_NOMEM;
    }
    if (rc == MH_OK && mhd::g_upload) rc = mhd::g_upload(d);
    if (rc != MH_OK) {
        mh_dict_free(d);
        return rc;
    }
    *out = d;
    return MH_OK;
}

void mh_dict_free(mh_dict *d) {
    if (d && d->d_image && mhd::g_release) mhd::g_release(d);
    delete d;
}

size_t mh_dict_size(const mh_dict *d) { return d ? d->n : 0; }
int mh_dict_max_len(const mh_dict *d) { return d ? int(d->max_len) : 0; }
size_t mh_dict_states(const mh_dict *d) { return d ? d->states : 0; }
int mh_dict_classes(const mh_dict *d) { return d ? int(d->ncls) : 0; }
size_t mh_dict_device_bytes(const mh_dict *d) { return d ? mhd::dict_image(d->states, d->ncls, d->out_pat.size()).total : 0; }

int mh_dict_find_bytes(const mh_dict *d, const uint8_t *data, size_t n, uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap,
                       uint64_t *n_hits) {
    if (n_hits) *n_hits = 0;
    if (!d || !n_hits || (!data && n)) return MH_ERR_ARG;
    uint64_t r = 0;
    uint32_t s = 0;
    for (size_t k = 0; k < n; ++k) {
        const uint16_t t = d->trans[size_t(s) * d->ncls + d->cls[data[k]]];
        s = t & 0x7FFFu;
        if (!(t & 0x8000u)) continue;
        for (uint32_t q = d->out_off[s]; q < d->out_off[s + 1]; ++q, ++r) {
            if (r >= hit_cap) continue;
            if (hits) { hits[2 * r] = k + 1 - d->out_len[q]; hits[2 * r + 1] = k + 1; }
            if (hit_pattern) hit_pattern[r] = d->out_pat[q];
        }
    }
    *n_hits = r;
    return (hits || hit_pattern) && r > hit_cap ? MH_ERR_CAPACITY : MH_OK;
}

}  // extern "C"
