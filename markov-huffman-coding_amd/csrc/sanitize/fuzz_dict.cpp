// fuzz_dict — random small-alphabet dictionaries through mh_dict_create and mh_dict_find_bytes against a naive matcher, under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Links mh_dict_host.cpp alone (no HIP, no device): `make fuzz_dict`.
//   fuzz_dict CASES SEED   ->  "<cases> cases, <hits> hits, <mismatches> mismatches"; exit 1 on a mismatch
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "../../../include/mh.h"

namespace {

uint8_t fold(uint8_t c) { return c >= 'A' && c <= 'Z' ? uint8_t(c + 32) : c; }

struct Hit {
    uint64_t begin, end;
    uint32_t pattern;
    bool operator==(const Hit &o) const { return begin == o.begin && end == o.end && pattern == o.pattern; }
};

// every occurrence of every pattern, ascending (end, pattern)
std::vector<Hit> naive(const std::vector<std::vector<uint8_t>> &pats, const std::vector<uint8_t> &text, bool folded) {
    std::vector<Hit> out;
    for (size_t end = 1; end <= text.size(); ++end)
        for (size_t j = 0; j < pats.size(); ++j) {
            const size_t len = pats[j].size();
            if (len > end) continue;
            bool same = true;
            for (size_t k = 0; k < len && same; ++k) {
                const uint8_t a = pats[j][k], b = text[end - len + k];
                same = folded ? fold(a) == fold(b) : a == b;
            }
            if (same) out.push_back(Hit{end - len, end, uint32_t(j)});
        }
    return out;
}

}  // namespace

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 2000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    auto below = [&](uint64_t n) { return rng() % n; };
    const uint8_t letters[] = {'a', 'A', 'b', 'B', 'z', 0, 255, '['};
    uint64_t hits_seen = 0, mismatches = 0;
    for (long c = 0; c < cases; ++c) {
        const size_t alpha = 1 + below(sizeof letters);
        const bool folded = below(3) == 0;
        const size_t np = 1 + below(c % 50 == 0 ? 200 : 12);
        const size_t max_len = c % 97 == 0 ? MH_DICT_MAX_LEN : 1 + below(8);
        std::vector<std::vector<uint8_t>> pats(np);
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> off(1, 0);
        for (auto &p : pats) {
            p.resize(1 + below(max_len));
            for (auto &b : p) b = letters[below(alpha)];
            bytes.insert(bytes.end(), p.begin(), p.end());
            off.push_back(uint32_t(bytes.size()));
        }
        std::vector<uint8_t> text(below(c % 97 == 0 ? 2000 : 300));
        for (auto &b : text) b = letters[below(alpha)];
        mh_dict *d = nullptr;
        int rc = mh_dict_create(bytes.data(), off.data(), np, folded ? MH_FIND_FOLD_ASCII : 0u, &d);
        if (rc != MH_OK || !d || mh_dict_size(d) != np || mh_dict_states(d) > bytes.size() + 1 || mh_dict_classes(d) > int(alpha) + 1) {
            ++mismatches;
            mh_dict_free(d);
            continue;
        }
        const std::vector<Hit> want = naive(pats, text, folded);
        uint64_t total = ~0ull;
        rc = mh_dict_find_bytes(d, text.data(), text.size(), nullptr, nullptr, 0, &total);
        if (rc != MH_OK || total != want.size()) ++mismatches;
        // with room for all, and with room for a prefix: exactly cap records are written
        const uint64_t caps[2] = {want.size(), want.empty() ? 0 : below(want.size())};
        for (const uint64_t cap : caps) {
            std::unique_ptr<uint64_t[]> at(new uint64_t[cap * 2]);   // (sized exactly: a write beyond cap is an ASan report;
            std::unique_ptr<uint32_t[]> pat(new uint32_t[cap]);      //  not null for cap 0, which would mean count-only)
            rc = mh_dict_find_bytes(d, text.data(), text.size(), at.get(), pat.get(), cap, &total);
            if (rc != (cap < want.size() ? MH_ERR_CAPACITY : MH_OK) || total != want.size()) ++mismatches;
            for (uint64_t r = 0; r < cap; ++r)
                if (!(Hit{at[2 * r], at[2 * r + 1], pat[r]} == want[r])) { ++mismatches; break; }
        }
        hits_seen += want.size();
        mh_dict_free(d);
    }
    // the refusals
    {
        const uint8_t b[4] = {'a', 'b', 'c', 'd'};
        const uint32_t ok[3] = {0, 2, 4}, empty[3] = {0, 0, 4}, first[3] = {1, 2, 4};
        mh_dict *d = nullptr;
        if (mh_dict_create(b, empty, 2, 0, &d) != MH_ERR_ARG || d) ++mismatches;
        if (mh_dict_create(b, first, 2, 0, &d) != MH_ERR_ARG || d) ++mismatches;
        if (mh_dict_create(b, ok, 0, 0, &d) != MH_ERR_ARG || d) ++mismatches;
        if (mh_dict_create(b, ok, 2, 2, &d) != MH_ERR_ARG || d) ++mismatches;
        if (mh_dict_create(nullptr, ok, 2, 0, &d) != MH_ERR_ARG || d) ++mismatches;
        std::vector<uint8_t> big(MH_DICT_MAX_LEN + 1, 'a');
        const uint32_t one[2] = {0, MH_DICT_MAX_LEN + 1};
        if (mh_dict_create(big.data(), one, 1, 0, &d) != MH_ERR_ARG || d) ++mismatches;
    }
    printf("%ld cases, %llu hits, %llu mismatches\n", cases, (unsigned long long)hits_seen, (unsigned long long)mismatches);
    return mismatches ? 1 : 0;
}
