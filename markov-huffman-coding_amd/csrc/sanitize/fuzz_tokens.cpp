// fuzz_tokens — mh_span_token_digest against a word-at-a-time SipHash-2-4 and mht::formats_check against the rules as
// include/mh.h states them, on random inputs under AddressSanitizer + UndefinedBehaviorSanitizer.  Links mh_token_host.cpp
// alone (no HIP, no device): `make fuzz_tokens`.  Buffers are heap blocks of exactly the size a call may read, so that a
// read past one is seen.
//   fuzz_tokens CASES SEED   ->  "<cases> cases, <mismatches> mismatches"; exit 1 on a mismatch
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../../include/mh.h"
#include "../mh_token_sip.hpp"

namespace {

uint64_t rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

// the published algorithm, a whole word at a time
uint64_t siphash24(const uint8_t *key, const std::vector<uint8_t> &in) {
    uint64_t k0, k1;
    memcpy(&k0, key, 8);
    memcpy(&k1, key + 8, 8);
    uint64_t v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull, v2 = k0 ^ 0x6c7967656e657261ull, v3 = k1 ^ 0x7465646279746573ull;
    auto round = [&] {
        v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
        v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
        v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
        v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
    };
    const size_t n = in.size(), full = n / 8 * 8;
    for (size_t k = 0; k <= full; k += 8) {
        uint64_t m = 0;
        if (k < full) memcpy(&m, in.data() + k, 8);
        else {
            for (size_t j = 0; j < n - full; ++j) m |= uint64_t(in[full + j]) << (8 * j);
            m |= uint64_t(n & 0xff) << 56;
        }
        v3 ^= m; round(); round(); v0 ^= m;
    }
    v2 ^= 0xff;
    round(); round(); round(); round();
    return v0 ^ v1 ^ v2 ^ v3;
}

}  // namespace

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 20000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    auto below = [&](uint64_t n) { return rng() % n; };
    uint64_t mismatches = 0;
    // the known answers under key 00 01 .. 0f
    {
        uint8_t key[16];
        for (int k = 0; k < 16; ++k) key[k] = uint8_t(k);
        const struct { size_t n; uint64_t want; } kat[] = {{0, 0x726fdb47dd0e0e31ull}, {8, 0x93f5f5799a932462ull}, {15, 0xa129ca6149be45e5ull},
                                                           {63, 0x958a324ceb064572ull}};
        for (const auto &t : kat) {
            std::vector<uint8_t> in(t.n);
            for (size_t k = 0; k < t.n; ++k) in[k] = uint8_t(k);
            if (mh_span_token_digest(key, in.data(), in.size(), 0) != t.want || siphash24(key, in) != t.want) {
                printf("known answer of %zu bytes differs\n", t.n);
                ++mismatches;
            }
        }
    }
    for (long c = 0; c < cases; ++c) {
        // ---- the digest: every length class, bytes of both cases, with and without the fold
        std::vector<uint8_t> key(16);
        for (auto &b : key) b = uint8_t(rng());
        const size_t n = c % 7 == 0 ? below(600) : below(70);
        std::vector<uint8_t> in(n);
        for (auto &b : in) b = below(2) ? uint8_t('@' + below(30)) : uint8_t(rng());
        const bool fold = below(2);
        std::vector<uint8_t> folded = in;
        if (fold) for (auto &b : folded) if (b >= 'A' && b <= 'Z') b = uint8_t(b + 32);
        const uint64_t got = mh_span_token_digest(key.data(), n ? in.data() : nullptr, n, fold ? MH_TOKEN_FOLD : 0u);
        if (got != siphash24(key.data(), folded)) {
            printf("case %ld: digest of %zu bytes (fold %d) differs\n", c, n, int(fold));
            ++mismatches;
        }
        // ---- the formats: valid tables, and tables with one rule broken
        const size_t nf = below(6);
        std::vector<uint64_t> off(2 * nf + 1, 0);
        std::vector<uint8_t> hex(nf);
        bool ok = true;
        for (size_t f = 0; f < nf; ++f) {
            const uint64_t pre = below(9) == 0 ? below(200) : below(12), suf = below(9) == 0 ? below(120) : below(6);
            hex[f] = uint8_t(below(11) == 0 ? below(40) : below(17));
            off[2 * f + 1] = off[2 * f] + pre;
            off[2 * f + 2] = off[2 * f + 1] + suf;
            ok &= hex[f] <= 16 && pre + suf + hex[f] <= MH_SPLICE_MAX_REP;
        }
        const int broke = int(below(5));
        if (broke == 1) { off[0] = 1 + below(3); ok = false; for (size_t k = 1; k < off.size(); ++k) off[k] += off[0]; }
        if (broke == 2 && nf) {                                  // a decreasing pair somewhere
            const size_t k = 1 + below(2 * nf);
            if (off[k] > 0) { off[k - 1] = off[k] + 1 + below(3); ok = false; }
        }
        std::vector<uint8_t> bytes(size_t(off[2 * nf]) + 0);
        const bool no_bytes = broke == 3 && !bytes.empty();
        if (no_bytes) ok = false;
        const int rc = mht::formats_check(off.data(), no_bytes || bytes.empty() ? nullptr : bytes.data(), nf ? hex.data() : nullptr, nf);
        if ((rc == MH_OK) != ok || (rc != MH_OK && rc != MH_ERR_ARG)) {
            printf("case %ld: formats_check gave %d, the rules say %s\n", c, rc, ok ? "valid" : "invalid");
            ++mismatches;
        }
    }
    if (mht::formats_check(nullptr, nullptr, nullptr, 0) != MH_ERR_ARG) ++mismatches;
    printf("%ld cases, %llu mismatches\n", cases, (unsigned long long)mismatches);
    return mismatches ? 1 : 0;
}
