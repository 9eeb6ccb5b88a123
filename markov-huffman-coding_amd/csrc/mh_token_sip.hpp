// mh_token_sip.hpp — the token of a span (include/mh.h, "TOKENS FROM MATCHED BYTES"): SipHash-2-4 and the format rules, plain
// C++ without a device dependency, compiled for the host (mh_token_host.cpp, which the sanitizer fuzz links alone) and for
// the device (mh_token.hip).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MHT_HD __host__ __device__
#else
#define MHT_HD
#endif

namespace mht {

// ---------------------------------------------------------------------------------------------------- SipHash-2-4
// The published algorithm, absorbing one byte at a time: a lane of the kernels has every byte in a register exactly once.
struct Sip {
    uint64_t v0, v1, v2, v3, m;
    uint64_t len;

    static MHT_HD inline uint64_t rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }
    MHT_HD inline void round() {
        v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
        v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
        v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
        v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
    }
    MHT_HD inline void init(uint64_t k0, uint64_t k1) {
        v0 = k0 ^ 0x736f6d6570736575ull; v1 = k1 ^ 0x646f72616e646f6dull;
        v2 = k0 ^ 0x6c7967656e657261ull; v3 = k1 ^ 0x7465646279746573ull;
        m = 0; len = 0;
    }
    MHT_HD inline void word(uint64_t w) { v3 ^= w; round(); round(); v0 ^= w; }
    // fold: ASCII A-Z absorbed as a-z
    MHT_HD inline void put(uint32_t byte, bool fold) {
        if (fold && byte - 0x41u < 26u) byte |= 0x20u;
        m |= uint64_t(byte) << (8u * (uint32_t(len) & 7u));
        if ((++len & 7u) == 0) { word(m); m = 0; }
    }
    MHT_HD inline uint64_t finish() {
        word(m | (len << 56));
        v2 ^= 0xff;
        round(); round(); round(); round();
        return v0 ^ v1 ^ v2 ^ v3;
    }
};

inline uint64_t load_le64(const uint8_t *p) {
    uint64_t x = 0;
    for (int k = 0; k < 8; ++k) x |= uint64_t(p[k]) << (8 * k);
    return x;
}

// ---------------------------------------------------------------------------------------------------- formats
// format f: prefix fmt_bytes[fmt_off[2f], fmt_off[2f + 1]), hex_digits[f] digits, suffix fmt_bytes[fmt_off[2f + 1], fmt_off[2f + 2])
constexpr uint32_t MAX_HEX = 16;
constexpr uint32_t MAX_TOKEN = 255;                  // MH_SPLICE_MAX_REP

// entry k of fmt_off (k <= 2 * n_formats) against its successor, and format k's length and digits (k < n_formats)
MHT_HD inline bool format_entry_bad(const uint64_t *fmt_off, const uint8_t *hex_digits, uint64_t n_formats, uint64_t k) {
    if (k == 0 && fmt_off[0] != 0) return true;
    if (k < 2 * n_formats && fmt_off[k + 1] < fmt_off[k]) return true;
    if (k < n_formats) {
        if (hex_digits[k] > MAX_HEX) return true;
        const uint64_t a = fmt_off[2 * k], b = fmt_off[2 * k + 2];
        if (b < a || b - a + hex_digits[k] > MAX_TOKEN) return true;
    }
    return false;
}

// every rule of a format table at once (host memory): MH_OK or MH_ERR_ARG.  fmt_bytes may be null when the table has no byte.
int formats_check(const uint64_t *fmt_off, const uint8_t *fmt_bytes, const uint8_t *hex_digits, size_t n_formats);

}  // namespace mht
