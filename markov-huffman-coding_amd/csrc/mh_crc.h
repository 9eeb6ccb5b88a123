// mh_crc.h — the CRC-32 arithmetic (host and device) and the launch interface between the digest calls of the C ABI
// (mh_api_crc.cpp) and their kernels (mh_crc.hip): the CRC-32 of every stream's decoded message, taken from the decoded
// symbols while they sit in a register (include/mh.h, "DIGESTS OF BATCHES").  The batch layouts are those of mh_batch.h, the
// per-stream models those of mh_each.h.
//
// CRC-32 as zlib, gzip and PNG define it: reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF.  A
// register holds a polynomial over GF(2) modulo P with the coefficient of x^k in bit 31 - k, so x^0 is 0x80000000.  With
// R(M) the register after message M from initial value 0 and no final XOR (R is linear in M):
//   R(A || B) = R(A) * x^(8|B|) + R(B)
//   crc(M)    = R(M) + 0xFFFFFFFF * x^(8|M|) + 0xFFFFFFFF
// so the chunks of a stream are digested independently and combined by XOR in any order.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"
#include "mh_each.h"

namespace mhc {

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t CRC_ONE = 0x80000000u;          // x^0
constexpr uint32_t CRC_ONES = 0xFFFFFFFFu;

// a * b mod P, 32 steps, no branch on the data
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}

// byte[c]: the register after byte c from register 0 (the byte-wise step: r = byte[(r ^ c) & 255] ^ (r >> 8));
// pow8[j] = x^(8 * 2^j) mod P.  The check kernels take the tables as an argument and copy them into the workspace.
struct CrcTables {
    uint32_t byte[256];
    uint32_t pow8[64];
};
constexpr uint32_t CRC_TABLE_WORDS = 256 + 64;
constexpr CrcTables make_tables() {
    CrcTables t{};
    for (uint32_t c = 0; c < 256; ++c) {
        uint32_t r = c;
        for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (CRC_POLY & (0u - (r & 1u)));
        t.byte[c] = r;
    }
    t.pow8[0] = CRC_ONE >> 8;
    for (int j = 1; j < 64; ++j) t.pow8[j] = gf_mul(t.pow8[j - 1], t.pow8[j - 1]);
    return t;
}

// x^(8n) mod P from pow8 (one multiply per set bit of n beyond the first)
__host__ __device__ inline uint32_t pow8_of(const uint32_t *pow8, uint64_t n) {
    uint32_t r = CRC_ONE;
    for (int j = 0; n; n >>= 1, ++j)
        if (n & 1u) r = r == CRC_ONE ? pow8[j] : gf_mul(r, pow8[j]);
    return r;
}

// crc(M) from R(M) and |M|
__host__ __device__ inline uint32_t finish_of(const uint32_t *pow8, uint32_t r, uint64_t len) {
    return r ^ gf_mul(CRC_ONES, pow8_of(pow8, len)) ^ CRC_ONES;
}

// workspace of the coded calls: status block | tables u32[320] | per-stream status (when the caller passes none).  Nothing
// per chunk: the chunks' partial digests are combined in the caller's d_crc.  The raw call uses the first two parts.
struct CrcLayout {
    size_t off_tab, off_status, total;
};
inline CrcLayout crc_layout(uint64_t n_streams) {
    CrcLayout l;
    l.off_tab = 64;
    l.off_status = l.off_tab + CRC_TABLE_WORDS * 4;
    l.total = (l.off_status + size_t(n_streams) * 4 + 255) & ~size_t(255);
    return l;
}

struct CrcParams {
    mhb::DecBatchParams b;          // the batch and, under a shared model, its decode tables (out / out_cap unused; sym_off read only)
    mhe::SetDev set;                // the models under a set
    uint32_t *crc;                  // n (written; the chunks' partial digests meet here)
    unsigned long long *len;        // n, or nullptr
};

// a piece of an uncompressed stream is one lane's work in the raw call: stream i's pieces from in_off_i / RAW_PIECE + i
constexpr uint32_t RAW_SHIFT = 10, RAW_PIECE = 1u << RAW_SHIFT;
inline uint64_t raw_pieces(uint64_t n_streams, uint64_t total) { return total / RAW_PIECE + n_streams + 1; }

// model: what the batch was coded under (mhb::Model, mh_batch.h); b's tables and b.prev0 as that model's batch decoder takes them
using mhb::Model;
hipError_t launch_crc(const CrcParams &p, Model model, void *d_ws, hipStream_t st);
hipError_t launch_crc_raw(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total, uint32_t *d_crc, void *d_ws, hipStream_t st);

}  // namespace mhc
