// mh_batch_dev.hpp — device code shared by the kernels of the batch call family: the decoders (mh_batch.hip, mh_each.hip,
// mh_batch_o2.hip), the random-access decoders (mh_range.hip), the state builder (mh_batch_states.hip), the
// search (mh_find.hip), the re-coders (mh_recode.hip) and the digests (mh_crc.hip).  What lives here, once:
//   gtid, grid_threads, grid_for     thread numbering and grid sizes
//   fail, stopped, stream_fail       the status word, the stop flag, a stream's verdict
//   find_stream                      closed-form unit and chunk numbering
//   offsets_bad, check_batch         the up-front checks of a batch to decode: every call of the family gives the same verdicts
//   Chunk, chunk_of<O2>              chunk w of an indexed batch in either entry format
//   load16, byte_of                  unaligned 16-byte loads
//   Unit, unit_of<CTX>               a lane's 16 bytes of an encoder's work unit and the one or two bytes in front of them
//   scan_exclusive                   the segmented u64 scans
//   batch_check_kernel, batch_enc_sizes_kernel, batch_zero_kernel, batch_tail_kernel
//                                    the stages of a batch encoder that do not look at the model (mh_batch.hip, mh_batch_o2.hip,
//                                    mh_each.hip; the last two serve the table files of mh_each.hip as well)
//   BitWriter, ByteOut, stream_src   bits out with shared edge words and the tail word, bytes out, a payload as a bit source
//   load_tables                      a shared model's decode tables into LDS (their size: mhb::tables_lds, mh_batch.h)
// Everything is in an unnamed namespace: each kernel file gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_batch.h"
#include "mh_decode_dev.hpp"
#include "mh_dev.hpp"
#include "../../include/mh.h"

namespace mhb {
namespace {

using mhk::BitSrc;
using mhk::DecTables;

constexpr uint32_t SUB_SHIFT = 10;                    // log2(B_SUB)
static_assert((1u << SUB_SHIFT) == B_SUB && B_SUB == 64 * B_VEC, "a sub-step is one wave of 16-byte lanes");

__device__ __forceinline__ void fail(int *status, int code) { atomicCAS(status, 0, code); }
__device__ __forceinline__ bool stopped(const int *stop) { return *reinterpret_cast<const volatile int *>(stop) != 0; }
__device__ __forceinline__ uint64_t gtid() { return uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; }
inline dim3 grid_threads(uint64_t items, uint32_t per_block) { return dim3(uint32_t((items + per_block - 1) / per_block)); }

// stream i's verdict
__device__ __forceinline__ void stream_fail(const DecBatchParams &p, int *status, uint64_t i, int mh_code, int dev_code) {
    p.stream_status[i] = mh_code;
    fail(status, dev_code);
}

// thread i <= n of an offset check: [0] == 0, [n] == total, non-decreasing
template <typename T>
__device__ __forceinline__ bool offsets_bad(const T *off, uint64_t n, uint64_t total, uint64_t i) {
    return (i == 0 && off[0] != 0) || (i == n && off[n] != total) || (i < n && off[i + 1] < off[i]);
}

// The up-front checks of a batch to decode, thread i <= n: pay_off[0] != 0, pay_off[n] != pay_total or a decreasing pair, the
// same of sym_off with an index -> BATCH_STATUS_ARG and the call stops (returns true); else stream_status[i] = MH_OK, or
// MH_ERR_ARG when nbits_i does not fit the stream's payload.
__device__ __forceinline__ bool check_batch(const DecBatchParams &p, uint64_t i, int *status, int *stop) {
    bool bad = offsets_bad(p.pay_off, p.n, p.pay_total, i);
    if (p.index) bad |= offsets_bad(p.sym_off, p.n, p.sym_total, i);
    if (bad) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
    if (i == p.n) return bad;
    p.stream_status[i] = MH_OK;
    if (!bad && p.nbits[i] > (p.pay_off[i + 1] - p.pay_off[i]) * 8u) stream_fail(p, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
    return bad;
}

// The stream that owns unit / chunk number u: the largest i <= n with (off[i] >> shift) + i <= u (the closed-form bases are
// strictly increasing).  i == n: u lies behind the last stream.
template <typename T>
__device__ __forceinline__ uint64_t find_stream(const T *off, uint64_t n, uint32_t shift, uint64_t u) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if ((off[mid] >> shift) + mid <= u) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// chunk w of an indexed batch: its stream, symbols, bit span and the raw context field of its entry
struct Chunk {
    uint64_t i, ni, first, nb, start, end;
    uint32_t nsym, ctx;
    bool last;
    __device__ __forceinline__ bool entry_ok() const { return start <= end && end <= nb; }
};
// O2: entries of an order-2 index (position in IDX2_POS, two context bytes from bit 48), else of an order-0/1 index
// (MH_INDEX_BIT_MASK, one byte from bit 56).  false when w is a gap.  dec_idx_kernel (mh_batch.hip) carries these steps in its
// own body, with the stream's status tested before the entry is read: change the entry format here and there.
template <bool O2>
__device__ __forceinline__ bool chunk_of(const DecBatchParams &b, uint64_t w, Chunk &c) {
    constexpr uint64_t pos = O2 ? mhk::IDX2_POS : MH_INDEX_BIT_MASK;
    const uint32_t cs = b.chunk_shift;
    c.i = find_stream(b.sym_off, b.n, cs, w);
    if (c.i >= b.n) return false;
    const uint64_t a = b.sym_off[c.i];
    c.ni = b.sym_off[c.i + 1] - a;
    c.first = (w - ((a >> cs) + c.i)) << cs;
    if (c.first >= c.ni) return false;
    c.nb = b.nbits[c.i];
    const uint64_t e = b.index[w];
    c.start = e & pos;
    c.ctx = uint32_t(e >> (O2 ? 48 : 56));
    c.last = c.first + (uint64_t(1) << cs) >= c.ni;
    c.end = c.last ? c.nb : (b.index[w + 1] & pos);
    c.nsym = uint32_t(c.last ? c.ni - c.first : (uint64_t(1) << cs));
    return true;
}

// cnt (1..16) bytes at an arbitrary address, zero beyond cnt; only the dwords that hold bytes of the range are read (a stream
// starts at any byte, so load_raw's 16-byte alignment does not hold here)
__device__ __forceinline__ void load16(const uint8_t *p, uint32_t cnt, uint32_t (&x)[4]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~uintptr_t(3));
    const uint32_t sh = uint32_t(a & 3u);
    const uint32_t nw = (sh + cnt + 3u) >> 2;
    uint32_t d[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = uint32_t(k) < nw ? w[k] : 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t v = uint32_t(((uint64_t(d[q + 1]) << 32) | d[q]) >> (8u * sh));
        const uint32_t lo = 4u * uint32_t(q);
        if (cnt <= lo) v = 0;
        else if (cnt < lo + 4u) v &= 0xFFFFFFFFu >> (8u * (lo + 4u - cnt));
        x[q] = v;
    }
}
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&x)[4], uint32_t t) { return (x[t >> 2] >> (8u * (t & 3u))) & 255u; }

// Work unit u of a batch to encode (closed-form numbering of mh_batch.h): its stream, the lane's bytes and the context in
// front of them, CTX bytes wide (1: order 0/1, 2: order 2) and prev0 at the stream's start; false when the unit
// (wave-uniform) has nothing to code.
struct Unit {
    uint64_t i, a, ni, ub, j0;
    uint32_t cnt, ctx;
    uint32_t x[4];
};
template <int CTX>
__device__ __forceinline__ bool unit_of(const uint8_t *data, const uint64_t *in_off, uint64_t n, uint32_t prev0, uint64_t u, Unit &l) {
    static_assert(CTX == 1 || CTX == 2, "one context byte or two");
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
    l.ctx = prev0;
    if (l.cnt) {
        load16(data + l.a + l.j0, l.cnt, l.x);
        if (l.j0) {                                                // (j0 is 0 or >= 16)
            const uint8_t *f = data + l.a + l.j0;
            l.ctx = CTX == 2 ? (uint32_t(f[-2]) << 8) | f[-1] : f[-1];
        }
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ scans (exclusive, u64)

constexpr int SCAN_T = 256;                        // SCAN_BLOCK / 4 elements per thread

template <int NT>
__device__ __forceinline__ unsigned long long block_exclusive(unsigned long long v, unsigned long long *s, unsigned long long &tot) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const unsigned long long x = int(threadIdx.x) >= d ? s[threadIdx.x - d] : 0ull;
        __syncthreads();
        s[threadIdx.x] += x;
        __syncthreads();
    }
    tot = s[NT - 1];
    const unsigned long long incl = s[threadIdx.x];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(SCAN_T) void batch_scan_block_kernel(unsigned long long *a, uint64_t len, unsigned long long *sums, const int *stop) {
    __shared__ unsigned long long s[SCAN_T];
    if (stopped(stop)) return;
    const uint64_t base = uint64_t(blockIdx.x) * SCAN_BLOCK + uint64_t(threadIdx.x) * 4u;
    unsigned long long v[4], t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = base + k < len ? a[base + k] : 0ull; t += v[k]; }
    unsigned long long tot;
    unsigned long long run = block_exclusive<SCAN_T>(t, s, tot);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (base + k < len) a[base + k] = run; run += v[k]; }
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(1024) void batch_scan_sums_kernel(unsigned long long *sums, uint64_t nb, const int *stop) {
    __shared__ unsigned long long s[1024];
    if (stopped(stop)) return;
    unsigned long long carry = 0;
    for (uint64_t c = 0; c < nb; c += 1024) {
        const uint64_t k = c + threadIdx.x;
        const unsigned long long v = k < nb ? sums[k] : 0ull;
        unsigned long long tot;
        const unsigned long long ex = block_exclusive<1024>(v, s, tot);
        if (k < nb) sums[k] = carry + ex;
        carry += tot;
    }
}

__global__ __launch_bounds__(SCAN_T) void batch_scan_add_kernel(unsigned long long *a, uint64_t len, const unsigned long long *sums, const int *stop) {
    if (stopped(stop)) return;
    const unsigned long long add = sums[blockIdx.x];
    const uint64_t base = uint64_t(blockIdx.x) * SCAN_BLOCK;
    for (uint32_t k = threadIdx.x; k < SCAN_BLOCK; k += SCAN_T)
        if (base + k < len) a[base + k] += add;
}

hipError_t scan_exclusive(unsigned long long *a, uint64_t len, unsigned long long *sums, const int *stop, hipStream_t st) {
    if (len == 0) return hipSuccess;
    const uint64_t nb = scan_blocks(len);
    hipLaunchKernelGGL(batch_scan_block_kernel, dim3(uint32_t(nb)), dim3(SCAN_T), 0, st, a, len, sums, stop);
    hipLaunchKernelGGL(batch_scan_sums_kernel, dim3(1), dim3(1024), 0, st, sums, nb, stop);
    hipLaunchKernelGGL(batch_scan_add_kernel, dim3(uint32_t(nb)), dim3(SCAN_T), 0, st, a, len, sums, stop);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ model-free encode stages

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"               // (a file that only decodes launches none of these)

// offsets non-decreasing, [0] == 0, [n] == total, else BATCH_STATUS_ARG and the call stops
__global__ void batch_check_kernel(const uint64_t *off, uint64_t n, uint64_t total, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i > n) return;
    if (offsets_bad(off, n, total, i)) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
}

// stream i: payload bits from the scanned unit bits, payload bytes into out_off (scanned next)
__global__ void batch_enc_sizes_kernel(const uint64_t *in_off, uint64_t n, const unsigned long long *ubase, unsigned long long *nbits,
                                       unsigned long long *out_off, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t i = gtid();
    if (i > n) return;
    if (i == n) { out_off[i] = 0; return; }
    const uint64_t u0 = (in_off[i] >> SUB_SHIFT) + i, u1 = (in_off[i + 1] >> SUB_SHIFT) + i + 1;
    const unsigned long long bits = ubase[u1] - ubase[u0];
    nbits[i] = bits;
    out_off[i] = (bits + 7) >> 3;
}

// zeroes the output bytes [0, *off_end) (bits are OR-ed into shared edge words) or reports that they do not fit
__global__ void batch_zero_kernel(const unsigned long long *off_end, uint8_t *out, uint64_t cap, int *status, int *stop, uint32_t *tail) {
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

// the bytes of the last, partial dword from the workspace's tail word (BitWriter): nothing is touched at or beyond *off_end
__global__ void batch_tail_kernel(const unsigned long long *off_end, uint8_t *out, const uint32_t *tail, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t bytes = *off_end;
    if (!(bytes & 3u)) return;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(tail);
    for (uint64_t b = bytes & ~uint64_t(3); b < bytes; ++b) out[b] = t[b & 3u];
}

#pragma clang diagnostic pop

// Bits into 32-bit words, first stream bit in bit 31 of a word stored byte-swapped (MSB first inside a byte,
// src/bitbuffer.cpp:12).  A word that lies wholly inside the lane's bits is stored; its edge words are shared with the
// neighbour lane, sub-step or stream and are OR-ed into zeroed memory.  The last dword of the whole output, when it reaches
// past the payload, is OR-ed into a workspace word instead and its bytes are copied out afterwards: nothing is touched at or
// beyond out_off[n] <= cap.
struct BitWriter {
    uint32_t *out;
    uint32_t *tail;
    uint64_t tail_w;
    uint64_t w;           // word the accumulator's first bit belongs to
    uint64_t acc;         // nb pending bits, right-aligned
    uint32_t nb;
    bool lead;            // the current word holds bits in front of the lane's
    __device__ __forceinline__ void init(uint32_t *o, uint32_t *t, uint64_t tw, uint64_t bit) {
        out = o; tail = t; tail_w = tw; w = bit >> 5; nb = uint32_t(bit & 31u); acc = 0; lead = nb != 0;
    }
    __device__ __forceinline__ void put_word(uint32_t v, bool shared) {
        const uint32_t m = __builtin_bswap32(v);
        if (w == tail_w) atomicOr(tail, m);
        else if (shared) atomicOr(out + w, m);
        else out[w] = m;
    }
    __device__ __forceinline__ void push(uint64_t v, uint32_t l) {        // l <= 32
        if (!l) return;
        acc = (acc << l) | v;
        nb += l;
        if (nb >= 32u) {
            nb -= 32u;
            put_word(uint32_t(acc >> nb), lead);
            lead = false;
            acc &= (uint64_t(1) << nb) - 1u;
            ++w;
        }
    }
    __device__ __forceinline__ void code(uint64_t c, uint32_t l) {         // l <= 64
        if (l > 32u) { push(c >> 32, l - 32u); push(c & 0xFFFFFFFFull, 32u); }
        else push(c, l);
    }
    __device__ __forceinline__ void finish() {
        if (nb) put_word(uint32_t(acc << (32u - nb)), true);
    }
};

// a stream's payload as a bit source: reads stay inside the dwords that hold its bytes
__device__ __forceinline__ BitSrc stream_src(const uint8_t *payload, uint64_t po, uint64_t nbits, uint64_t &bit0) {
    const uint64_t base = po & ~uint64_t(3);
    BitSrc s;
    s.p = payload + base;
    s.bytes = po + ((nbits + 7) >> 3) - base;
    s.full_words = s.bytes >> 2;
    bit0 = (po - base) * 8u;
    return s;
}

// output bytes of one lane: whole aligned dwords where the lane owns them, single bytes at its edges
struct ByteOut {
    uint8_t *o;
    uint64_t beg, pos;
    uint32_t q;
    __device__ __forceinline__ void init(uint8_t *out, uint64_t at) { o = out; beg = pos = at; q = 0; }
    __device__ __forceinline__ void put(uint32_t b) {
        q |= b << (8u * uint32_t(pos & 3u));
        if ((pos & 3u) == 3u) {
            const uint64_t d = pos - 3u;
            if (d >= beg) *reinterpret_cast<uint32_t *>(o + d) = q;
            else for (uint64_t k = beg; k <= pos; ++k) o[k] = uint8_t(q >> (8u * uint32_t(k & 3u)));
            q = 0;
        }
        ++pos;
    }
    __device__ __forceinline__ void flush() {
        if (pos & 3u) {
            const uint64_t d = pos & ~uint64_t(3);
            for (uint64_t k = d > beg ? d : beg; k < pos; ++k) o[k] = uint8_t(q >> (8u * uint32_t(k & 3u)));
        }
    }
};

// LDS: sec_base u32[256] | prim u16[256 << P] | sec u16[nsec] when the model's tables fit (the chunk decoder's layout).
// mhb::tables_lds (mh_batch.h) is the size of exactly this layout: the two are a pair, change them together.
__device__ __forceinline__ DecTables load_tables(const DecBatchParams &p, unsigned char *smem, const uint16_t *&lut, const uint32_t *&sub_base) {
    uint32_t *sb = reinterpret_cast<uint32_t *>(smem);
    uint16_t *lp = reinterpret_cast<uint16_t *>(smem + 1024);
    const uint32_t nprim16 = (256u << p.P) / 8u;
    for (uint32_t i = threadIdx.x; i < nprim16; i += blockDim.x) reinterpret_cast<uint4 *>(lp)[i] = reinterpret_cast<const uint4 *>(p.prim)[i];
    uint16_t *lsec = lp + (256u << p.P);
    if (p.sec_lds) {
        const uint32_t nsec16 = (p.nsec + 7u) / 8u;
        for (uint32_t i = threadIdx.x; i < nsec16; i += blockDim.x) reinterpret_cast<uint4 *>(lsec)[i] = reinterpret_cast<const uint4 *>(p.sec)[i];
    }
    for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) sb[i] = p.sec_base[i];
    __syncthreads();
    lut = lp;
    sub_base = sb;
    return DecTables{p.sec_lds ? lsec : p.sec, p.tree, p.P, p.direct, p.H,
                     __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(p.sec), 0, int((p.nsec + 8u) * 2u), 0x00020000)};
}

inline int grid_for(uint64_t items, uint64_t per_block, int per_cu) {
    const uint64_t want = (items + per_block - 1) / per_block;
    const uint64_t cap = uint64_t(mhk::cu_count()) * uint64_t(per_cu);
    return int(want < 1 ? 1 : (want > cap ? cap : want));
}

}  // namespace
}  // namespace mhb
