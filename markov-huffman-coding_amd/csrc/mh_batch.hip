// mh_batch.hip — batches of independent order-0/1 streams under one shared model (include/mh.h, "BATCHES OF INDEPENDENT
// STREAMS").  Every stream starts in context prev0, as every file of the reference does (src/coding.cpp:67,118).
//   batch_check_kernel        offsets non-decreasing, [0] == 0, [n] == total (else MH_ERR_ARG through the status word)
//   batch_hist_fixup_kernel   the order-1 histogram of the concatenation counted each stream's first pair in the context of
//                             the previous stream's last byte: one thread per boundary moves it to prev0
//   batch_enc_len_kernel      one wave per (stream, 1 KiB sub-step): the sub-step's payload bits
//   batch_scan_*              exclusive scans (unit bits -> stream-relative bit offsets; payload bytes -> out_off)
//   batch_enc_emit_kernel     one wave per (stream, 1 KiB sub-step): codes through the 12-bit LDS image, longer ones through
//                             the full (len8, code64) tables; the sub-step's index entries
//   batch_dec_idx_kernel      one lane per (stream, chunk) with an index
//   batch_dec_walk_kernel     one lane per stream without an index: a count pass, then (after the scan) an emit pass
// Hand-offs between workgroups go across launch boundaries only (mh_encode.hip records why the look-back scan lost).
// The single-stream kernels and their headers are used read-only: nothing here changes how a single stream is coded.
#include "mh_batch.h"
#include "mh_batch_dev.hpp"
#include "mh_decode_dev.hpp"
#include "mh_dev.hpp"
#include "../../include/mh.h"

namespace mhb {

using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;

namespace {

// ------------------------------------------------------------------------------------------------ checks, histogram fix-up

__global__ void batch_check_kernel(const uint64_t *off, uint64_t n, uint64_t total, int *status, int *stop, int *stream_status) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > n) return;
    bool bad = (i == 0 && off[0] != 0) || (i == n && off[n] != total) || (i < n && off[i + 1] < off[i]);
    if (bad) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
    if (stream_status && i < n) stream_status[i] = MH_OK;
}

__global__ void batch_hist_fixup_kernel(const uint8_t *data, const uint64_t *off, uint64_t n, uint64_t total, uint32_t prev0,
                                        unsigned long long *counts, int order, int *status) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > n) return;
    const bool bad = (i == 0 && off[0] != 0) || (i == n && off[n] != total) || (i < n && off[i + 1] < off[i]);
    if (bad) atomicExch(status, BATCH_STATUS_ARG);               // (the conservation check's CORRUPT gives way: the input was wrong)
    if (order == 0 || i >= n || bad) return;
    const uint64_t a = off[i], b = off[i + 1];
    if (a == 0 || b <= a || b > total) return;
    const uint32_t first = data[a], p = data[a - 1];
    if (p == prev0) return;
    atomicAdd(&counts[p * 256u + first], ~0ull);                  // -1
    atomicAdd(&counts[prev0 * 256u + first], 1ull);
}

// ------------------------------------------------------------------------------------------------ encode

// the unit's stream and the lane's bytes; false when the unit (wave-uniform) has nothing to code
struct UnitLane {
    uint64_t i, a, ni, ub, j0;
    uint32_t cnt, prev;
    uint32_t x[4];
};
__device__ __forceinline__ bool unit_lane(const EncBatchParams &p, uint64_t u, UnitLane &l) {
    l.i = find_stream(p.in_off, p.n, SUB_SHIFT, u);
    if (l.i >= p.n) return false;
    l.a = p.in_off[l.i];
    l.ni = p.in_off[l.i + 1] - l.a;
    l.ub = (l.a >> SUB_SHIFT) + l.i;
    const uint64_t s0 = (u - l.ub) << SUB_SHIFT;
    if (s0 >= l.ni) return false;
    l.j0 = s0 + uint64_t(mhk::lane_id()) * B_VEC;
    l.cnt = l.j0 < l.ni ? uint32_t(l.ni - l.j0 < B_VEC ? l.ni - l.j0 : B_VEC) : 0u;
    l.x[0] = l.x[1] = l.x[2] = l.x[3] = 0;
    l.prev = p.prev0;
    if (l.cnt) {
        load16(p.data + l.a + l.j0, l.cnt, l.x);
        if (l.j0) l.prev = p.data[l.a + l.j0 - 1];
    }
    return true;
}

__global__ __launch_bounds__(B_THREADS) void batch_enc_len_kernel(EncBatchParams p, uint64_t nunits, unsigned long long *ubits, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    for (uint32_t k = threadIdx.x; k < 65536u / 16u; k += B_THREADS)
        reinterpret_cast<uint4 *>(smem)[k] = reinterpret_cast<const uint4 *>(p.len_slot)[k];
    __syncthreads();
    const uint64_t nw = uint64_t(gridDim.x) * (B_THREADS / 64);
    for (uint64_t u = uint64_t(blockIdx.x) * (B_THREADS / 64) + threadIdx.x / 64; u < nunits; u += nw) {
        UnitLane l;
        uint32_t bits = 0;
        if (unit_lane(p, u, l)) {
            uint32_t prev = l.prev;
#pragma unroll
            for (uint32_t t = 0; t < B_VEC; ++t) {                // (unrolled: the byte index stays a constant, no scratch)
                const uint32_t sym = byte_of(l.x, t);
                if (t < l.cnt) bits += smem[mh::enc_slot(sym << 8 | prev)];
                prev = sym;
            }
        }
        bits = mhk::wave_sum(bits);
        if (mhk::lane_id() == 0) ubits[u] = bits;
    }
}

// stream i: payload bits from the scanned unit bits, payload bytes into out_off (scanned next)
__global__ void batch_enc_sizes_kernel(EncBatchParams p, const unsigned long long *ubase, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > p.n) return;
    if (i == p.n) { p.out_off[i] = 0; return; }
    const uint64_t u0 = (p.in_off[i] >> SUB_SHIFT) + i, u1 = (p.in_off[i + 1] >> SUB_SHIFT) + i + 1;
    const unsigned long long bits = ubase[u1] - ubase[u0];
    p.nbits[i] = bits;
    p.out_off[i] = (bits + 7) >> 3;
}

// zeroes the payload bytes (codes are OR-ed into shared edge dwords) or reports that they do not fit
__global__ void batch_enc_zero_kernel(EncBatchParams p, int *status, int *stop, uint32_t *tail) {
    if (stopped(stop)) return;
    const uint64_t bytes = p.out_off[p.n];
    if (bytes > p.cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
        return;
    }
    const uint64_t nfull = bytes >> 2;
    uint32_t *o = reinterpret_cast<uint32_t *>(p.out);
    for (uint64_t k = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < nfull; k += uint64_t(gridDim.x) * blockDim.x) o[k] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *tail = 0u;
}

__device__ __forceinline__ void lookup(const uint16_t *lenc, const EncBatchParams &p, uint32_t prev, uint32_t sym, uint32_t &len, uint64_t &code) {
    const uint32_t e = lenc[mh::enc_slot(sym << 8 | prev)];
    if (e == mh::ENC16_ESCAPE) {                                   // longer than the 12-bit image: the full tables (L2)
        len = p.len8[prev * 256u + sym];
        code = p.code64[prev * 256u + sym];
    } else {
        len = e >> 12;                                              // 0: the pair has no code, skipped (mh_model.hpp:21)
        code = e & 0xFFFu;
    }
}

__global__ __launch_bounds__(B_THREADS) void batch_enc_emit_kernel(EncBatchParams p, uint64_t nunits, const unsigned long long *ubase,
                                                                   uint32_t *tail, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    const uint16_t *lenc = reinterpret_cast<const uint16_t *>(smem);
    for (uint32_t k = threadIdx.x; k < 131072u / 16u; k += B_THREADS)
        reinterpret_cast<uint4 *>(smem)[k] = reinterpret_cast<const uint4 *>(p.enc16)[k];
    __syncthreads();
    const uint64_t bytes = p.out_off[p.n];
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint64_t nw = uint64_t(gridDim.x) * (B_THREADS / 64);
    for (uint64_t u = uint64_t(blockIdx.x) * (B_THREADS / 64) + threadIdx.x / 64; u < nunits; u += nw) {
        UnitLane l;
        if (!unit_lane(p, u, l)) continue;                         // wave-uniform
        uint32_t bits = 0, prev = l.prev;
#pragma unroll
        for (uint32_t t = 0; t < B_VEC; ++t) {
            const uint32_t sym = byte_of(l.x, t);
            uint32_t len = 0; uint64_t code;
            if (t < l.cnt) lookup(lenc, p, prev, sym, len, code);
            bits += len;
            prev = sym;
        }
        const uint32_t excl = mhk::wave_inclusive_sum(bits) - bits;
        const uint64_t sbit = (ubase[u] - ubase[l.ub]) + excl;     // stream-relative
        if (p.index && l.cnt && (l.j0 & ((uint64_t(1) << p.chunk_shift) - 1u)) == 0)
            p.index[(l.a >> p.chunk_shift) + l.i + (l.j0 >> p.chunk_shift)] = (uint64_t(l.prev) << 56) | sbit;
        if (!bits) continue;
        BitWriter bw;
        bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[l.i]) * 8u + sbit);
        prev = l.prev;
#pragma unroll
        for (uint32_t t = 0; t < B_VEC; ++t) {
            const uint32_t sym = byte_of(l.x, t);
            uint32_t len = 0; uint64_t code = 0;
            if (t < l.cnt) lookup(lenc, p, prev, sym, len, code);
            bw.code(code, len);
            prev = sym;
        }
        bw.finish();
    }
}

__global__ void batch_enc_tail_kernel(EncBatchParams p, const uint32_t *tail, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t bytes = p.out_off[p.n];
    if (!(bytes & 3u)) return;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(tail);
    for (uint64_t b = bytes & ~uint64_t(3); b < bytes; ++b) p.out[b] = t[b & 3u];
}

// ------------------------------------------------------------------------------------------------ decode

__global__ void batch_dec_check_kernel(DecBatchParams p, int *status, int *stop) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > p.n) return;
    check_batch(p, i, status, stop);
}

__global__ __launch_bounds__(B_THREADS) void batch_dec_idx_kernel(DecBatchParams p, uint64_t nwork, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    const uint16_t *lut; const uint32_t *sub_base;
    const DecTables tabs = load_tables(p, smem, lut, sub_base);
    const uint32_t cs = p.chunk_shift;
    for (uint64_t w = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t i = find_stream(p.sym_off, p.n, cs, w);
        if (i >= p.n) continue;
        const uint64_t a = p.sym_off[i], ni = p.sym_off[i + 1] - a;
        const uint64_t first = (w - ((a >> cs) + i)) << cs;
        if (first >= ni || p.stream_status[i] == MH_ERR_ARG) continue;
        const uint64_t nb = p.nbits[i];
        const uint64_t e = p.index[w];
        const uint64_t start = e & MH_INDEX_BIT_MASK;
        const bool last = first + (uint64_t(1) << cs) >= ni;
        const uint64_t end = last ? nb : (p.index[w + 1] & MH_INDEX_BIT_MASK);
        const uint32_t nsym = uint32_t(last ? ni - first : (uint64_t(1) << cs));
        if (start > end || end > nb) { stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        uint64_t bit0;
        const BitSrc src = stream_src(p.payload, p.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + start);
        uint32_t prev = uint32_t(e >> 56), used = 0;
        bool bad = false;
        ByteOut bo;
        bo.init(p.out, a + first);
        for (uint32_t t = 0; t < nsym && !bad; ++t) {
            prev = mhk::decode_one(lut, sub_base, tabs, src, bc, prev, used, bad);
            bo.put(prev);
        }
        bo.flush();
        if (bad || used != end - start) stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
    }
}

// EMIT = false: count the stream's symbols into sym_off[i] (scanned next); true: write them at out[sym_off[i] ...)
template <bool EMIT>
__global__ __launch_bounds__(B_THREADS) void batch_dec_walk_kernel(DecBatchParams p, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    const uint16_t *lut; const uint32_t *sub_base;
    const DecTables tabs = load_tables(p, smem, lut, sub_base);
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i <= p.n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (i == p.n) { if (!EMIT) p.sym_off[i] = 0; continue; }
        if (!EMIT) p.sym_off[i] = 0;
        if (p.stream_status[i] != MH_OK) continue;
        const uint64_t nb = p.nbits[i];
        if (!EMIT && nb > p.walk_max_bits) { stream_fail(p, status, i, MH_ERR_ARG, BATCH_STATUS_ARG); continue; }
        uint64_t count = 0;
        if (EMIT) {
            const uint64_t a = p.sym_off[i];
            count = p.sym_off[i + 1] - a;
            if (a + count > p.out_cap) { stream_fail(p, status, i, MH_ERR_CAPACITY, mhk::MHK_STATUS_CAPACITY); continue; }
        }
        uint64_t bit0;
        const BitSrc src = stream_src(p.payload, p.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0);
        uint32_t prev = p.prev0, used = 0;
        bool bad = false;
        ByteOut bo;
        bo.init(p.out, EMIT ? p.sym_off[i] : 0);
        uint64_t k = 0;
        // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
        while (used < nb && !bad && (!EMIT || k < count)) {
            prev = mhk::decode_one(lut, sub_base, tabs, src, bc, prev, used, bad);
            if (EMIT && !bad) bo.put(prev);
            ++k;
        }
        if (EMIT) bo.flush();
        if (bad || used != nb || (EMIT && k != count)) { stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        if (!EMIT) p.sym_off[i] = k;                               // src/coding.cpp:158: the stream ends exactly at nbits
    }
}

}  // namespace

hipError_t launch_hist_fixup(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total, uint32_t prev0,
                             unsigned long long *d_counts, int order, int *d_status, hipStream_t st) {
    const uint64_t threads = n + 1;
    hipLaunchKernelGGL(batch_hist_fixup_kernel, dim3(uint32_t((threads + 255) / 256)), dim3(256), 0, st, d_data, d_in_off, n, total, prev0,
                       d_counts, order, d_status);
    return hipGetLastError();
}

hipError_t launch_encode_batch(const EncBatchParams &p, void *d_ws, hipStream_t st) {
    hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(batch_enc_len_kernel), 65536);    // (per call: per device)
    if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(batch_enc_emit_kernel), 131072);
    if (attr != hipSuccess) return attr;
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const EncLayout L = enc_layout(p.n, p.total);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    auto *ubits = reinterpret_cast<unsigned long long *>(ws + L.off_units);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    auto *tail = reinterpret_cast<uint32_t *>(ws + L.off_tail);
    const uint64_t U = units_of(p.total, p.n);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(batch_check_kernel, dim3(uint32_t((p.n + 1 + 255) / 256)), dim3(256), 0, st, p.in_off, p.n, p.total, status, stop,
                       static_cast<int *>(nullptr));
    const int waves_per_block = B_THREADS / 64;
    hipLaunchKernelGGL(batch_enc_len_kernel, dim3(grid_for(U, waves_per_block, 2)), dim3(B_THREADS), 65536, st, p, U, ubits, stop);
    if ((e = scan_exclusive(ubits, U, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(batch_enc_sizes_kernel, dim3(uint32_t((p.n + 1 + 255) / 256)), dim3(256), 0, st, p, ubits, stop);
    if ((e = scan_exclusive(p.out_off, p.n + 1, sums, stop, st)) != hipSuccess) return e;
    const uint64_t bound_words = (p.total * uint64_t(p.max_len > 0 ? p.max_len : 1) / 8 + p.n + 4) / 4;
    hipLaunchKernelGGL(batch_enc_zero_kernel, dim3(grid_for(bound_words, 256, 8)), dim3(256), 0, st, p, status, stop, tail);
    hipLaunchKernelGGL(batch_enc_emit_kernel, dim3(grid_for(U, waves_per_block, 1)), dim3(B_THREADS), 131072, st, p, U, ubits, tail, stop);
    hipLaunchKernelGGL(batch_enc_tail_kernel, dim3(1), dim3(1), 0, st, p, tail, stop);
    return hipGetLastError();
}

hipError_t launch_decode_batch(const DecBatchParams &p, void *d_ws, hipStream_t st) {
    const int lds_max = 163840;
    hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(batch_dec_idx_kernel), lds_max);
    if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(batch_dec_walk_kernel<false>), lds_max);
    if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(batch_dec_walk_kernel<true>), lds_max);
    if (attr != hipSuccess) return attr;
    const size_t lds = tables_lds(p);
    if (lds > 163840) return hipErrorInvalidValue;
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const DecLayout L = dec_layout(p.n);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(batch_dec_check_kernel, dim3(uint32_t((p.n + 1 + 255) / 256)), dim3(256), 0, st, p, status, stop);
    if (p.index) {
        const uint64_t W = p.sym_total / (uint64_t(1) << p.chunk_shift) + p.n + 1;
        hipLaunchKernelGGL(batch_dec_idx_kernel, dim3(grid_for(W, B_THREADS, 1)), dim3(B_THREADS), lds, st, p, W, status, stop);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(batch_dec_walk_kernel<false>, dim3(grid_for(p.n + 1, B_THREADS, 1)), dim3(B_THREADS), lds, st, p, status, stop);
    if ((e = scan_exclusive(p.sym_off, p.n + 1, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(batch_dec_walk_kernel<true>, dim3(grid_for(p.n + 1, B_THREADS, 1)), dim3(B_THREADS), lds, st, p, status, stop);
    return hipGetLastError();
}

}  // namespace mhb
