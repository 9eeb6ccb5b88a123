// mh_batch.hip — batches of independent order-0/1 streams under one shared model (include/mh.h, "BATCHES OF INDEPENDENT
// STREAMS"), and the batch decoders of every model kind (launch_decode).  Every stream starts in context prev0, as
// every file of the reference does (src/coding.cpp:67,118).
//   batch_hist_fixup_kernel   the order-1 histogram of the concatenation counted each stream's first pair in the context of
//                             the previous stream's last byte: one thread per boundary moves it to prev0
//   batch_check_kernel, batch_enc_sizes_kernel, batch_zero_kernel, batch_tail_kernel, batch_scan_*
//                             (mh_batch_dev.hpp) the encoder's stages that do not look at the model: the offset check, unit
//                             bits -> stream-relative bit offsets, payload bytes -> out_off, the zeroed output, its last dword
//   batch_enc_len_kernel      one wave per (stream, 1 KiB sub-step): the sub-step's payload bits
//   batch_enc_emit_kernel     one wave per (stream, 1 KiB sub-step): codes through the 12-bit LDS image, longer ones through
//                             the full (len8, code64) tables; the sub-step's index entries
//   dec_check_kernel          the up-front checks of a batch to decode (mhb::check_batch)
//   dec_idx_kernel<K>         one lane per (stream, chunk) with an index
//   dec_walk_kernel<K, EMIT>  one lane per stream without an index: a count pass, then (after the scan) an emit pass
// The decoders are one kernel family over the symbol decoder of the model kind K (mhb::Dec<K>, mh_symdec_dev.hpp): a shared
// order-0/1 model (tables in LDS), a model set (stream i's slots in L2) and a shared order-2 model (tables in L2).
// Hand-offs between workgroups go across launch boundaries only (mh_encode.hip records why the look-back scan lost).
// The single-stream kernels and their headers are used read-only: nothing here changes how a single stream is coded.
#include "mh_batch.h"
#include "mh_each.h"
#include "mh_symdec_dev.hpp"
#include "../../include/mh.h"

namespace mhb {

using mhk::BitCursor;
using mhk::BitSrc;

namespace {

// ------------------------------------------------------------------------------------------------ histogram fix-up

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

__global__ __launch_bounds__(B_THREADS) void batch_enc_len_kernel(EncBatchParams p, uint64_t nunits, unsigned long long *ubits, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    for (uint32_t k = threadIdx.x; k < 65536u / 16u; k += B_THREADS)
        reinterpret_cast<uint4 *>(smem)[k] = reinterpret_cast<const uint4 *>(p.len_slot)[k];
    __syncthreads();
    const uint64_t nw = uint64_t(gridDim.x) * (B_THREADS / 64);
    for (uint64_t u = uint64_t(blockIdx.x) * (B_THREADS / 64) + threadIdx.x / 64; u < nunits; u += nw) {
        Unit l;
        uint32_t bits = 0;
        if (unit_of<1>(p.data, p.in_off, p.n, p.prev0, u, l)) {
            uint32_t prev = l.ctx;
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
        Unit l;
        if (!unit_of<1>(p.data, p.in_off, p.n, p.prev0, u, l)) continue;   // wave-uniform
        uint32_t bits = 0, prev = l.ctx;
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
            p.index[(l.a >> p.chunk_shift) + l.i + (l.j0 >> p.chunk_shift)] = (uint64_t(l.ctx) << 56) | sbit;
        if (!bits) continue;
        BitWriter bw;
        bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[l.i]) * 8u + sbit);
        prev = l.ctx;
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

// ------------------------------------------------------------------------------------------------ decode, every model kind

__global__ void dec_check_kernel(DecBatchParams b, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i > b.n) return;
    check_batch(b, i, status, stop);
}

template <Model K>
__global__ __launch_bounds__(Dec<K>::NT) void dec_idx_kernel(DecodeParams p, uint64_t nwork, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        // chunk_of's steps (mh_batch_dev.hpp) with the stream's status tested between the stream and its entry, as the decoders
        // always did: a refused stream's lanes leave before the entry loads are issued.  Through chunk_of, which reads the entry
        // first, the three kernels had 14 to 18 instructions and up to 5 VGPRs more and took up to 9 % longer.
        constexpr uint64_t pos = Dec<K>::O2 ? mhk::IDX2_POS : MH_INDEX_BIT_MASK;
        const uint32_t cs = p.b.chunk_shift;
        Chunk c;
        c.i = find_stream(p.b.sym_off, p.b.n, cs, w);
        if (c.i >= p.b.n) continue;
        const uint64_t a = p.b.sym_off[c.i];
        c.ni = p.b.sym_off[c.i + 1] - a;
        c.first = (w - ((a >> cs) + c.i)) << cs;
        if (c.first >= c.ni || p.b.stream_status[c.i] == MH_ERR_ARG) continue;
        c.nb = p.b.nbits[c.i];
        const uint64_t e = p.b.index[w];
        c.start = e & pos;
        c.ctx = uint32_t(e >> (Dec<K>::O2 ? 48 : 56));
        c.last = c.first + (uint64_t(1) << cs) >= c.ni;
        c.end = c.last ? c.nb : (p.b.index[w + 1] & pos);
        c.nsym = uint32_t(c.last ? c.ni - c.first : (uint64_t(1) << cs));
        if (!c.entry_ok()) { stream_fail(p.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        uint64_t bit0;
        const BitSrc src = stream_src(p.b.payload, p.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        dec.stream(p, c.i);
        uint32_t ctx = c.ctx, used = 0;
        bool bad = false;
        ByteOut bo;
        bo.init(p.b.out, a + c.first);
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) bo.put(dec.next(p, src, bc, ctx, used, bad));   // (stored in the step that turns bad, too)
        bo.flush();
        if (bad || used != c.end - c.start) stream_fail(p.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
    }
}

// EMIT = false: count the stream's symbols into sym_off[i] (scanned next); true: write them at out[sym_off[i] ...)
template <Model K, bool EMIT>
__global__ __launch_bounds__(Dec<K>::NT) void dec_walk_kernel(DecodeParams p, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    for (uint64_t i = gtid(); i <= p.b.n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (i == p.b.n) { if (!EMIT) p.b.sym_off[i] = 0; continue; }
        if (!EMIT) p.b.sym_off[i] = 0;
        if (p.b.stream_status[i] != MH_OK) continue;
        const uint64_t nb = p.b.nbits[i];
        if (!EMIT && nb > p.b.walk_max_bits) { stream_fail(p.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG); continue; }
        uint64_t count = 0;
        if (EMIT) {
            const uint64_t a = p.b.sym_off[i];
            count = p.b.sym_off[i + 1] - a;
            if (a + count > p.b.out_cap) { stream_fail(p.b, status, i, MH_ERR_CAPACITY, mhk::MHK_STATUS_CAPACITY); continue; }
        }
        uint64_t bit0;
        const BitSrc src = stream_src(p.b.payload, p.b.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0);
        dec.stream(p, i);
        uint32_t ctx = p.b.prev0, used = 0;
        bool bad = false;
        ByteOut bo;
        bo.init(p.b.out, EMIT ? p.b.sym_off[i] : 0);
        uint64_t k = 0;
        // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
        while (used < nb && !bad && (!EMIT || k < count)) {
            const uint32_t sym = dec.next(p, src, bc, ctx, used, bad);
            if (EMIT && !bad) bo.put(sym);
            ++k;
        }
        if (EMIT) bo.flush();
        if (bad || used != nb || (EMIT && k != count)) { stream_fail(p.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        if (!EMIT) p.b.sym_off[i] = k;                             // src/coding.cpp:158: the stream ends exactly at nbits
    }
}

// lds: the dynamic LDS of the model's tables (Shared), else 0
template <Model K>
hipError_t launch(const DecodeParams &p, size_t lds, void *d_ws, hipStream_t st) {
    constexpr int NT = Dec<K>::NT, PER_CU = Dec<K>::PER_CU;
    if (K == Model::Shared) {
        const int lds_max = 163840;
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(dec_idx_kernel<K>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(dec_walk_kernel<K, false>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(dec_walk_kernel<K, true>), lds_max);
        if (attr != hipSuccess) return attr;
        if (lds > 163840) return hipErrorInvalidValue;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.b.n;
    const DecLayout L = dec_layout(n);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dec_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p.b, status, stop);
    if (p.b.index) {
        const uint64_t W = work_items(n, p.b.sym_total, 1u << p.b.chunk_shift);
        hipLaunchKernelGGL(dec_idx_kernel<K>, dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, status, stop);
        return hipGetLastError();
    }
    const dim3 grid(grid_for(n + 1, NT, PER_CU));
    hipLaunchKernelGGL((dec_walk_kernel<K, false>), grid, dim3(NT), lds, st, p, status, stop);
    if ((e = scan_exclusive(p.b.sym_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL((dec_walk_kernel<K, true>), grid, dim3(NT), lds, st, p, status, stop);
    return hipGetLastError();
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
    hipLaunchKernelGGL(batch_check_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p.in_off, p.n, p.total, status, stop);
    const int waves_per_block = B_THREADS / 64;
    hipLaunchKernelGGL(batch_enc_len_kernel, dim3(grid_for(U, waves_per_block, 2)), dim3(B_THREADS), 65536, st, p, U, ubits, stop);
    if ((e = scan_exclusive(ubits, U, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(batch_enc_sizes_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p.in_off, p.n, ubits, p.nbits, p.out_off, stop);
    if ((e = scan_exclusive(p.out_off, p.n + 1, sums, stop, st)) != hipSuccess) return e;
    const uint64_t bound_words = (p.total * uint64_t(p.max_len > 0 ? p.max_len : 1) / 8 + p.n + 4) / 4;
    hipLaunchKernelGGL(batch_zero_kernel, dim3(grid_for(bound_words, 256, 8)), dim3(256), 0, st, p.out_off + p.n, p.out, p.cap, status, stop, tail);
    hipLaunchKernelGGL(batch_enc_emit_kernel, dim3(grid_for(U, waves_per_block, 1)), dim3(B_THREADS), 131072, st, p, U, ubits, tail, stop);
    hipLaunchKernelGGL(batch_tail_kernel, dim3(1), dim3(1), 0, st, p.out_off + p.n, p.out, tail, stop);
    return hipGetLastError();
}

hipError_t launch_decode(const DecodeParams &p, Model model, void *d_ws, hipStream_t st) {
    switch (model) {
        case Model::Shared: return launch<Model::Shared>(p, tables_lds(p.b), d_ws, st);
        case Model::Set: return launch<Model::Set>(p, 0, d_ws, st);
        case Model::Shared2: return launch<Model::Shared2>(p, 0, d_ws, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace mhb
