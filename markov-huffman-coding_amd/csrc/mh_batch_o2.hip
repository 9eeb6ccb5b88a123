// mh_batch_o2.hip — batches of independent streams under one shared ORDER-2 model (include/mh.h, "BATCHES OF ORDER-2
// STREAMS"; extension, parity unpinned).  Every stream starts in context (prev0, prev0), as mh_encode starts an order-2 stream.
//   batch2_hist_fixup_kernel   the order-2 histogram of the concatenation counted each stream's first two symbols in contexts
//                              that reach into the streams in front of it: one thread per stream moves them to its own
//   batch2_enc_len_kernel      one wave per (stream, 1 KiB sub-step): the sub-step's payload bits
//   batch_check_kernel, batch_enc_sizes_kernel, batch_zero_kernel, batch_tail_kernel, batch_scan_*
//                              (mh_batch_dev.hpp) the encoder's stages that do not look at the model: the offset check, unit
//                              bits -> stream-relative bit offsets, payload bytes -> out_off, the zeroed output, its last dword
//   batch2_enc_emit_kernel     one wave per (stream, 1 KiB sub-step): codes through the live contexts' LDS image
//                              (o2hot_lookup16) when the model hands one over, escapes and every other model through the
//                              packed (len << 56 | code) table in L2, codes over 56 bits through (len8, code64); the
//                              sub-step's index entries
// The work units and their finder, the model-free stages, the bit writer and the byte output are the order-0/1 batch's
// (mh_batch_dev.hpp); the decoder is mh_batch.hip's dec_*_kernel<Model::Shared2>.  The kernels of the single-stream order-2
// path are not changed.
#include "mh_batch_o2.h"
#include "mh_batch_dev.hpp"
#include "mh_decode_dev.hpp"
#include "mh_dev.hpp"
#include "../../include/mh.h"

namespace mhb {

namespace {

// The live contexts' image and its sixteen-symbol lookup: a copy of mh_encode.hip's O2H_* and o2hot_lookup16 (the layout is
// described there).  It stays a copy so that the single-stream encoder's sources, and the counter figures committed against
// them, do not change.
constexpr uint32_t O2H_MAP_OFF = 256, O2H_HOT_OFF = 256 + 64 * 64 * 2;
__device__ __forceinline__ void o2hot_lookup16(const unsigned char *img, const uint4 &x4, uint32_t ctx, uint32_t (&e)[16]) {
    const uint16_t *ctxmap = reinterpret_cast<const uint16_t *>(img + O2H_MAP_OFF);
    const uint16_t *hot = reinterpret_cast<const uint16_t *>(img + O2H_HOT_OFF);
    const uint32_t x[4] = {x4.x, x4.y, x4.z, x4.w};
    uint32_t id[18];
    id[0] = img[ctx >> 8];
    id[1] = img[ctx & 255u];
#pragma unroll
    for (int j = 0; j < 16; ++j) id[2 + j] = img[(x[j >> 2] >> (8 * (j & 3))) & 255u];
    // Both tables are read at a column XOR-ed with the id of the byte in front: with a few dozen byte values, and
    // rows of 64 two-byte entries = 32 banks, the bank of a plain [row][id] access is id / 2 whatever the row — every
    // lane that looks at a frequent letter lands on the same bank (the builder stores the rows permuted accordingly)
    uint32_t cs[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) cs[j] = ctxmap[(id[j] << 6) | (id[j + 1] ^ id[j])];
#pragma unroll
    for (int j = 0; j < 16; ++j) e[j] = hot[(cs[j] << 6) | (id[j + 2] ^ id[j + 1])];
}

constexpr uint32_t HOT_ESCAPE = 0xD000u;          // image entries at or above: longer than 12 bits (ENC16_ESCAPE) — the L2 tables

// ------------------------------------------------------------------------------------------------ histogram fix-up

// Position g of the concatenation was counted in context (byte g-2, byte g-1), prev0 standing in for the bytes in front of
// position 0; stream [a, b) wants prev0 for every byte in front of a.  The two differ at a and a + 1 only (and only where the
// stream has those positions): a run of one-byte streams is handled too, since the context of the concatenation is read from
// the concatenation itself.  Every position is moved by the one stream that owns it, so the total is conserved.
__global__ void batch2_hist_fixup_kernel(const uint8_t *data, const uint64_t *off, uint64_t n, uint64_t total, uint32_t prev0,
                                         unsigned long long *counts, int *status) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > n) return;
    const bool bad = offsets_bad(off, n, total, i);
    if (bad) atomicExch(status, BATCH_STATUS_ARG);               // (the conservation check's CORRUPT gives way: the input was wrong)
    if (i >= n || bad) return;
    const uint64_t a = off[i], b = off[i + 1];
    if (b <= a || b > total) return;
    for (uint64_t g = a; g < b && g < a + 2; ++g) {
        const uint32_t sym = data[g];
        const uint32_t c2 = g >= 2 ? data[g - 2] : prev0, c1 = g >= 1 ? data[g - 1] : prev0;
        const uint32_t s2 = g >= a + 2 ? data[g - 2] : prev0, s1 = g >= a + 1 ? data[g - 1] : prev0;
        const uint32_t was = (c2 << 8) | c1, own = (s2 << 8) | s1;
        if (was == own) continue;
        atomicAdd(&counts[(was << 8) | sym], ~0ull);              // -1
        atomicAdd(&counts[(own << 8) | sym], 1ull);
    }
}

// ------------------------------------------------------------------------------------------------ encode

template <bool HOT>
__device__ __forceinline__ void load_image(const EncBatchO2Params &p, unsigned char *smem) {
    if (!HOT) return;
    for (uint32_t k = threadIdx.x; k < (p.o2img_bytes + 15u) / 16u; k += B_THREADS)
        reinterpret_cast<uint4 *>(smem)[k] = reinterpret_cast<const uint4 *>(p.o2img)[k];
    __syncthreads();
}

// the lane's sixteen image entries (HOT) — escapes and models without an image go to the L2 tables symbol by symbol
template <bool HOT>
__device__ __forceinline__ void image16(const unsigned char *smem, const Unit &l, uint32_t (&e)[16]) {
    if (HOT) {
        o2hot_lookup16(smem, make_uint4(l.x[0], l.x[1], l.x[2], l.x[3]), l.ctx, e);
    } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) e[t] = HOT_ESCAPE;
    }
}

__device__ __forceinline__ uint32_t len_l2(const EncBatchO2Params &p, uint32_t key) {
    const uint32_t len = p.len8[key];
    return len > 64u ? 0u : len;                                // 0: the pair has no code, skipped (mh_model.hpp:21)
}

__device__ __forceinline__ void code_l2(const EncBatchO2Params &p, uint32_t key, uint32_t &len, uint64_t &code) {
    const uint64_t e = p.enc64 ? p.enc64[key] : 0xFF00000000000000ull;
    len = uint32_t(e >> 56);
    code = e & 0x00FFFFFFFFFFFFFFull;
    if (len == 255u) {                                          // longer than 56 bits (or no packed table)
        len = p.len8[key];
        code = p.code64[key];
    }
    if (len > 64u) len = 0;
}

template <bool HOT>
__global__ __launch_bounds__(B_THREADS) void batch2_enc_len_kernel(EncBatchO2Params p, uint64_t nunits, unsigned long long *ubits, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    load_image<HOT>(p, smem);
    const uint64_t nw = uint64_t(gridDim.x) * (B_THREADS / 64);
    for (uint64_t u = uint64_t(blockIdx.x) * (B_THREADS / 64) + threadIdx.x / 64; u < nunits; u += nw) {
        Unit l;
        uint32_t bits = 0;
        if (unit_of<2>(p.data, p.in_off, p.n, p.prev0, u, l)) {
            uint32_t e[16];
            image16<HOT>(smem, l, e);
            uint32_t ctx = l.ctx;
#pragma unroll
            for (uint32_t t = 0; t < B_VEC; ++t) {                // (unrolled: the byte index stays a constant, no scratch)
                const uint32_t key = (ctx << 8) | byte_of(l.x, t);
                if (t < l.cnt) bits += e[t] < HOT_ESCAPE ? e[t] >> 12 : len_l2(p, key);
                ctx = key & 0xFFFFu;
            }
        }
        bits = mhk::wave_sum(bits);
        if (mhk::lane_id() == 0) ubits[u] = bits;
    }
}

template <bool HOT>
__global__ __launch_bounds__(B_THREADS) void batch2_enc_emit_kernel(EncBatchO2Params p, uint64_t nunits, const unsigned long long *ubase,
                                                                    uint32_t *tail, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    load_image<HOT>(p, smem);
    const uint64_t bytes = p.out_off[p.n];
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint64_t nw = uint64_t(gridDim.x) * (B_THREADS / 64);
    for (uint64_t u = uint64_t(blockIdx.x) * (B_THREADS / 64) + threadIdx.x / 64; u < nunits; u += nw) {
        Unit l;
        if (!unit_of<2>(p.data, p.in_off, p.n, p.prev0, u, l)) continue;   // wave-uniform
        uint32_t e[16];
        image16<HOT>(smem, l, e);
        uint32_t len[16], bits = 0, ctx = l.ctx;
        uint64_t code[16];
#pragma unroll
        for (uint32_t t = 0; t < B_VEC; ++t) {
            const uint32_t key = (ctx << 8) | byte_of(l.x, t);
            len[t] = 0; code[t] = 0;
            if (t < l.cnt) {
                if (e[t] < HOT_ESCAPE) { len[t] = e[t] >> 12; code[t] = e[t] & 0xFFFu; }
                else code_l2(p, key, len[t], code[t]);
            }
            bits += len[t];
            ctx = key & 0xFFFFu;
        }
        const uint32_t excl = mhk::wave_inclusive_sum(bits) - bits;
        const uint64_t sbit = (ubase[u] - ubase[l.ub]) + excl;     // stream-relative
        if (p.index && l.cnt && (l.j0 & ((uint64_t(1) << p.chunk_shift) - 1u)) == 0)
            p.index[(l.a >> p.chunk_shift) + l.i + (l.j0 >> p.chunk_shift)] = (uint64_t(l.ctx) << 48) | sbit;
        if (!bits) continue;
        BitWriter bw;
        bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[l.i]) * 8u + sbit);
#pragma unroll
        for (uint32_t t = 0; t < B_VEC; ++t) bw.code(code[t], len[t]);
        bw.finish();
    }
}

}  // namespace

hipError_t launch_hist2_fixup(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total, uint32_t prev0,
                              unsigned long long *d_counts, int *d_status, hipStream_t st) {
    const uint64_t threads = n + 1;
    hipLaunchKernelGGL(batch2_hist_fixup_kernel, dim3(uint32_t((threads + 255) / 256)), dim3(256), 0, st, d_data, d_in_off, n, total, prev0,
                       d_counts, d_status);
    return hipGetLastError();
}

hipError_t launch_encode_batch_o2(const EncBatchO2Params &p, void *d_ws, hipStream_t st) {
    const bool hot = p.o2img && p.o2img_bytes && p.o2img_bytes <= uint32_t(mhk::LEN_LDS_BYTES);
    const size_t lds = hot ? ((size_t(p.o2img_bytes) + 15) & ~size_t(15)) : 0;
    if (hot) {
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(batch2_enc_len_kernel<true>), int(lds));   // (per call: per device)
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(batch2_enc_emit_kernel<true>), int(lds));
        if (attr != hipSuccess) return attr;
    }
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
    const dim3 len_grid(grid_for(U, waves_per_block, 2)), emit_grid(grid_for(U, waves_per_block, 1));
    if (hot) hipLaunchKernelGGL(batch2_enc_len_kernel<true>, len_grid, dim3(B_THREADS), lds, st, p, U, ubits, stop);
    else hipLaunchKernelGGL(batch2_enc_len_kernel<false>, len_grid, dim3(B_THREADS), 0, st, p, U, ubits, stop);
    if ((e = scan_exclusive(ubits, U, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(batch_enc_sizes_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p.in_off, p.n, ubits, p.nbits, p.out_off, stop);
    if ((e = scan_exclusive(p.out_off, p.n + 1, sums, stop, st)) != hipSuccess) return e;
    const uint64_t bound_words = (p.total * uint64_t(p.max_len > 0 ? p.max_len : 1) / 8 + p.n + 4) / 4;
    hipLaunchKernelGGL(batch_zero_kernel, dim3(grid_for(bound_words, 256, 8)), dim3(256), 0, st, p.out_off + p.n, p.out, p.cap, status, stop, tail);
    if (hot) hipLaunchKernelGGL(batch2_enc_emit_kernel<true>, emit_grid, dim3(B_THREADS), lds, st, p, U, ubits, tail, stop);
    else hipLaunchKernelGGL(batch2_enc_emit_kernel<false>, emit_grid, dim3(B_THREADS), 0, st, p, U, ubits, tail, stop);
    hipLaunchKernelGGL(batch_tail_kernel, dim3(1), dim3(1), 0, st, p.out_off + p.n, p.out, tail, stop);
    return hipGetLastError();
}

}  // namespace mhb
