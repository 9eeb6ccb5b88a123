// mh_crc.hip — the CRC-32 of every stream of a compressed batch without writing the decoded bytes (include/mh.h, "DIGESTS
// OF BATCHES").  The batch decoders hold every decoded byte in a register for one step; here that byte feeds a CRC register
// (mh_crc.h) instead of a store: r = byte[(r ^ c) & 255] ^ (r >> 8), a second dependent LDS chain beside the decoder's
// (context -> table -> next context), not part of it.
//   crc_check_kernel    the batch checks (mhb::check_batch); d_crc and d_len zeroed; the tables into the workspace
//   crc_idx_kernel      one lane per (stream, chunk), register from 0 with no final XOR: R(chunk).  A chunk that passes gives
//                       R(chunk) * x^(8 * symbols behind it) to its stream by XOR: the lanes of a wave that hold the same
//                       stream reduce among themselves, then one 32-bit atomic XOR per (wave, stream) goes to d_crc[i]
//   crc_finish_kernel   one lane per stream, every chunk judged by now: the initial value and the final XOR for a stream
//                       that passed, 0 for one that failed
//   crc_walk_kernel     index-free, one lane per stream under the walk cap of dec_walk_kernel: the register carried
//                       through the whole walk, the symbols counted, finished in place
//   crc_raw_check_kernel, crc_raw_kernel   the same digests of uncompressed messages, one lane per 1 KiB piece, the same
//                       combine and crc_finish_kernel
// XOR is exact in any order, so the results do not depend on the schedule.  Verdicts are the batch decoders': same checks,
// same statuses.  Every loop is bounded by a symbol count, a byte count or nbits_i.  One kernel family serves three models
// (mhb::Dec<K>): a shared order-0/1 model (tables in LDS as load_tables lays them out, the 1 KiB byte table behind them when
// they leave room (TLDS), else read from the workspace), a model set and a shared order-2 model (tables in L2, the byte table
// in LDS at offset 0).
#include "mh_crc.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"               // (the scans of mh_batch_dev.hpp have no use here)
#include "mh_symdec_dev.hpp"
#pragma clang diagnostic pop
#include "../../include/mh.h"

namespace mhc {

using mhb::BATCH_STATUS_ARG;
using mhk::BitCursor;
using mhk::BitSrc;

namespace {

using mhb::check_batch;
using mhb::Chunk;
using mhb::chunk_of;
using mhb::Dec;
using mhb::fail;
using mhb::find_stream;
using mhb::grid_for;
using mhb::grid_threads;
using mhb::gtid;
using mhb::stopped;
using mhb::stream_fail;

constexpr uint64_t NO_STREAM = ~uint64_t(0);

// byte[c]: one ds_read_b32 (TLDS) or a 4-byte load from the workspace
template <bool TLDS> struct ByteTab {
    const uint32_t *t;
    __device__ __forceinline__ ByteTab(const uint32_t *ws_tab, unsigned char *smem, uint32_t lds_at)
        : t(TLDS ? reinterpret_cast<const uint32_t *>(smem + lds_at) : ws_tab) {
        if (TLDS) {
            uint32_t *d = reinterpret_cast<uint32_t *>(smem + lds_at);
            for (uint32_t k = threadIdx.x; k < 256u; k += blockDim.x) d[k] = ws_tab[k];
            __syncthreads();
        }
    }
    __device__ __forceinline__ uint32_t step(uint32_t r, uint32_t c) const { return t[(r ^ c) & 255u] ^ (r >> 8); }
};

// v of every lane whose key equals this lane's, XOR-ed into acc[key] by the first lane of each run.  Called by whole waves;
// equal keys sit in consecutive lanes (chunk and piece numbers ascend with the lane, NO_STREAM marks a lane without work).
__device__ __forceinline__ void wave_xor(uint64_t key, uint32_t v, uint32_t *acc) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t ok = __shfl_down(key, d, 64);
        const uint32_t ov = __shfl_down(v, d, 64);
        if (lane + d < 64u && ok == key) v ^= ov;
    }
    const uint64_t pk = __shfl_up(key, 1u, 64);
    if (key != NO_STREAM && (lane == 0 || pk != key) && v) atomicXor(acc + key, v);
}

__global__ __launch_bounds__(256) void crc_check_kernel(CrcParams p, CrcTables t, uint32_t *ws_tab, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i < 256u) ws_tab[i] = t.byte[i];
    else if (i < CRC_TABLE_WORDS) ws_tab[i] = t.pow8[i - 256u];
    if (i > p.b.n) return;
    if (i < p.b.n) {
        p.crc[i] = 0;
        if (p.len) p.len[i] = 0;
    }
    check_batch(p.b, i, status, stop);
}

template <Model K, bool TLDS>
__global__ __launch_bounds__(Dec<K>::NT) void crc_idx_kernel(CrcParams p, uint64_t nwork, const uint32_t *ws_tab, uint32_t lds_at, int *status,
                                                             const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    const ByteTab<TLDS> T(ws_tab, smem, lds_at);
    // every lane of a wave makes the same trips, so wave_xor always sees whole waves
    for (uint64_t base = uint64_t(blockIdx.x) * blockDim.x; base < nwork; base += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t w = base + threadIdx.x;
        uint64_t key = NO_STREAM;
        uint32_t v = 0;
        Chunk c;
        if (w < nwork && chunk_of<Dec<K>::O2>(p.b, w, c)) {
            key = c.i;
            if (p.b.stream_status[c.i] != MH_ERR_ARG) {
                bool bad = !c.entry_ok();
                uint32_t used = 0, r = 0;
                if (!bad) {
                    uint64_t bit0;
                    const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[c.i], c.nb, bit0);
                    BitCursor bc;
                    bc.init(src, bit0 + c.start);
                    dec.stream(p, c.i);
                    uint32_t ctx = c.ctx;
                    for (uint32_t t = 0; t < c.nsym && !bad; ++t) r = T.step(r, dec.next(p, src, bc, ctx, used, bad));
                    bad |= used != c.end - c.start;
                }
                if (bad) stream_fail(p.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                else v = gf_mul(r, pow8_of(ws_tab + 256, c.ni - c.first - c.nsym));
            }
        }
        wave_xor(key, v, p.crc);
    }
}

// status: the streams' verdicts (coded: p.b.stream_status), or nullptr: every stream passed (raw)
__global__ __launch_bounds__(256) void crc_finish_kernel(uint32_t *crc, unsigned long long *len, const unsigned long long *off, const int *sst,
                                                         uint64_t n, const uint32_t *ws_tab, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t i = gtid();
    if (i >= n) return;
    if (sst && sst[i] != MH_OK) { crc[i] = 0; return; }           // (len_i is 0 since the check kernel)
    const uint64_t ni = off[i + 1] - off[i];
    crc[i] = finish_of(ws_tab + 256, crc[i], ni);
    if (len) len[i] = ni;
}

template <Model K, bool TLDS>
__global__ __launch_bounds__(Dec<K>::NT) void crc_walk_kernel(CrcParams p, const uint32_t *ws_tab, uint32_t lds_at, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    const ByteTab<TLDS> T(ws_tab, smem, lds_at);
    for (uint64_t i = gtid(); i < p.b.n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (p.b.stream_status[i] != MH_OK) continue;
        const uint64_t nb = p.b.nbits[i];
        if (nb > p.b.walk_max_bits) { stream_fail(p.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG); continue; }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0);
        dec.stream(p, i);
        uint32_t ctx = p.b.prev0, used = 0, r = CRC_ONES;
        bool bad = false;
        uint64_t k = 0;
        // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
        while (used < nb && !bad) {
            r = T.step(r, dec.next(p, src, bc, ctx, used, bad));
            ++k;
        }
        if (bad || used != nb) { stream_fail(p.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        p.crc[i] = r ^ CRC_ONES;                                  // src/coding.cpp:158: the stream ends exactly at nbits
        if (p.len) p.len[i] = k;
    }
}

__global__ __launch_bounds__(256) void crc_raw_check_kernel(const uint64_t *in_off, uint64_t n, uint64_t total, uint32_t *crc, CrcTables t,
                                                            uint32_t *ws_tab, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i < 256u) ws_tab[i] = t.byte[i];
    else if (i < CRC_TABLE_WORDS) ws_tab[i] = t.pow8[i - 256u];
    if (i > n) return;
    if (i < n) crc[i] = 0;
    if (mhb::offsets_bad(in_off, n, total, i)) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
}

__global__ __launch_bounds__(256) void crc_raw_kernel(const uint8_t *data, const uint64_t *in_off, uint64_t n, uint64_t npieces, uint32_t *crc,
                                                      const uint32_t *ws_tab, const int *stop) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[1024];
    if (stopped(stop)) return;
    const ByteTab<true> T(ws_tab, smem, 0);
    for (uint64_t base = uint64_t(blockIdx.x) * blockDim.x; base < npieces; base += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t w = base + threadIdx.x;
        uint64_t key = NO_STREAM;
        uint32_t v = 0;
        if (w < npieces) {
            const uint64_t i = find_stream(in_off, n, RAW_SHIFT, w);
            if (i < n) {
                const uint64_t a = in_off[i], ni = in_off[i + 1] - a;
                const uint64_t first = (w - ((a >> RAW_SHIFT) + i)) << RAW_SHIFT;
                if (first < ni) {
                    key = i;
                    const uint32_t cnt = uint32_t(ni - first < RAW_PIECE ? ni - first : RAW_PIECE);
                    uint32_t r = 0;
                    for (uint32_t o = 0; o < cnt; o += 16u) {
                        const uint32_t m = cnt - o < 16u ? cnt - o : 16u;
                        uint32_t x[4];
                        mhb::load16(data + a + first + o, m, x);
                        for (uint32_t t = 0; t < m; ++t) r = T.step(r, mhb::byte_of(x, t));
                    }
                    v = gf_mul(r, pow8_of(ws_tab + 256, ni - first - cnt));
                }
            }
        }
        wave_xor(key, v, crc);
    }
}

template <Model K, bool TLDS>
hipError_t launch(const CrcParams &p, size_t lds_tables, void *d_ws, hipStream_t st) {
    constexpr int NT = Dec<K>::NT, PER_CU = Dec<K>::PER_CU;
    static constexpr CrcTables tables = make_tables();
    const size_t lds = lds_tables + (TLDS ? 1024 : 0);
    const uint32_t lds_at = uint32_t(lds_tables);
    if (K == Model::Shared) {
        const int lds_max = 163840;
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(crc_idx_kernel<K, TLDS>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(crc_walk_kernel<K, TLDS>), lds_max);
        if (attr != hipSuccess) return attr;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.b.n;
    const CrcLayout L = crc_layout(n);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    uint32_t *ws_tab = reinterpret_cast<uint32_t *>(ws + L.off_tab);
    const hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crc_check_kernel, grid_threads((n + 1 > CRC_TABLE_WORDS ? n + 1 : CRC_TABLE_WORDS), 256), dim3(256), 0, st, p, tables, ws_tab,
                       status, stop);
    if (p.b.index) {
        const uint64_t W = mhb::work_items(n, p.b.sym_total, 1u << p.b.chunk_shift);
        hipLaunchKernelGGL((crc_idx_kernel<K, TLDS>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, ws_tab, lds_at, status, stop);
        hipLaunchKernelGGL(crc_finish_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p.crc, p.len, p.b.sym_off, p.b.stream_status, n, ws_tab, stop);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((crc_walk_kernel<K, TLDS>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, ws_tab, lds_at, status, stop);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_crc(const CrcParams &p, Model model, void *d_ws, hipStream_t st) {
    // tables in L2: the byte table alone in LDS, at offset 0
    if (model == Model::Set) return launch<Model::Set, true>(p, 0, d_ws, st);
    if (model == Model::Shared2) return launch<Model::Shared2, true>(p, 0, d_ws, st);
    // the tables as launch_decode places them; the byte table behind them when 1 KiB is left of the 160 KiB
    const size_t lds = mhb::tables_lds(p.b);
    if (lds > 163840) return hipErrorInvalidValue;
    return lds + 1024 <= 163840 ? launch<Model::Shared, true>(p, lds, d_ws, st) : launch<Model::Shared, false>(p, lds, d_ws, st);
}

hipError_t launch_crc_raw(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total, uint32_t *d_crc, void *d_ws,
                          hipStream_t st) {
    static constexpr CrcTables tables = make_tables();
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    uint32_t *ws_tab = reinterpret_cast<uint32_t *>(ws + crc_layout(0).off_tab);
    const uint64_t np = raw_pieces(n, total);
    const hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crc_raw_check_kernel, grid_threads((n + 1 > CRC_TABLE_WORDS ? n + 1 : CRC_TABLE_WORDS), 256), dim3(256), 0, st, d_in_off, n,
                       total, d_crc, tables, ws_tab, status, stop);
    hipLaunchKernelGGL(crc_raw_kernel, dim3(grid_for(np, 256, 8)), dim3(256), 0, st, d_data, d_in_off, n, np, d_crc, ws_tab, stop);
    hipLaunchKernelGGL(crc_finish_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, d_crc, static_cast<unsigned long long *>(nullptr),
                       reinterpret_cast<const unsigned long long *>(d_in_off), static_cast<const int *>(nullptr), n, ws_tab, stop);
    return hipGetLastError();
}

}  // namespace mhc
