// mh_recode.hip — a compressed batch's training histogram and the batch coded again under another model, without writing
// the decoded bytes (include/mh.h, "RE-CODING BATCHES").  The batch decoders hold every decoded byte in a register for one
// step; here that byte feeds a counter, or the destination model's code and a BitWriter, instead of a store.
//   recode_check_kernel      the batch checks (mhb::check_batch); out_off, nbits and dropped zeroed (this and the other kernels
//                            that never decode — sizes, cap, zero, tail — are in mh_recode_dev.hpp)
//   recode_idx_len_kernel    one lane per (stream, chunk): decodes under src, sums dst's code lengths and the symbols without a code
//   recode_comb_kernel       the chunks of failed streams count 0 bits; the dropped symbols of the others go to dropped[i]
//   (scan)                   chunk bits -> bit offsets (mh_batch_dev.hpp); then payload bytes -> out_off
//   recode_sizes_kernel      stream i: nbits from the scanned chunk bits, its bytes into out_off
//   recode_cap_kernel        index-free: more symbols than the destination index was sized for -> MHK_STATUS_CAPACITY
//   recode_zero_kernel       clears the payload (edge words are OR-ed) or reports that it does not fit
//   recode_idx_emit_kernel   decodes again and pushes (len8, code64) of dst through BitWriter; the chunk's index entry
//   recode_walk_kernel       index-free, one lane per stream: count (scans) emit, under the walk cap of batch_dec_walk_kernel
//   recode_tail_kernel       the bytes of the last, partial dword
//   histc_idx_kernel         one lane per (stream, chunk): counts the pairs as it decodes; a chunk that fails takes its own
//                            counts back; <FIX>: the chunks that passed inside a stream that failed take theirs back
//   histc_walk_kernel        index-free, one lane per stream: counts, and takes the stream's counts back when it fails
// Verdicts are the batch decoders': same checks, same statuses.  Every loop is bounded by a symbol count or nbits_i.  Shared
// source model: tables in LDS as load_tables lays them out; behind them dst's len8 image (64 KiB order 1, 256 B order 0)
// when it fits, else len8 comes from L2; code64 always comes from L2.  Model set: tables in L2, an order-0 len8 image in LDS.
// The counters: a direct-mapped cache of (pair -> u64) in the LDS the tables leave, 64-bit global atomics behind it.
#include "mh_recode.h"
#include "mh_batch_dev.hpp"
#include "mh_recode_dev.hpp"
#include "mh_each_dev.hpp"
#include "../../include/mh.h"

namespace mhr {

using mhb::BATCH_STATUS_ARG;
using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;

namespace {

using mhb::BitWriter;
using mhb::Chunk;
using mhb::chunk_of;
using mhb::fail;
using mhb::find_stream;
using mhb::grid_for;
using mhb::grid_threads;
using mhb::gtid;
using mhb::scan_exclusive;
using mhb::stopped;
using mhb::stream_fail;

constexpr int NT_SHARED = mhb::B_THREADS;          // batch_dec_idx_kernel's shape: one workgroup per CU beside the tables
constexpr int NT_EACH = 256;                       // each_dec_idx_kernel's
constexpr int LDS_MAX = 163840;

// the symbol decoder of a lane: the shared model's two-level tables, or stream i's slots
template <bool SHARED> struct Dec;
template <> struct Dec<true> {
    const uint16_t *lut;
    const uint32_t *sub_base;
    DecTables tabs;
    __device__ __forceinline__ Dec(const Src &s, unsigned char *smem) : tabs(mhb::load_tables(s.b, smem, lut, sub_base)) {}
    __device__ __forceinline__ void stream(const Src &, uint64_t) {}
    __device__ __forceinline__ uint32_t next(const Src &, const BitSrc &src, BitCursor &bc, uint32_t prev, uint32_t &used, bool &bad) const {
        return mhk::decode_one(lut, sub_base, tabs, src, bc, prev, used, bad);
    }
};
template <> struct Dec<false> {
    const uint32_t *row;
    bool o1;
    __device__ __forceinline__ Dec(const Src &, unsigned char *) : row(nullptr), o1(false) {}
    __device__ __forceinline__ void stream(const Src &s, uint64_t i) { row = s.set.ctx_slot + i * 256u; o1 = s.set.type[i] != 0; }
    __device__ __forceinline__ uint32_t next(const Src &s, const BitSrc &src, BitCursor &bc, uint32_t prev, uint32_t &used, bool &bad) const {
        return mhe::decode_sym(s.set, row, o1 ? prev : 0u, src, bc, used, bad);
    }
};

// dst's code lengths: one ds_read_u8 (DLDS) or a byte from L2; the index serves code64 too
template <bool DLDS> struct Lens {
    const uint8_t *g;
    const uint8_t *l;
    uint32_t mask;
    __device__ __forceinline__ Lens(const Dst &d, unsigned char *smem, uint32_t lds_at) : g(d.len8), l(smem + lds_at), mask(d.ctx_mask) {
        if (DLDS) {
            const uint32_t n16 = (d.ctx_mask ? 65536u : 256u) / 16u;
            uint4 *dl = reinterpret_cast<uint4 *>(smem + lds_at);
            for (uint32_t k = threadIdx.x; k < n16; k += blockDim.x) dl[k] = reinterpret_cast<const uint4 *>(d.len8)[k];
            __syncthreads();
        }
    }
    __device__ __forceinline__ uint32_t at(uint32_t prev, uint32_t sym) const { return ((prev & mask) << 8) | sym; }
    __device__ __forceinline__ uint32_t operator()(uint32_t idx) const {
        if constexpr (DLDS) return l[idx]; else return g[idx];
    }
};

// ------------------------------------------------------------------------------------------------ histogram

// Direct-mapped counters in LDS: slot -> (pair, u64 count); a pair that finds its slot taken goes to the 64-bit global
// counter.  Counts go up and down (a failed chunk takes its counts back): the sums wrap modulo 2^64 and are exact.
// nslot == 0: no LDS left, global atomics only.
struct PairCache {
    static constexpr uint32_t EMPTY = 0xFFFFFFFFu;
    unsigned long long *cnt;
    uint32_t *tag;
    uint32_t shift, nslot;
    bool o1;
    unsigned long long *g;
    __device__ __forceinline__ void init(unsigned char *smem, uint32_t lds_at, uint32_t log2n, uint32_t order, unsigned long long *counts) {
        nslot = log2n ? 1u << log2n : 0u;
        shift = 16u - log2n;
        cnt = reinterpret_cast<unsigned long long *>(smem + lds_at);
        tag = reinterpret_cast<uint32_t *>(cnt + nslot);
        o1 = order != 0;
        g = counts;
        for (uint32_t k = threadIdx.x; k < nslot; k += blockDim.x) { tag[k] = EMPTY; cnt[k] = 0ull; }
        __syncthreads();
    }
    __device__ __forceinline__ void add(uint32_t prev, uint32_t sym, int delta) {
        const uint32_t p = o1 ? (prev << 8 | sym) : sym;
        const unsigned long long d = static_cast<unsigned long long>(static_cast<long long>(delta));
        if (nslot) {
            const uint32_t slot = o1 ? ((p * 40503u) & 0xFFFFu) >> shift : p;      // (nslot >= 256: order 0 never collides)
            uint32_t t = tag[slot];
            if (t == EMPTY) {
                const uint32_t old = atomicCAS(&tag[slot], EMPTY, p);
                t = old == EMPTY ? p : old;
            }
            if (t == p) { atomicAdd(&cnt[slot], d); return; }
        }
        atomicAdd(&g[p], d);
    }
    __device__ __forceinline__ void flush() {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < nslot; k += blockDim.x) {
            const unsigned long long v = cnt[k];
            if (v) atomicAdd(&g[tag[k]], v);
        }
    }
};

// `count` symbols of chunk c from its entry, each pair counted `delta` times (0: decode only); returns the symbols done
template <bool SHARED>
__device__ __forceinline__ uint32_t walk_chunk(const Src &s, const Dec<SHARED> &dec, const Chunk &c, uint32_t count, int delta, PairCache &pc,
                                               uint32_t &used, bool &bad) {
    uint64_t bit0;
    const BitSrc src = mhb::stream_src(s.b.payload, s.b.pay_off[c.i], c.nb, bit0);
    BitCursor bc;
    bc.init(src, bit0 + c.start);
    uint32_t prev = c.ctx, t = 0;
    used = 0; bad = false;
    for (; t < count; ++t) {
        const uint32_t sym = dec.next(s, src, bc, prev, used, bad);
        if (bad) break;
        if (delta) pc.add(prev, sym, delta);
        prev = sym;
    }
    return t;
}

template <bool SHARED, bool FIX>
__global__ __launch_bounds__(SHARED ? NT_SHARED : NT_EACH) void histc_idx_kernel(HistParams p, uint64_t nwork, uint32_t lds_at, uint32_t log2n,
                                                                               int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    if (FIX && *reinterpret_cast<const volatile int *>(status) == 0) return;      // no stream failed: nothing to take back
    Dec<SHARED> dec(p.s, smem);
    PairCache pc;
    pc.init(smem, lds_at, log2n, p.order, p.counts);
    for (uint64_t base = uint64_t(blockIdx.x) * blockDim.x; base < nwork; base += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t w = base + threadIdx.x;
        Chunk c;
        if (w < nwork && chunk_of<false>(p.s.b, w, c)) {
            dec.stream(p.s, c.i);
            const int verdict = p.s.b.stream_status[c.i];
            uint32_t used; bool bad;
            if (!FIX && verdict != MH_ERR_ARG) {
                if (!c.entry_ok()) {
                    stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                } else {
                    const uint32_t done = walk_chunk<SHARED>(p.s, dec, c, c.nsym, 1, pc, used, bad);
                    if (bad || used != c.end - c.start) {
                        stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                        walk_chunk<SHARED>(p.s, dec, c, done, -1, pc, used, bad);
                    }
                }
            }
            if (FIX && verdict == MH_ERR_CORRUPT && c.entry_ok()) {               // (a chunk that failed has taken its counts back)
                walk_chunk<SHARED>(p.s, dec, c, c.nsym, 0, pc, used, bad);
                if (!bad && used == c.end - c.start) walk_chunk<SHARED>(p.s, dec, c, c.nsym, -1, pc, used, bad);
            }
        }
    }
    pc.flush();
}

// at most `limit` symbols of stream i from bit 0, each pair counted `delta` times; returns the symbols done
template <bool SHARED>
__device__ __forceinline__ uint64_t walk_stream(const Src &s, const Dec<SHARED> &dec, uint64_t i, uint64_t nb, uint64_t limit, int delta,
                                                PairCache &pc, uint32_t &used, bool &bad) {
    uint64_t bit0;
    const BitSrc src = mhb::stream_src(s.b.payload, s.b.pay_off[i], nb, bit0);
    BitCursor bc;
    bc.init(src, bit0);
    uint32_t prev = s.b.prev0;
    uint64_t k = 0;
    used = 0; bad = false;
    // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
    while (used < nb && k < limit) {
        const uint32_t sym = dec.next(s, src, bc, prev, used, bad);
        if (bad) break;
        pc.add(prev, sym, delta);
        prev = sym;
        ++k;
    }
    return k;
}

template <bool SHARED>
__global__ __launch_bounds__(SHARED ? NT_SHARED : NT_EACH) void histc_walk_kernel(HistParams p, uint32_t lds_at, uint32_t log2n, int *status,
                                                                                const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<SHARED> dec(p.s, smem);
    PairCache pc;
    pc.init(smem, lds_at, log2n, p.order, p.counts);
    const uint64_t n = p.s.b.n;
    for (uint64_t base = uint64_t(blockIdx.x) * blockDim.x; base < n; base += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        if (i < n && p.s.b.stream_status[i] == MH_OK) {
            const uint64_t nb = p.s.b.nbits[i];
            if (nb > p.s.b.walk_max_bits) {
                stream_fail(p.s.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
            } else {
                dec.stream(p.s, i);
                uint32_t used; bool bad;
                const uint64_t done = walk_stream<SHARED>(p.s, dec, i, nb, ~uint64_t(0), 1, pc, used, bad);
                if (bad || used != nb) {                            // src/coding.cpp:158: the stream ends exactly at nbits
                    stream_fail(p.s.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                    walk_stream<SHARED>(p.s, dec, i, nb, done, -1, pc, used, bad);
                }
            }
        }
    }
    pc.flush();
}

// ------------------------------------------------------------------------------------------------ re-code

template <bool SHARED, bool DLDS>
__global__ __launch_bounds__(SHARED ? NT_SHARED : NT_EACH) void recode_idx_len_kernel(RecodeParams p, uint64_t nwork, uint32_t lds_at,
                                                                                    unsigned long long *cbits, uint32_t *cdrop, int *status,
                                                                                    const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<SHARED> dec(p.s, smem);
    const Lens<DLDS> L(p.dst, smem, lds_at);
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of<false>(p.s.b, w, c) || p.s.b.stream_status[c.i] == MH_ERR_ARG) continue;
        if (!c.entry_ok()) { stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        dec.stream(p.s, c.i);
        uint32_t prev = c.ctx, used = 0, bits = 0, drops = 0;
        bool bad = false;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {
            const uint32_t sym = dec.next(p.s, src, bc, prev, used, bad);
            if (bad) break;
            const uint32_t l = L(L.at(prev, sym));
            bits += l;
            drops += l == 0u;
            prev = sym;
        }
        if (bad || used != c.end - c.start) { stream_fail(p.s.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        cbits[w] = bits;
        cdrop[w] = drops;
    }
}

__global__ __launch_bounds__(256) void recode_comb_kernel(RecodeParams p, uint64_t nwork, unsigned long long *cbits, const uint32_t *cdrop,
                                                          const int *stop) {
    if (stopped(stop)) return;
    const uint64_t w = gtid();
    if (w > nwork) return;
    unsigned long long v = 0;
    if (w < nwork) {
        const uint32_t cs = p.s.b.chunk_shift;
        const uint64_t i = find_stream(p.s.b.sym_off, p.s.b.n, cs, w);
        if (i < p.s.b.n) {
            const uint64_t a = p.s.b.sym_off[i], ni = p.s.b.sym_off[i + 1] - a;
            const uint64_t k = w - ((a >> cs) + i);
            if ((k << cs) < ni && p.s.b.stream_status[i] == MH_OK) {
                v = cbits[w];
                const uint32_t d = cdrop[w];
                if (d && p.dropped) atomicAdd(&p.dropped[i], static_cast<unsigned long long>(d));
            }
        }
    }
    cbits[w] = v;
}

template <bool SHARED, bool DLDS>
__global__ __launch_bounds__(SHARED ? NT_SHARED : NT_EACH) void recode_idx_emit_kernel(RecodeParams p, uint64_t nwork, uint32_t lds_at,
                                                                                     const unsigned long long *cbase, uint32_t *tail,
                                                                                     const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<SHARED> dec(p.s, smem);
    const Lens<DLDS> L(p.dst, smem, lds_at);
    const uint64_t bytes = p.out_off[p.s.b.n];
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint32_t cs = p.s.b.chunk_shift;
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of<false>(p.s.b, w, c) || p.s.b.stream_status[c.i] != MH_OK) continue;
        const unsigned long long b0 = cbase[w];
        const uint64_t rel = b0 - cbase[(p.s.b.sym_off[c.i] >> cs) + c.i];          // relative to the stream's own payload
        if (p.out_index) p.out_index[w] = (uint64_t(c.ctx) << 56) | rel;
        if (!p.out || cbase[w + 1] == b0) continue;
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        dec.stream(p.s, c.i);
        BitWriter bw;
        bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[c.i]) * 8u + rel);
        uint32_t prev = c.ctx, used = 0;
        bool bad = false;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {            // (the stream passed: bad stays false)
            const uint32_t sym = dec.next(p.s, src, bc, prev, used, bad);
            const uint32_t at = L.at(prev, sym);
            const uint32_t l = L(at);
            if (l) bw.code(p.dst.code64[at], l);                    // 0: the pair has no code, skipped (mh_model.hpp:21)
            prev = sym;
        }
        bw.finish();
    }
}

// EMIT = false: the stream's verdict, its symbols into sym_off[i] (scanned next), its dst bits and dropped symbols;
// true: its codes from out_off[i] and its index entries
template <bool SHARED, bool DLDS, bool EMIT>
__global__ __launch_bounds__(SHARED ? NT_SHARED : NT_EACH) void recode_walk_kernel(RecodeParams p, uint32_t lds_at, uint32_t *tail, int *status,
                                                                                 const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<SHARED> dec(p.s, smem);
    const Lens<DLDS> L(p.dst, smem, lds_at);
    const uint64_t n = p.s.b.n;
    const uint64_t bytes = EMIT ? p.out_off[n] : 0;
    const uint64_t tail_w = (bytes & 3u) ? bytes >> 2 : ~uint64_t(0);
    const uint32_t ocs = p.out_chunk_shift;
    for (uint64_t i = gtid(); i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (p.s.b.stream_status[i] != MH_OK) continue;
        const uint64_t nb = p.s.b.nbits[i];
        uint64_t a = 0, count = ~uint64_t(0);
        if (EMIT) {
            a = p.s.b.sym_off[i];
            count = p.s.b.sym_off[i + 1] - a;
            if (!count) continue;
        } else if (nb > p.s.b.walk_max_bits) {
            stream_fail(p.s.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
            continue;
        }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.s.b.payload, p.s.b.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0);
        dec.stream(p.s, i);
        BitWriter bw;
        if (EMIT && p.out) bw.init(reinterpret_cast<uint32_t *>(p.out), tail, tail_w, uint64_t(p.out_off[i]) * 8u);
        uint32_t prev = p.s.b.prev0, used = 0;
        bool bad = false;
        uint64_t k = 0, bits = 0, drops = 0;
        // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
        while (used < nb && !bad && k < count) {
            if (EMIT && p.out_index && (k & ((uint64_t(1) << ocs) - 1u)) == 0)
                p.out_index[(a >> ocs) + i + (k >> ocs)] = (uint64_t(prev) << 56) | bits;
            const uint32_t sym = dec.next(p.s, src, bc, prev, used, bad);
            if (bad) break;
            const uint32_t at = L.at(prev, sym);
            const uint32_t l = L(at);
            if (EMIT) { if (l && p.out) bw.code(p.dst.code64[at], l); }
            else drops += l == 0u;
            bits += l;
            prev = sym;
            ++k;
        }
        if (EMIT) { if (p.out) bw.finish(); continue; }
        if (bad || used != nb) { stream_fail(p.s.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        p.s.b.sym_off[i] = k;                                       // src/coding.cpp:158: the stream ends exactly at nbits
        p.out_nbits[i] = bits;
        if (p.dropped) p.dropped[i] = drops;
    }
}

template <bool SHARED>
hipError_t launch_hist(const HistParams &p, size_t lds_tables, void *d_ws, hipStream_t st) {
    constexpr int NT = SHARED ? NT_SHARED : NT_EACH;
    constexpr int PER_CU = SHARED ? 1 : 8;
    // the counters take what the tables leave, 12 bytes a slot: 256 .. 4096 slots (a model set: 1024), or none
    uint32_t log2n = 0;
    const size_t room = SHARED ? size_t(LDS_MAX) - lds_tables : size_t(12288);
    for (uint32_t k = 8; k <= 12; ++k)
        if ((size_t(12) << k) <= room) log2n = k;
    const size_t lds = lds_tables + (log2n ? size_t(12) << log2n : 0);
    const uint32_t lds_at = uint32_t(lds_tables);
    if (SHARED) {
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(histc_idx_kernel<SHARED, false>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(histc_idx_kernel<SHARED, true>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(histc_walk_kernel<SHARED>), LDS_MAX);
        if (attr != hipSuccess) return attr;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.s.b.n;
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e == hipSuccess) e = hipMemsetAsync(p.counts, 0, (p.order ? 65536u : 256u) * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(histc_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p.s, status, stop);
    if (p.s.b.index) {
        const uint64_t W = mhb::work_items(n, p.s.b.sym_total, 1u << p.s.b.chunk_shift);
        hipLaunchKernelGGL((histc_idx_kernel<SHARED, false>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, lds_at, log2n, status, stop);
        hipLaunchKernelGGL((histc_idx_kernel<SHARED, true>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, lds_at, log2n, status, stop);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((histc_walk_kernel<SHARED>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, lds_at, log2n, status, stop);
    return hipGetLastError();
}

template <bool SHARED, bool DLDS>
hipError_t launch_rc(const RecodeParams &p, size_t lds_tables, void *d_ws, hipStream_t st) {
    constexpr int NT = SHARED ? NT_SHARED : NT_EACH;
    constexpr int PER_CU = SHARED ? 1 : 8;
    const size_t lds = lds_tables + (DLDS ? (p.dst.ctx_mask ? 65536 : 256) : 0);
    const uint32_t lds_at = uint32_t(lds_tables);
    if (SHARED) {
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(recode_idx_len_kernel<SHARED, DLDS>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(recode_idx_emit_kernel<SHARED, DLDS>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(recode_walk_kernel<SHARED, DLDS, false>), LDS_MAX);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(recode_walk_kernel<SHARED, DLDS, true>), LDS_MAX);
        if (attr != hipSuccess) return attr;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.s.b.n;
    const uint64_t W = p.s.b.index ? mhb::work_items(n, p.s.b.sym_total, 1u << p.s.b.chunk_shift) : 0;
    const RecodeLayout L = recode_layout(n, W);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    uint32_t *tail = reinterpret_cast<uint32_t *>(ws + TAIL_AT);
    auto *cbits = reinterpret_cast<unsigned long long *>(ws + L.off_bits);
    auto *cdrop = reinterpret_cast<uint32_t *>(ws + L.off_drop);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e == hipSuccess && W) e = hipMemsetAsync(ws + L.off_bits, 0, L.off_sums - L.off_bits, st);    // chunk bits and dropped counts
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(recode_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, status, stop);
    if (p.s.b.index) {
        hipLaunchKernelGGL((recode_idx_len_kernel<SHARED, DLDS>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, lds_at, cbits, cdrop,
                           status, stop);
        hipLaunchKernelGGL(recode_comb_kernel, grid_threads(W + 1, 256), dim3(256), 0, st, p, W, cbits, cdrop, stop);
        if ((e = scan_exclusive(cbits, W + 1, sums, stop, st)) != hipSuccess) return e;
    } else {
        hipLaunchKernelGGL((recode_walk_kernel<SHARED, DLDS, false>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, lds_at, tail, status,
                           stop);
        if ((e = scan_exclusive(p.s.b.sym_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(recode_sizes_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, cbits, stop);
    if ((e = scan_exclusive(p.out_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    if (!p.s.b.index && p.out_index) hipLaunchKernelGGL(recode_cap_kernel, dim3(1), dim3(1), 0, st, p, status, stop);
    if (p.out) hipLaunchKernelGGL(recode_zero_kernel, dim3(grid_for(p.cap / 4 + 1, 256, 8)), dim3(256), 0, st, p, status, stop, tail);
    if (p.s.b.index) {
        if (p.out || p.out_index)
            hipLaunchKernelGGL((recode_idx_emit_kernel<SHARED, DLDS>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, lds_at, cbits, tail,
                               stop);
    } else if (p.out || p.out_index) {
        hipLaunchKernelGGL((recode_walk_kernel<SHARED, DLDS, true>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, lds_at, tail, status,
                           stop);
    }
    if (p.out) hipLaunchKernelGGL(recode_tail_kernel, dim3(1), dim3(1), 0, st, p, tail, stop);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_histogram_coded(const HistParams &p, bool shared, void *d_ws, hipStream_t st) {
    if (!shared) return launch_hist<false>(p, 0, d_ws, st);
    const size_t lds = mhb::tables_lds(p.s.b);
    if (lds > size_t(LDS_MAX)) return hipErrorInvalidValue;
    return launch_hist<true>(p, lds, d_ws, st);
}

hipError_t launch_recode(const RecodeParams &p, bool shared, void *d_ws, hipStream_t st) {
    // a model set's tables stay in L2 and eight workgroups share a CU: only an order-0 image (256 B) goes to LDS
    if (!shared) return p.dst.ctx_mask ? launch_rc<false, false>(p, 0, d_ws, st) : launch_rc<false, true>(p, 0, d_ws, st);
    const size_t lds = mhb::tables_lds(p.s.b);
    if (lds > size_t(LDS_MAX)) return hipErrorInvalidValue;
    const size_t img = p.dst.ctx_mask ? 65536 : 256;
    return lds + img <= size_t(LDS_MAX) ? launch_rc<true, true>(p, lds, d_ws, st) : launch_rc<true, false>(p, lds, d_ws, st);
}

}  // namespace mhr
