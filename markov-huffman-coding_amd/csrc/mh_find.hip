// mh_find.hip — pattern search in batches of order-0/1 streams without writing the decoded bytes (include/mh.h, "SEARCH IN
// BATCHES").  The batch decoders hold every decoded byte in a register for one step; here that byte feeds a Shift-And
// automaton (mh_find.h) instead of a store: D = ((D << 1) | first) & mask[c], hits = D & last.  The update hangs off the
// decoder's dependent chain (context -> table -> next context), it is not part of it.
//   find_check_kernel        the batch checks (mhb::check_batch); hit_off zeroed; the masks into the workspace
//   find_idx_count_kernel    one lane per (stream, chunk), D from 0: the hits that end in the chunk, the chunk's end state, and
//                            a tail into the next chunk with no new starts (the hits that begin here and end there)
//   find_comb_kernel         hits that end in chunk k = own(k) + tail(k - 1); 0 for a failed stream (every chunk is judged by now)
//   (scan)                   exclusive scan over the chunks (mh_batch_dev.hpp)
//   find_off_kernel          hit_off from the scanned counts; hits beyond hit_cap -> MHK_STATUS_CAPACITY
//   find_idx_emit_kernel     only lanes whose chunk has hits: decode again from the kept state of the chunk in front, so the
//                            records come out in (end, pattern) order
//   find_walk_kernel         index-free, one lane per stream: count (scan) emit, under the walk cap of dec_walk_kernel
//   find_cap_kernel          index-free: hits beyond hit_cap -> MHK_STATUS_CAPACITY
// A chunk that is not its stream's last has chunk_symbols >= 256 > 63 symbols, so a state started at 0 is the true state at
// its end, and a hit spans at most two chunks.  Verdicts are the batch decoders': same checks, same statuses.  Every loop is
// bounded by a symbol count or nbits_i.  One kernel family serves three models (Dec<K>): a shared order-0/1 model (tables in
// LDS as load_tables lays them out, the 2 KiB of masks behind them when they leave room (MLDS), else read from the workspace),
// a model set and a shared order-2 model (tables in L2, masks in LDS at offset 0).
#include "mh_find.h"
#include "mh_symdec_dev.hpp"
#include "../../include/mh.h"

namespace mhf {

using mhb::BATCH_STATUS_ARG;
using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;

namespace {

using mhb::check_batch;
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

using mhb::Dec;                                               // the symbol decoder of a lane, one policy per model (mh_symdec_dev.hpp)

// mask[c]: one ds_read_b64 (MLDS) or an 8-byte load from the workspace
template <bool MLDS> struct Masks {
    const uint64_t *g;
    const uint64_t *l;
    __device__ __forceinline__ Masks(const uint64_t *ws_mask, unsigned char *smem, uint32_t lds_at) : g(ws_mask), l(reinterpret_cast<const uint64_t *>(smem + lds_at)) {
        if (MLDS) {
            uint64_t *d = reinterpret_cast<uint64_t *>(smem + lds_at);
            for (uint32_t k = threadIdx.x; k < 256u; k += blockDim.x) d[k] = ws_mask[k];
            __syncthreads();
        }
    }
    __device__ __forceinline__ uint64_t operator()(uint32_t c) const {
        if constexpr (MLDS) return l[c]; else return g[c];
    }
};

// one record: pattern j = the rank of bit b among `last`; its length from the pattern's lowest bit (the highest bit of `first` <= b)
__device__ __forceinline__ void put_hit(const FindParams &p, uint64_t r, uint64_t i, uint64_t end, uint32_t b) {
    const uint32_t j = uint32_t(__popcll(p.last & ((1ull << b) - 1ull)));
    const uint32_t lo = 63u - uint32_t(__clzll((long long)(p.first & ((2ull << b) - 1ull))));
    const uint64_t len = b - lo + 1u;
    p.hits[3 * r] = i;
    p.hits[3 * r + 1] = end - len;
    p.hits[3 * r + 2] = end;
    if (p.hit_pattern) p.hit_pattern[r] = j;
}

__global__ __launch_bounds__(256) void find_check_kernel(FindParams p, Automaton a, uint64_t *ws_mask, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i < 256u) ws_mask[i] = a.mask[i];
    if (i > p.b.n) return;
    p.hit_off[i] = 0;
    check_batch(p.b, i, status, stop);
}

template <Model K, bool MLDS>
__global__ __launch_bounds__(Dec<K>::NT) void find_idx_count_kernel(FindParams p, uint64_t nwork, const uint64_t *ws_mask, uint32_t lds_at,
                                                                    unsigned long long *state, uint32_t *own, uint32_t *tail, int *status,
                                                                    const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    const Masks<MLDS> M(ws_mask, smem, lds_at);
    const uint64_t F = p.first, L = p.last;
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of<Dec<K>::O2>(p.b, w, c) || p.b.stream_status[c.i] == MH_ERR_ARG) continue;
        if (!c.entry_ok()) { stream_fail(p.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        dec.stream(p, c.i);
        uint32_t ctx = c.ctx, used = 0, cnt = 0;
        bool bad = false;
        uint64_t D = 0;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {
            const uint32_t sym = dec.next(p, src, bc, ctx, used, bad);
            D = ((D << 1) | F) & M(sym);
            cnt += uint32_t(__popcll(D & L));
        }
        if (bad || used != c.end - c.start) { stream_fail(p.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        own[w] = cnt;
        state[w] = D;
        if (c.last || !D) continue;
        // the tail: what began in this chunk and still completes in the next one.  No new starts (the bit that leaves one
        // pattern's top must not start the next), no verdict: the next chunk's own lane judges that chunk.
        const uint64_t rest = c.ni - c.first - c.nsym;
        const uint32_t lim = uint32_t(rest < p.max_len - 1u ? rest : p.max_len - 1u);
        uint32_t tc = 0;
        for (uint32_t t = 0; t < lim && D; ++t) {
            const uint32_t sym = dec.next(p, src, bc, ctx, used, bad);
            if (bad) break;
            D = (D << 1) & ~F & M(sym);
            tc += uint32_t(__popcll(D & L));
        }
        tail[w] = tc;
    }
}

__global__ __launch_bounds__(256) void find_comb_kernel(FindParams p, uint64_t nwork, const uint32_t *own, const uint32_t *tail,
                                                        unsigned long long *cnt, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t w = gtid();
    if (w > nwork) return;
    unsigned long long v = 0;
    if (w < nwork) {
        const uint32_t cs = p.b.chunk_shift;
        const uint64_t i = find_stream(p.b.sym_off, p.b.n, cs, w);
        if (i < p.b.n) {
            const uint64_t a = p.b.sym_off[i], ni = p.b.sym_off[i + 1] - a;
            const uint64_t k = w - ((a >> cs) + i);
            if ((k << cs) < ni && p.b.stream_status[i] == MH_OK) v = uint64_t(own[w]) + (k ? tail[w - 1] : 0u);
        }
    }
    cnt[w] = v;
}

__global__ __launch_bounds__(256) void find_off_kernel(FindParams p, uint64_t nwork, const unsigned long long *cnt, int *status, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t i = gtid();
    if (i > p.b.n) return;
    const unsigned long long v = i < p.b.n ? cnt[(p.b.sym_off[i] >> p.b.chunk_shift) + i] : cnt[nwork];
    p.hit_off[i] = v;
    if (i == p.b.n && p.hits && v > p.hit_cap) fail(status, mhk::MHK_STATUS_CAPACITY);
}

template <Model K, bool MLDS>
__global__ __launch_bounds__(Dec<K>::NT) void find_idx_emit_kernel(FindParams p, uint64_t nwork, const uint64_t *ws_mask, uint32_t lds_at,
                                                                   const unsigned long long *state, const unsigned long long *cnt,
                                                                   const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    const Masks<MLDS> M(ws_mask, smem, lds_at);
    const uint64_t F = p.first, L = p.last;
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t r0 = cnt[w], r1 = cnt[w + 1];
        if (r1 == r0 || r0 >= p.hit_cap) continue;                // (a chunk with hits belongs to a stream that passed)
        Chunk c;
        if (!chunk_of<Dec<K>::O2>(p.b, w, c)) continue;
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        dec.stream(p, c.i);
        uint32_t ctx = c.ctx, used = 0;
        bool bad = false;
        uint64_t D = c.first ? state[w - 1] : 0ull, r = r0;
        for (uint32_t t = 0; t < c.nsym && r < r1 && !bad; ++t) {
            const uint32_t sym = dec.next(p, src, bc, ctx, used, bad);
            D = ((D << 1) | F) & M(sym);
            for (uint64_t h = D & L; h && r < r1; h &= h - 1ull, ++r)
                if (r < p.hit_cap) put_hit(p, r, c.i, c.first + t + 1u, uint32_t(__builtin_ctzll(h)));
        }
    }
}

// EMIT = false: the stream's verdict and its hit count into hit_off[i] (scanned next); true: its records from hit_off[i]
template <Model K, bool MLDS, bool EMIT>
__global__ __launch_bounds__(Dec<K>::NT) void find_walk_kernel(FindParams p, const uint64_t *ws_mask, uint32_t lds_at, int *status,
                                                               const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    const Masks<MLDS> M(ws_mask, smem, lds_at);
    const uint64_t F = p.first, L = p.last;
    for (uint64_t i = gtid(); i < p.b.n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (p.b.stream_status[i] != MH_OK) continue;
        const uint64_t nb = p.b.nbits[i];
        uint64_t r = 0, r1 = 0;
        if (EMIT) {
            r = p.hit_off[i]; r1 = p.hit_off[i + 1];
            if (r1 == r || r >= p.hit_cap) continue;
        } else if (nb > p.b.walk_max_bits) {
            stream_fail(p.b, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
            continue;
        }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0);
        dec.stream(p, i);
        uint32_t ctx = p.b.prev0, used = 0;
        bool bad = false;
        uint64_t D = 0, k = 0, cnt = 0;
        // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
        while (used < nb && !bad && (!EMIT || r < r1)) {
            const uint32_t sym = dec.next(p, src, bc, ctx, used, bad);
            D = ((D << 1) | F) & M(sym);
            ++k;
            if (EMIT) {
                for (uint64_t h = D & L; h && r < r1; h &= h - 1ull, ++r)
                    if (r < p.hit_cap) put_hit(p, r, i, k, uint32_t(__builtin_ctzll(h)));
            } else {
                cnt += uint64_t(__popcll(D & L));
            }
        }
        if (EMIT) continue;
        if (bad || used != nb) { stream_fail(p.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        p.hit_off[i] = cnt;                                       // src/coding.cpp:158: the stream ends exactly at nbits
    }
}

__global__ void find_cap_kernel(FindParams p, int *status, const int *stop) {
    if (stopped(stop)) return;
    if (p.hits && p.hit_off[p.b.n] > p.hit_cap) fail(status, mhk::MHK_STATUS_CAPACITY);
}

template <Model K, bool MLDS>
hipError_t launch(const FindParams &p, const Automaton &a, size_t lds_tables, void *d_ws, hipStream_t st) {
    constexpr int NT = Dec<K>::NT, PER_CU = Dec<K>::PER_CU;
    const size_t lds = lds_tables + (MLDS ? 2048 : 0);
    const uint32_t lds_at = uint32_t(lds_tables);
    if (K == Model::Shared) {
        const int lds_max = 163840;
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(find_idx_count_kernel<K, MLDS>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(find_idx_emit_kernel<K, MLDS>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(find_walk_kernel<K, MLDS, false>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(find_walk_kernel<K, MLDS, true>), lds_max);
        if (attr != hipSuccess) return attr;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.b.n;
    const uint64_t W = p.b.index ? mhb::work_items(n, p.b.sym_total, 1u << p.b.chunk_shift) : 0;
    const FindLayout L = find_layout(n, W);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    uint64_t *ws_mask = reinterpret_cast<uint64_t *>(ws + L.off_mask);
    auto *state = reinterpret_cast<unsigned long long *>(ws + L.off_state);
    auto *own = reinterpret_cast<uint32_t *>(ws + L.off_own);
    auto *tail = reinterpret_cast<uint32_t *>(ws + L.off_tail);
    auto *cnt = reinterpret_cast<unsigned long long *>(ws + L.off_cnt);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e == hipSuccess && W) e = hipMemsetAsync(ws + L.off_state, 0, L.off_cnt - L.off_state, st);   // states, own and tail counts
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(find_check_kernel, grid_threads((n + 1 > 256 ? n + 1 : 256), 256), dim3(256), 0, st, p, a, ws_mask, status, stop);
    if (p.b.index) {
        hipLaunchKernelGGL((find_idx_count_kernel<K, MLDS>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, ws_mask, lds_at, state,
                           own, tail, status, stop);
        hipLaunchKernelGGL(find_comb_kernel, grid_threads(W + 1, 256), dim3(256), 0, st, p, W, own, tail, cnt, stop);
        if ((e = scan_exclusive(cnt, W + 1, sums, stop, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(find_off_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, W, cnt, status, stop);
        if (p.hits)
            hipLaunchKernelGGL((find_idx_emit_kernel<K, MLDS>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, ws_mask, lds_at,
                               state, cnt, stop);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((find_walk_kernel<K, MLDS, false>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, ws_mask, lds_at, status, stop);
    if ((e = scan_exclusive(p.hit_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(find_cap_kernel, dim3(1), dim3(1), 0, st, p, status, stop);
    if (p.hits)
        hipLaunchKernelGGL((find_walk_kernel<K, MLDS, true>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, ws_mask, lds_at, status, stop);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_find(const FindParams &p, const Automaton &a, Model model, void *d_ws, hipStream_t st) {
    // tables in L2: the masks alone in LDS, at offset 0
    if (model == Model::Set) return launch<Model::Set, true>(p, a, 0, d_ws, st);
    if (model == Model::Shared2) return launch<Model::Shared2, true>(p, a, 0, d_ws, st);
    // the tables as launch_decode places them; the masks behind them when 2 KiB are left of the 160 KiB
    const size_t lds = mhb::tables_lds(p.b);
    if (lds > 163840) return hipErrorInvalidValue;
    return lds + 2048 <= 163840 ? launch<Model::Shared, true>(p, a, lds, d_ws, st) : launch<Model::Shared, false>(p, a, lds, d_ws, st);
}

}  // namespace mhf
