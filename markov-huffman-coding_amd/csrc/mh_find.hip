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
// The same family serves two matchers, a second policy beside Dec<K>: ShiftAnd (the above) and Dfa, the dictionary search
// (include/mh.h, "DICTIONARY SEARCH IN BATCHES"; mh_dict.h): a lane's state is the 16-bit transition it took last, the
// kept state of a chunk the DFA state, and a tail goes on while the state is deeper than the symbols behind the seam.
// The class map and the first rows of the transition table sit in LDS behind the tables, the other rows come from L2.
#include "mh_find.h"
#include "mh_symdec_dev.hpp"
#include "../../include/mh.h"

#include <algorithm>

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

// ---- the matcher of a lane, one policy per automaton.  State: what a lane carries from symbol to symbol.
//   root / resume / keep    the state at a stream's start, from and into a chunk's state slot (keep: after flush)
//   step, flush             one symbol of a counting pass: the hits that end at it are added to cnt, at the latest by flush
//   alive                   after flush: may a hit that began here still end in the next chunk
//   tail                    symbol t = 1, 2, .. behind the seam, no new starts: the hits that began in front of it; false when
//                           nothing that began there is alive any more
//   emit, emit_flush        one symbol of an emit pass, `end` symbols of the stream read: records r .. r1 - 1 in
//                           (end, pattern) order, those below hit_cap written
template <bool MLDS> struct ShiftAnd {
    struct Args {
        const uint64_t *ws_mask;
        uint32_t lds_at;
        void bind(const uint64_t *m) { ws_mask = m; }
    };
    using State = uint64_t;
    const FindParams &p;
    const Masks<MLDS> M;
    const uint64_t F, L;
    __device__ __forceinline__ ShiftAnd(const FindParams &p, const Args &a, unsigned char *smem)
        : p(p), M(a.ws_mask, smem, a.lds_at), F(p.first), L(p.last) {}
    __device__ __forceinline__ State root() const { return 0; }
    __device__ __forceinline__ State resume(unsigned long long kept) const { return kept; }
    __device__ __forceinline__ unsigned long long keep(State D) const { return D; }
    template <typename C> __device__ __forceinline__ void step(State &D, uint32_t sym, C &cnt) const {
        D = ((D << 1) | F) & M(sym);
        cnt += C(__popcll(D & L));
    }
    template <typename C> __device__ __forceinline__ void flush(State &, C &) const {}
    __device__ __forceinline__ bool alive(State D) const { return D != 0; }
    __device__ __forceinline__ uint32_t tail_max() const { return p.max_len - 1u; }
    // (the bit that leaves one pattern's top must not start the next)
    __device__ __forceinline__ bool tail(State &D, uint32_t sym, uint32_t, uint32_t &tc) const {
        D = (D << 1) & ~F & M(sym);
        tc += uint32_t(__popcll(D & L));
        return D != 0;
    }
    __device__ __forceinline__ void emit(State &D, uint32_t sym, uint64_t i, uint64_t end, uint64_t &r, uint64_t r1) const {
        D = ((D << 1) | F) & M(sym);
        for (uint64_t h = D & L; h && r < r1; h &= h - 1ull, ++r)
            if (r < p.hit_cap) put_hit(p, r, i, end, uint32_t(__builtin_ctzll(h)));
    }
    __device__ __forceinline__ void emit_flush(State &, uint64_t, uint64_t, uint64_t &, uint64_t) const {}
};

// The DFA of a dictionary.  A lane's state is the transition it took last (target | 0x8000: the target's outputs are still to
// be taken): step() takes the outputs of the transition loaded one symbol ago and issues the next load, so that load is in
// flight while the decoder works on the next symbol and never sits on its context -> table -> next-context chain.
// LDS at lds_at: the class map (256 bytes) and rows 0 .. R-1 of the transition table; CLDS false (no 256 bytes left beside
// the tables): everything from L2.
template <bool CLDS> struct Dfa {
    struct Args {
        mhd::DictDev d;
        uint32_t lds_at, hot_rows;
        void bind(const uint64_t *) {}                            // (no masks)
    };
    using State = uint32_t;
    const FindParams &p;
    const mhd::DictDev &d;
    const uint8_t *cls;
    const uint16_t *hot;
    const uint32_t R, ncls;
    __device__ __forceinline__ Dfa(const FindParams &p, const Args &a, unsigned char *smem)
        : p(p), d(a.d), cls(CLDS ? smem + a.lds_at : a.d.cls), hot(reinterpret_cast<const uint16_t *>(smem + a.lds_at + 256u)),
          R(CLDS ? a.hot_rows : 0u), ncls(a.d.ncls) {
        if (CLDS) {
            // (the image's parts are padded to 16 bytes: the last uint4 of the rows stays inside the transition table's part)
            uint4 *l = reinterpret_cast<uint4 *>(smem + a.lds_at);
            const uint32_t n16 = 16u + (R * ncls * 2u + 15u) / 16u;
            for (uint32_t k = threadIdx.x; k < n16; k += blockDim.x)
                l[k] = k < 16u ? reinterpret_cast<const uint4 *>(a.d.cls)[k] : reinterpret_cast<const uint4 *>(a.d.trans)[k - 16u];
            __syncthreads();
        }
    }
    __device__ __forceinline__ State root() const { return 0; }
    __device__ __forceinline__ State resume(unsigned long long kept) const { return uint32_t(kept) & 0x7FFFu; }
    __device__ __forceinline__ unsigned long long keep(State S) const { return S; }
    // a select between two loads: the row from LDS or from L2
    __device__ __forceinline__ uint32_t load(uint32_t s, uint32_t sym) const {
        const uint32_t at = s * ncls + cls[sym & 255u];
        return s < R ? hot[at] : d.trans[at];
    }
    template <typename C> __device__ __forceinline__ void step(State &S, uint32_t sym, C &cnt) const {
        const uint32_t s = S & 0x7FFFu;
        if (S & 0x8000u) cnt += C(d.out_off[s + 1] - d.out_off[s]);
        S = load(s, sym);
    }
    template <typename C> __device__ __forceinline__ void flush(State &S, C &cnt) const {
        const uint32_t s = S & 0x7FFFu;
        if (S & 0x8000u) cnt += C(d.out_off[s + 1] - d.out_off[s]);
        S = s;
    }
    __device__ __forceinline__ bool alive(State S) const { return d.depth[S] != 0; }
    __device__ __forceinline__ uint32_t tail_max() const { return d.max_len - 1u; }
    // t symbols behind the seam a state of depth <= t holds nothing from in front of it, and of a deeper state's outputs only
    // those longer than t began there (the shorter ones belong to the next chunk's own lane)
    __device__ __forceinline__ bool tail(State &S, uint32_t sym, uint32_t t, uint32_t &tc) const {
        const uint32_t tr = load(S, sym), s = tr & 0x7FFFu;
        S = s;
        if (d.depth[s] <= t) return false;
        if (tr & 0x8000u)
            for (uint32_t q = d.out_off[s], q1 = d.out_off[s + 1]; q < q1; ++q) tc += d.out_len[q] > t ? 1u : 0u;
        return true;
    }
    // the outputs of the transition taken last, which ended at symbol `end`: list order is pattern order
    __device__ __forceinline__ void put(State S, uint64_t i, uint64_t end, uint64_t &r, uint64_t r1) const {
        if (!(S & 0x8000u)) return;
        const uint32_t s = S & 0x7FFFu;
        for (uint32_t q = d.out_off[s], q1 = d.out_off[s + 1]; q < q1 && r < r1; ++q, ++r) {
            if (r >= p.hit_cap) continue;
            p.hits[3 * r] = i;
            p.hits[3 * r + 1] = end - d.out_len[q];
            p.hits[3 * r + 2] = end;
            if (p.hit_pattern) p.hit_pattern[r] = d.out_pat[q];
        }
    }
    __device__ __forceinline__ void emit(State &S, uint32_t sym, uint64_t i, uint64_t end, uint64_t &r, uint64_t r1) const {
        put(S, i, end - 1u, r, r1);
        S = load(S & 0x7FFFu, sym);
    }
    __device__ __forceinline__ void emit_flush(State &S, uint64_t i, uint64_t end, uint64_t &r, uint64_t r1) const {
        put(S, i, end, r, r1);
        S &= 0x7FFFu;
    }
};

__global__ __launch_bounds__(256) void find_check_kernel(FindParams p, Automaton a, uint64_t *ws_mask, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i < 256u) ws_mask[i] = a.mask[i];
    if (i > p.b.n) return;
    p.hit_off[i] = 0;
    check_batch(p.b, i, status, stop);
}

template <Model K, class MT>
__global__ __launch_bounds__(Dec<K>::NT) void find_idx_count_kernel(FindParams p, uint64_t nwork, typename MT::Args ma, unsigned long long *state,
                                                                    uint32_t *own, uint32_t *tail, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    const MT M(p, ma, smem);
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
        typename MT::State D = M.root();
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {
            const uint32_t sym = dec.next(p, src, bc, ctx, used, bad);
            M.step(D, sym, cnt);
        }
        if (bad || used != c.end - c.start) { stream_fail(p.b, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        M.flush(D, cnt);
        own[w] = cnt;
        state[w] = M.keep(D);
        if (c.last || !M.alive(D)) continue;
        // the tail: what began in this chunk and still completes in the next one.  No new starts, no verdict: the next chunk's
        // own lane judges that chunk.  The symbols behind the seam are decoded as that lane and the emit pass decode them: from
        // the next entry's context field (the cursor stands on its position: used == end - start), not from this lane's
        // running context.  The two differ only under an index whose context field is wrong, and then the count must be that
        // of the bytes the decoders return.
        ctx = uint32_t(p.b.index[w + 1] >> (Dec<K>::O2 ? 48 : 56));
        const uint64_t rest = c.ni - c.first - c.nsym;
        const uint32_t lim = uint32_t(rest < M.tail_max() ? rest : M.tail_max());
        uint32_t tc = 0;
        bool live = true;
        for (uint32_t t = 1; t <= lim && live; ++t) {
            const uint32_t sym = dec.next(p, src, bc, ctx, used, bad);
            if (bad) break;
            live = M.tail(D, sym, t, tc);
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

template <Model K, class MT>
__global__ __launch_bounds__(Dec<K>::NT) void find_idx_emit_kernel(FindParams p, uint64_t nwork, typename MT::Args ma,
                                                                   const unsigned long long *state, const unsigned long long *cnt,
                                                                   const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    const MT M(p, ma, smem);
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
        typename MT::State D = c.first ? M.resume(state[w - 1]) : M.root();
        uint64_t r = r0;
        uint32_t t = 0;
        for (; t < c.nsym && r < r1 && !bad; ++t) {
            const uint32_t sym = dec.next(p, src, bc, ctx, used, bad);
            M.emit(D, sym, c.i, c.first + t + 1u, r, r1);
        }
        if (!bad) M.emit_flush(D, c.i, c.first + t, r, r1);
    }
}

// EMIT = false: the stream's verdict and its hit count into hit_off[i] (scanned next); true: its records from hit_off[i]
template <Model K, class MT, bool EMIT>
__global__ __launch_bounds__(Dec<K>::NT) void find_walk_kernel(FindParams p, typename MT::Args ma, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Dec<K> dec(p, smem);
    const MT M(p, ma, smem);
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
        typename MT::State D = M.root();
        uint64_t k = 0, cnt = 0;
        // every code has at least one bit: at most nb steps (src/coding.cpp:124 — decode while bits remain)
        while (used < nb && !bad && (!EMIT || r < r1)) {
            const uint32_t sym = dec.next(p, src, bc, ctx, used, bad);
            if (EMIT) M.emit(D, sym, i, k + 1u, r, r1);
            else M.step(D, sym, cnt);
            ++k;
        }
        if (EMIT) {
            if (!bad) M.emit_flush(D, i, k, r, r1);
            continue;
        }
        if (bad || used != nb) { stream_fail(p.b, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        M.flush(D, cnt);
        p.hit_off[i] = cnt;                                       // src/coding.cpp:158: the stream ends exactly at nbits
    }
}

__global__ void find_cap_kernel(FindParams p, int *status, const int *stop) {
    if (stopped(stop)) return;
    if (p.hits && p.hit_off[p.b.n] > p.hit_cap) fail(status, mhk::MHK_STATUS_CAPACITY);
}

// lds: the tables and, behind them at ma.lds_at, what the matcher keeps there
template <Model K, class MT>
hipError_t launch(const FindParams &p, const Automaton &a, typename MT::Args ma, size_t lds, void *d_ws, hipStream_t st) {
    constexpr int NT = Dec<K>::NT, PER_CU = Dec<K>::PER_CU;
    if (K == Model::Shared) {
        const int lds_max = 163840;
        hipError_t attr = mhk::allow_lds(reinterpret_cast<const void *>(find_idx_count_kernel<K, MT>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(find_idx_emit_kernel<K, MT>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(find_walk_kernel<K, MT, false>), lds_max);
        if (attr == hipSuccess) attr = mhk::allow_lds(reinterpret_cast<const void *>(find_walk_kernel<K, MT, true>), lds_max);
        if (attr != hipSuccess) return attr;
    }
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.b.n;
    const uint64_t W = p.b.index ? mhb::work_items(n, p.b.sym_total, 1u << p.b.chunk_shift) : 0;
    const FindLayout L = find_layout(n, W);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    uint64_t *ws_mask = reinterpret_cast<uint64_t *>(ws + L.off_mask);
    ma.bind(ws_mask);
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
        hipLaunchKernelGGL((find_idx_count_kernel<K, MT>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, ma, state, own, tail, status,
                           stop);
        hipLaunchKernelGGL(find_comb_kernel, grid_threads(W + 1, 256), dim3(256), 0, st, p, W, own, tail, cnt, stop);
        if ((e = scan_exclusive(cnt, W + 1, sums, stop, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(find_off_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, W, cnt, status, stop);
        if (p.hits)
            hipLaunchKernelGGL((find_idx_emit_kernel<K, MT>), dim3(grid_for(W, NT, PER_CU)), dim3(NT), lds, st, p, W, ma, state, cnt, stop);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((find_walk_kernel<K, MT, false>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, ma, status, stop);
    if ((e = scan_exclusive(p.hit_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(find_cap_kernel, dim3(1), dim3(1), 0, st, p, status, stop);
    if (p.hits)
        hipLaunchKernelGGL((find_walk_kernel<K, MT, true>), dim3(grid_for(n + 1, NT, PER_CU)), dim3(NT), lds, st, p, ma, status, stop);
    return hipGetLastError();
}

// the Shift-And search: the masks (2 KiB) at lds_tables
template <Model K, bool MLDS>
hipError_t launch_masks(const FindParams &p, const Automaton &a, size_t lds_tables, void *d_ws, hipStream_t st) {
    return launch<K, ShiftAnd<MLDS>>(p, a, {nullptr, uint32_t(lds_tables)}, lds_tables + (MLDS ? 2048 : 0), d_ws, st);
}

// The dictionary search: the class map and as many transition rows as `room` bytes hold at lds_tables.  (The check kernel is
// the Shift-And search's as it is: its masks go to the workspace and nobody reads them.)
template <Model K>
hipError_t launch_dict(const FindParams &p, const mhd::DictDev &d, size_t lds_tables, size_t room, void *d_ws, hipStream_t st) {
    static const Automaton none{};
    if (room < 256) return launch<K, Dfa<false>>(p, none, {d, uint32_t(lds_tables), 0u}, lds_tables, d_ws, st);
    const size_t row = size_t(d.ncls) * 2;
#ifdef MH_EXP_DICT_NO_HOT_ROWS                                     // (csrc/Makefile, `exp`: the A/B of tools/dict_rate.py)
    const size_t rows = 0;
#else
    const size_t rows = std::min<size_t>(d.states, (room - 256) / row);
#endif
    const size_t lds = lds_tables + 256 + ((rows * row + 15) & ~size_t(15));
    return launch<K, Dfa<true>>(p, none, {d, uint32_t(lds_tables), uint32_t(rows)}, lds, d_ws, st);
}

}  // namespace

hipError_t launch_find(const FindParams &p, const Automaton &a, Model model, void *d_ws, hipStream_t st) {
    // tables in L2: the masks alone in LDS, at offset 0
    if (model == Model::Set) return launch_masks<Model::Set, true>(p, a, 0, d_ws, st);
    if (model == Model::Shared2) return launch_masks<Model::Shared2, true>(p, a, 0, d_ws, st);
    // the tables as launch_decode places them; the masks behind them when 2 KiB are left of the 160 KiB
    const size_t lds = mhb::tables_lds(p.b);
    if (lds > 163840) return hipErrorInvalidValue;
    return lds + 2048 <= 163840 ? launch_masks<Model::Shared, true>(p, a, lds, d_ws, st) : launch_masks<Model::Shared, false>(p, a, lds, d_ws, st);
}

hipError_t launch_find_dict(const FindParams &p, const mhd::DictDev &d, Model model, void *d_ws, hipStream_t st) {
    // tables in L2: the LDS that keeps PER_CU workgroups resident
    if (model == Model::Set) return launch_dict<Model::Set>(p, d, 0, 163840 / Dec<Model::Set>::PER_CU, d_ws, st);
    if (model == Model::Shared2) return launch_dict<Model::Shared2>(p, d, 0, 163840 / Dec<Model::Shared2>::PER_CU, d_ws, st);
    // what the tables leave of the 160 KiB
    const size_t lds = mhb::tables_lds(p.b);
    if (lds > 163840) return hipErrorInvalidValue;
    return launch_dict<Model::Shared>(p, d, lds, 163840 - lds, d_ws, st);
}

}  // namespace mhf
