// mh_find_o2.hip — pattern search in batches of ORDER-2 streams without writing the decoded bytes (include/mh.h, "ORDER 2 IN
// SEARCH AND RE-CODING").  The passes are those of mh_find.hip (check, count, combine, scan, offsets, emit; index-free: count,
// scan, cap, emit) with a third decoder: the model's order-2 tables read from L2 as batch2_dec_idx_kernel reads them, the
// rolling context ctx = ((ctx << 8) | sym) & 0xFFFF, entries masked with IDX2_POS and their context taken from e >> 48.
// Workgroups of 256 lanes, eight per CU, no tables in LDS; the matcher's 2 KiB of masks are in LDS.  The matcher, the record
// order and the seam rule (a chunk that is not its stream's last has >= 256 > 63 symbols) are mh_find.hip's, kept as copies so
// that the order-0/1 kernels stay the same code.  Verdicts are mh_dev_decode_batch_o2's: same checks, same statuses.  Every
// loop is bounded by a symbol count or nbits_i.
#include "mh_find_o2.h"
#include "mh_batch_dev.hpp"
#include "../../include/mh.h"

namespace mhf {

using mhb::BATCH_STATUS_ARG;
using mhk::BitCursor;
using mhk::BitSrc;
using mhk::DecTables;

namespace {

using mhb::fail;
using mhb::find_stream;
using mhb::grid_for;
using mhb::scan_exclusive;
using mhb::stopped;

constexpr int NT2 = 256;                           // batch2_dec_idx_kernel's shape
constexpr int PER_CU2 = 8;

__device__ __forceinline__ uint64_t gtid() { return uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; }
inline dim3 grid_threads(uint64_t items, uint32_t per_block) { return dim3(uint32_t((items + per_block - 1) / per_block)); }

// the model's order-2 tables as decode2_kernel reads them: general form, every level gathered from L2
struct Dec2 {
    const uint16_t *prim;
    const uint32_t *sec_base;
    DecTables tabs;
    __device__ __forceinline__ explicit Dec2(const mhb::DecBatchParams &b) : prim(b.prim), sec_base(b.sec_base), tabs{b.sec, b.tree, b.P, 0u, 0u} {}
    // decodes one symbol in context ctx and rolls the context on
    __device__ __forceinline__ uint32_t next(const BitSrc &src, BitCursor &bc, uint32_t &ctx, uint32_t &used, bool &bad) const {
        const uint32_t sym = mhk::decode_one(prim, sec_base, tabs, src, bc, ctx, used, bad);
        ctx = ((ctx << 8) | sym) & 0xFFFFu;
        return sym;
    }
};

// mask[c] from LDS: one ds_read_b64
struct Masks {
    const uint64_t *l;
    __device__ __forceinline__ Masks(const uint64_t *ws_mask, unsigned char *smem) : l(reinterpret_cast<const uint64_t *>(smem)) {
        uint64_t *d = reinterpret_cast<uint64_t *>(smem);
        for (uint32_t k = threadIdx.x; k < 256u; k += blockDim.x) d[k] = ws_mask[k];
        __syncthreads();
    }
    __device__ __forceinline__ uint64_t operator()(uint32_t c) const { return l[c]; }
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

__device__ __forceinline__ void stream_fail(const FindParams &p, int *status, uint64_t i, int mh_code, int dev_code) {
    p.b.stream_status[i] = mh_code;
    fail(status, dev_code);
}

__global__ __launch_bounds__(256) void find2_check_kernel(FindParams p, Automaton a, uint64_t *ws_mask, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i < 256u) ws_mask[i] = a.mask[i];
    if (i > p.b.n) return;
    p.hit_off[i] = 0;
    bool bad = (i == 0 && p.b.pay_off[0] != 0) || (i == p.b.n && p.b.pay_off[p.b.n] != p.b.pay_total) || (i < p.b.n && p.b.pay_off[i + 1] < p.b.pay_off[i]);
    if (p.b.index)
        bad |= (i == 0 && p.b.sym_off[0] != 0) || (i == p.b.n && p.b.sym_off[p.b.n] != p.b.sym_total) || (i < p.b.n && p.b.sym_off[i + 1] < p.b.sym_off[i]);
    if (bad) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
    if (i == p.b.n) return;
    p.b.stream_status[i] = MH_OK;
    if (!bad && p.b.nbits[i] > (p.b.pay_off[i + 1] - p.b.pay_off[i]) * 8u) stream_fail(p, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
}

// chunk w of the indexed batch: its stream, symbols, bit span and entry context; false when w is a gap
struct Chunk {
    uint64_t i, ni, first, nb, start, end;
    uint32_t nsym, ctx;
    bool last;
};
__device__ __forceinline__ bool chunk_of(const FindParams &p, uint64_t w, Chunk &c) {
    const uint32_t cs = p.b.chunk_shift;
    c.i = find_stream(p.b.sym_off, p.b.n, cs, w);
    if (c.i >= p.b.n) return false;
    const uint64_t a = p.b.sym_off[c.i];
    c.ni = p.b.sym_off[c.i + 1] - a;
    c.first = (w - ((a >> cs) + c.i)) << cs;
    if (c.first >= c.ni) return false;
    c.nb = p.b.nbits[c.i];
    const uint64_t e = p.b.index[w];
    c.start = e & mhk::IDX2_POS;
    c.ctx = uint32_t(e >> 48);
    c.last = c.first + (uint64_t(1) << cs) >= c.ni;
    c.end = c.last ? c.nb : (p.b.index[w + 1] & mhk::IDX2_POS);
    c.nsym = uint32_t(c.last ? c.ni - c.first : (uint64_t(1) << cs));
    return true;
}

__global__ __launch_bounds__(NT2) void find2_idx_count_kernel(FindParams p, uint64_t nwork, const uint64_t *ws_mask, unsigned long long *state,
                                                              uint32_t *own, uint32_t *tail, int *status, const int *stop) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2048];
    if (stopped(stop)) return;
    const Dec2 dec(p.b);
    const Masks M(ws_mask, smem);
    const uint64_t F = p.first, L = p.last;
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        Chunk c;
        if (!chunk_of(p, w, c) || p.b.stream_status[c.i] == MH_ERR_ARG) continue;
        if (c.start > c.end || c.end > c.nb) { stream_fail(p, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        uint32_t ctx = c.ctx, used = 0, cnt = 0;
        bool bad = false;
        uint64_t D = 0;
        for (uint32_t t = 0; t < c.nsym && !bad; ++t) {
            const uint32_t sym = dec.next(src, bc, ctx, used, bad);
            D = ((D << 1) | F) & M(sym);
            cnt += uint32_t(__popcll(D & L));
        }
        if (bad || used != c.end - c.start) { stream_fail(p, status, c.i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        own[w] = cnt;
        state[w] = D;
        if (c.last || !D) continue;
        // the tail: what began in this chunk and still completes in the next one.  No new starts, no verdict: the next
        // chunk's own lane judges that chunk.
        const uint64_t rest = c.ni - c.first - c.nsym;
        const uint32_t lim = uint32_t(rest < p.max_len - 1u ? rest : p.max_len - 1u);
        uint32_t tc = 0;
        for (uint32_t t = 0; t < lim && D; ++t) {
            const uint32_t sym = dec.next(src, bc, ctx, used, bad);
            if (bad) break;
            D = (D << 1) & ~F & M(sym);
            tc += uint32_t(__popcll(D & L));
        }
        tail[w] = tc;
    }
}

__global__ __launch_bounds__(256) void find2_comb_kernel(FindParams p, uint64_t nwork, const uint32_t *own, const uint32_t *tail,
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

__global__ __launch_bounds__(256) void find2_off_kernel(FindParams p, uint64_t nwork, const unsigned long long *cnt, int *status, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t i = gtid();
    if (i > p.b.n) return;
    const unsigned long long v = i < p.b.n ? cnt[(p.b.sym_off[i] >> p.b.chunk_shift) + i] : cnt[nwork];
    p.hit_off[i] = v;
    if (i == p.b.n && p.hits && v > p.hit_cap) fail(status, mhk::MHK_STATUS_CAPACITY);
}

__global__ __launch_bounds__(NT2) void find2_idx_emit_kernel(FindParams p, uint64_t nwork, const uint64_t *ws_mask, const unsigned long long *state,
                                                             const unsigned long long *cnt, const int *stop) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2048];
    if (stopped(stop)) return;
    const Dec2 dec(p.b);
    const Masks M(ws_mask, smem);
    const uint64_t F = p.first, L = p.last;
    for (uint64_t w = gtid(); w < nwork; w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t r0 = cnt[w], r1 = cnt[w + 1];
        if (r1 == r0 || r0 >= p.hit_cap) continue;                // (a chunk with hits belongs to a stream that passed)
        Chunk c;
        if (!chunk_of(p, w, c)) continue;
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[c.i], c.nb, bit0);
        BitCursor bc;
        bc.init(src, bit0 + c.start);
        uint32_t ctx = c.ctx, used = 0;
        bool bad = false;
        uint64_t D = c.first ? state[w - 1] : 0ull, r = r0;
        for (uint32_t t = 0; t < c.nsym && r < r1 && !bad; ++t) {
            const uint32_t sym = dec.next(src, bc, ctx, used, bad);
            D = ((D << 1) | F) & M(sym);
            for (uint64_t h = D & L; h && r < r1; h &= h - 1ull, ++r)
                if (r < p.hit_cap) put_hit(p, r, c.i, c.first + t + 1u, uint32_t(__builtin_ctzll(h)));
        }
    }
}

// EMIT = false: the stream's verdict and its hit count into hit_off[i] (scanned next); true: its records from hit_off[i]
template <bool EMIT>
__global__ __launch_bounds__(NT2) void find2_walk_kernel(FindParams p, const uint64_t *ws_mask, int *status, const int *stop) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2048];
    if (stopped(stop)) return;
    const Dec2 dec(p.b);
    const Masks M(ws_mask, smem);
    const uint64_t F = p.first, L = p.last;
    for (uint64_t i = gtid(); i < p.b.n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (p.b.stream_status[i] != MH_OK) continue;
        const uint64_t nb = p.b.nbits[i];
        uint64_t r = 0, r1 = 0;
        if (EMIT) {
            r = p.hit_off[i]; r1 = p.hit_off[i + 1];
            if (r1 == r || r >= p.hit_cap) continue;
        } else if (nb > p.b.walk_max_bits) {
            stream_fail(p, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
            continue;
        }
        uint64_t bit0;
        const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[i], nb, bit0);
        BitCursor bc;
        bc.init(src, bit0);
        uint32_t ctx = p.b.prev0, used = 0;                       // (prev0, prev0)
        bool bad = false;
        uint64_t D = 0, k = 0, cnt = 0;
        // every code has at least one bit: at most nb steps
        while (used < nb && !bad && (!EMIT || r < r1)) {
            const uint32_t sym = dec.next(src, bc, ctx, used, bad);
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
        if (bad || used != nb) { stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT); continue; }
        p.hit_off[i] = cnt;                                       // the stream ends exactly at nbits
    }
}

__global__ void find2_cap_kernel(FindParams p, int *status, const int *stop) {
    if (stopped(stop)) return;
    if (p.hits && p.hit_off[p.b.n] > p.hit_cap) fail(status, mhk::MHK_STATUS_CAPACITY);
}

}  // namespace

hipError_t launch_find_o2(const FindParams &p, const Automaton &a, void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint64_t n = p.b.n;
    const uint64_t W = p.b.index ? p.b.sym_total / (uint64_t(1) << p.b.chunk_shift) + n + 1 : 0;
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
    hipLaunchKernelGGL(find2_check_kernel, grid_threads((n + 1 > 256 ? n + 1 : 256), 256), dim3(256), 0, st, p, a, ws_mask, status, stop);
    if (p.b.index) {
        const dim3 grid(grid_for(W, NT2, PER_CU2));
        hipLaunchKernelGGL(find2_idx_count_kernel, grid, dim3(NT2), 0, st, p, W, ws_mask, state, own, tail, status, stop);
        hipLaunchKernelGGL(find2_comb_kernel, grid_threads(W + 1, 256), dim3(256), 0, st, p, W, own, tail, cnt, stop);
        if ((e = scan_exclusive(cnt, W + 1, sums, stop, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(find2_off_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, p, W, cnt, status, stop);
        if (p.hits) hipLaunchKernelGGL(find2_idx_emit_kernel, grid, dim3(NT2), 0, st, p, W, ws_mask, state, cnt, stop);
        return hipGetLastError();
    }
    const dim3 grid(grid_for(n + 1, NT2, PER_CU2));
    hipLaunchKernelGGL(find2_walk_kernel<false>, grid, dim3(NT2), 0, st, p, ws_mask, status, stop);
    if ((e = scan_exclusive(p.hit_off, n + 1, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(find2_cap_kernel, dim3(1), dim3(1), 0, st, p, status, stop);
    if (p.hits) hipLaunchKernelGGL(find2_walk_kernel<true>, grid, dim3(NT2), 0, st, p, ws_mask, status, stop);
    return hipGetLastError();
}

}  // namespace mhf
