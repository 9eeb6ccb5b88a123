// mh_bank.hip — banks of K shared order-0/1 models, each stream coded under the one that suits it best (include/mh.h, "BANKS OF
// SHARED MODELS").  Layouts: mh_bank.h; the bank is a model set (mh_each.h); units, scans and loads: mh_batch_dev.hpp.
//   bank_check_kernel       offsets non-decreasing, [0] == 0, [n] == total
//   bank_image_kernel       one thread per (entry, context, symbol): the entry's dense 64 KiB length image (0 = no code; an
//                           order-0 entry is replicated over the 256 contexts, so the hot loop has no branch on the order)
//   bank_select_kernel      one wave per (batch unit, group of G entries), G images in LDS: per entry the unit's code-length
//                           sum (one wave reduction, one 64-bit atomic) and, for a symbol without a code, one bit of the
//                           stream's uncovered mask; the input is read ceil(K / G) times
//   bank_argmin_kernel      one thread per stream: the covering entry with the fewest bits, ties to the lowest k
//   bank_pick_kernel        one thread per (stream, context): a view's rows from the chosen entries
//   bank_sort_*             stable counting sort of the streams by group (training): counts per block of 1024 streams,
//                           bases per (block, group), ranks inside a block
//   bank_gather_kernel      one workgroup per sorted stream: its bytes into its group's 16-aligned range, its re-based offset
// Every loop is bounded by a symbol count, K, a block of streams or a stream's length.
#include "mh_bank.h"
#include "mh_batch_dev.hpp"
#include "../../include/mh.h"

namespace mhbank {

using mhb::B_SUB;
using mhb::B_THREADS;
using mhb::B_VEC;
using mhb::BATCH_STATUS_ARG;
using mhe::NO_SLOT;
using mhe::SetDev;

namespace {

using mhb::byte_of;
using mhb::fail;
using mhb::find_stream;
using mhb::grid_for;
using mhb::grid_threads;
using mhb::gtid;
using mhb::load16;
using mhb::scan_exclusive;
using mhb::stopped;
using mhb::SUB_SHIFT;

constexpr uint32_t WAVES = B_THREADS / 64;

// a stream's group (the selection never gives MH_BANK_NONE to a stream whose group model was trained on it; clamped all the same,
// the same way by every kernel, so that no index leaves its array)
__device__ __forceinline__ uint32_t group_of(const uint32_t *group, uint64_t i, uint32_t K) { const uint32_t g = group[i]; return g < K ? g : K - 1u; }


__global__ void bank_check_kernel(const uint64_t *off, uint64_t n, uint64_t total, int *status, int *stop) {
    const uint64_t i = gtid();
    if (i > n) return;
    const bool bad = (i == 0 && off[0] != 0) || (i == n && off[n] != total) || (i < n && off[i + 1] < off[i]);
    if (bad) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
}

// grid (256 contexts, K entries) x 256 symbols
__global__ __launch_bounds__(256) void bank_image_kernel(SetDev bank, uint8_t *img, const int *stop) {
    if (stopped(stop)) return;
    const uint32_t k = blockIdx.y, ctx = blockIdx.x, sym = threadIdx.x;
    const uint32_t slot = bank.ctx_slot[size_t(k) * 256u + (bank.type[k] ? ctx : 0u)];
    img[size_t(k) * IMG_BYTES + ctx * 256u + sym] = slot == NO_SLOT ? uint8_t(0) : bank.len8[size_t(slot) * 256u + sym];
}

// grid (workgroups, ceil(K / G)): workgroup group y holds the images of entries [G y, G y + ge) in LDS
__global__ __launch_bounds__(B_THREADS) void bank_select_kernel(const uint8_t *data, const uint64_t *in_off, uint64_t n, uint64_t nunits,
                                                                uint32_t prev0, const uint8_t *img, uint32_t K, unsigned long long *sums,
                                                                unsigned long long *miss, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;                                        // (uniform: before the barrier)
    const uint32_t e0 = blockIdx.y * G;
    const uint32_t ge = K - e0 < G ? K - e0 : G;
    const uint4 *src = reinterpret_cast<const uint4 *>(img + size_t(e0) * IMG_BYTES);
    uint4 *dst = reinterpret_cast<uint4 *>(smem);
    for (uint32_t q = threadIdx.x; q < ge * (IMG_BYTES / 16); q += B_THREADS) dst[q] = src[q];
    __syncthreads();
    const uint64_t nw = uint64_t(gridDim.x) * WAVES;
    for (uint64_t u = uint64_t(blockIdx.x) * WAVES + threadIdx.x / 64; u < nunits; u += nw) {
        const uint64_t i = find_stream(in_off, n, SUB_SHIFT, u);
        if (i >= n) continue;                                         // wave-uniform from here to the atomics
        const uint64_t a = in_off[i], ni = in_off[i + 1] - a;
        const uint64_t s0 = (u - ((a >> SUB_SHIFT) + i)) << SUB_SHIFT;
        if (s0 >= ni) continue;
        const uint64_t j0 = s0 + uint64_t(mhk::lane_id()) * B_VEC;
        const uint32_t cnt = j0 < ni ? uint32_t(ni - j0 < B_VEC ? ni - j0 : B_VEC) : 0u;
        uint32_t x[4] = {0, 0, 0, 0};
        uint32_t prev = prev0;
        if (cnt) {
            load16(data + a + j0, cnt, x);
            if (j0) prev = data[a + j0 - 1];
        }
        uint32_t bits[G], missing[G];
#pragma unroll
        for (uint32_t e = 0; e < G; ++e) { bits[e] = 0; missing[e] = 0; }
#pragma unroll
        for (uint32_t t = 0; t < B_VEC; ++t) {
            const uint32_t sym = byte_of(x, t);
            if (t < cnt) {
                const uint32_t at = (prev << 8) | sym;
#pragma unroll
                for (uint32_t e = 0; e < G; ++e) {
                    const uint32_t len = smem[e * IMG_BYTES + at];     // (an entry beyond ge reads the other image: not used)
                    bits[e] += len;
                    missing[e] |= len == 0u;
                }
            }
            prev = sym;
        }
#pragma unroll
        for (uint32_t e = 0; e < G; ++e) {
            if (e >= ge) break;
            const uint32_t b = mhk::wave_sum(bits[e]);                 // <= 64 lanes x 16 symbols x 64 bits
            const bool any = __ballot(missing[e] != 0u) != 0ull;
            if (mhk::lane_id() == 0) {
                if (b) atomicAdd(&sums[i * K + e0 + e], (unsigned long long)b);
                if (any) atomicOr(&miss[i], 1ull << (e0 + e));
            }
        }
    }
}

__global__ void bank_argmin_kernel(const unsigned long long *sums, const unsigned long long *miss, uint64_t n, uint32_t K, uint32_t *choice,
                                   unsigned long long *nbits, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t i = gtid();
    if (i >= n) return;
    const unsigned long long m = miss[i];
    unsigned long long best = ~0ull;
    uint32_t c = NONE;
    for (uint32_t k = 0; k < K; ++k) {
        const unsigned long long v = sums[i * K + k];
        if (!((m >> k) & 1ull) && (c == NONE || v < best)) { best = v; c = k; }
    }
    choice[i] = c;
    if (nbits) nbits[i] = c == NONE ? ~0ull : best;
}

__global__ __launch_bounds__(256) void bank_pick_kernel(SetDev bank, const uint32_t *choice, SetDev view, int *status) {
    const uint64_t t = gtid();
    if (t >= view.n * 256u) return;
    const uint64_t i = t >> 8;
    const uint32_t c = uint32_t(t & 255u), k = choice[i];
    if (k >= bank.n) {
        if (c == 0) fail(status, BATCH_STATUS_ARG);
        return;
    }
    view.ctx_slot[t] = bank.ctx_slot[size_t(k) * 256u + c];
    if (c == 0) { view.type[i] = bank.type[k]; view.maxlen[i] = bank.maxlen[k]; }
}

// ------------------------------------------------------------------------------------------------ training: sort and gather

// per block of SORT_BLOCK streams: counts per group
__global__ __launch_bounds__(256) void bank_sort_count_kernel(const uint32_t *group, uint64_t n, uint32_t K, uint32_t *bcnt, const int *stop) {
    __shared__ uint32_t cnt[BANK_MAX];
    if (stopped(stop)) return;
    if (threadIdx.x < BANK_MAX) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t b0 = uint64_t(blockIdx.x) * SORT_BLOCK;
    for (uint32_t t = threadIdx.x; t < SORT_BLOCK; t += 256)
        if (b0 + t < n) atomicAdd(&cnt[group_of(group, b0 + t, K)], 1u);
    __syncthreads();
    if (threadIdx.x < K) bcnt[size_t(blockIdx.x) * K + threadIdx.x] = cnt[threadIdx.x];
}

// one workgroup of BANK_MAX threads: bcnt becomes the first sorted position of (block, group); summary[c] = start of group c
__global__ __launch_bounds__(BANK_MAX) void bank_sort_base_kernel(uint32_t *bcnt, uint64_t nb, uint32_t K, unsigned long long *summary,
                                                                  const int *stop) {
    __shared__ unsigned long long tot[BANK_MAX + 1];
    if (stopped(stop)) return;
    const uint32_t c = threadIdx.x;
    unsigned long long run = 0;
    if (c < K)
        for (uint64_t b = 0; b < nb; ++b) { const uint32_t v = bcnt[b * K + c]; bcnt[b * K + c] = uint32_t(run); run += v; }
    tot[c] = run;
    __syncthreads();
    if (c == 0) {
        unsigned long long s = 0;
        for (uint32_t g = 0; g < K; ++g) { const unsigned long long v = tot[g]; tot[g] = s; s += v; }
        tot[K] = s;
    }
    __syncthreads();
    if (c < K)
        for (uint64_t b = 0; b < nb; ++b) bcnt[b * K + c] += uint32_t(tot[c]);
    if (c < K) summary[c] = tot[c];
    if (c == 0) summary[K] = tot[K];
}

// stable placement: a stream's rank among the earlier streams of its block in the same group
__global__ __launch_bounds__(SORT_BLOCK) void bank_sort_place_kernel(const uint32_t *group, const uint64_t *in_off, uint64_t n, uint32_t K,
                                                                     const uint32_t *bcnt, uint32_t *perm, unsigned long long *glen,
                                                                     const int *stop) {
    __shared__ uint8_t g[SORT_BLOCK];
    if (stopped(stop)) return;
    const uint64_t i = uint64_t(blockIdx.x) * SORT_BLOCK + threadIdx.x;
    g[threadIdx.x] = i < n ? uint8_t(group_of(group, i, K)) : uint8_t(0);
    __syncthreads();
    if (i == n) glen[n] = 0;
    if (i >= n) return;
    const uint8_t mine = g[threadIdx.x];
    uint32_t rank = 0;
    for (uint32_t t = 0; t < threadIdx.x; ++t) rank += g[t] == mine;
    const uint32_t pos = bcnt[size_t(blockIdx.x) * K + mine] + rank;
    perm[pos] = uint32_t(i);
    glen[pos] = in_off[i + 1] - in_off[i];
}

// one thread: the 16-aligned byte base of every group in the gathered buffer (summary[K + 1 + c]) and its bytes (summary[2 (K + 1) + c])
__global__ void bank_group_base_kernel(const unsigned long long *goff, uint32_t K, unsigned long long *summary, const int *stop) {
    if (stopped(stop)) return;
    unsigned long long base = 0;
    for (uint32_t c = 0; c <= K; ++c) {
        summary[K + 1 + c] = base;
        const unsigned long long bytes = c < K ? goff[summary[c + 1]] - goff[summary[c]] : 0ull;
        summary[2 * (K + 1) + c] = bytes;
        base = (base + bytes + 15ull) & ~15ull;
    }
}

__global__ __launch_bounds__(256) void bank_gather_kernel(const uint8_t *data, const uint64_t *in_off, uint64_t n, const uint32_t *group,
                                                          uint32_t K, const uint32_t *perm, const unsigned long long *goff,
                                                          const unsigned long long *summary, uint8_t *gdata, unsigned long long *coff,
                                                          const int *stop) {
    if (stopped(stop)) return;
    for (uint64_t p = blockIdx.x; p < n; p += gridDim.x) {
        const uint32_t i = perm[p], c = group_of(group, i, K);
        const unsigned long long start = summary[c], end = summary[c + 1];
        const unsigned long long rel = goff[p] - goff[start];
        const uint64_t a = in_off[i], len = in_off[i + 1] - a;
        uint8_t *dst = gdata + summary[K + 1 + c] + rel;
        for (uint64_t j = threadIdx.x; j < len; j += 256) dst[j] = data[a + j];
        if (threadIdx.x == 0) {
            coff[p + c] = rel;
            if (p + 1 == end) coff[p + 1 + c] = goff[p + 1] - goff[start];
        }
    }
}

__global__ void bank_changed_kernel(const uint32_t *old_c, const uint32_t *new_c, const uint32_t *remap, uint64_t n, unsigned long long *changed) {
    const uint64_t i = gtid();
    if (i >= n) return;
    if (new_c[i] != remap[old_c[i] < BANK_MAX ? old_c[i] : 0u]) atomicAdd(changed, 1ull);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ launchers

hipError_t launch_select(const SetDev &bank, const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total, uint32_t prev0,
                         uint32_t *d_choice, unsigned long long *d_nbits, void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const uint32_t K = uint32_t(bank.n);
    const SelLayout L = sel_layout(K, n);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    uint8_t *img = ws + L.off_img;
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    auto *miss = reinterpret_cast<unsigned long long *>(ws + L.off_miss);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e == hipSuccess && n) e = hipMemsetAsync(sums, 0, L.total - L.off_sums, st);     // sums and masks
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bank_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, d_in_off, n, total, status, stop);
    if (!n) return hipGetLastError();
    hipLaunchKernelGGL(bank_image_kernel, dim3(256, K), dim3(256), 0, st, bank, img, stop);
    if (total) {
        const uint64_t U = mhb::units_of(total, n);
        const uint32_t groups = (K + G - 1) / G;
        hipLaunchKernelGGL(bank_select_kernel, dim3(grid_for(U, WAVES, 1), groups), dim3(B_THREADS), G * IMG_BYTES, st, d_data, d_in_off, n, U,
                           prev0, img, K, sums, miss, stop);
    }
    hipLaunchKernelGGL(bank_argmin_kernel, grid_threads(n, 256), dim3(256), 0, st, sums, miss, n, K, d_choice, d_nbits, stop);
    return hipGetLastError();
}

hipError_t launch_check(const uint64_t *d_in_off, uint64_t n, uint64_t total, void *d_ws, hipStream_t st) {
    int *status = static_cast<int *>(d_ws);
    hipError_t e = hipMemsetAsync(status, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bank_check_kernel, grid_threads(n + 1, 256), dim3(256), 0, st, d_in_off, n, total, status, status + 1);
    return hipGetLastError();
}

hipError_t launch_pick(const SetDev &bank, const uint32_t *d_choice, const SetDev &view, int *status, hipStream_t st) {
    hipError_t e = hipMemsetAsync(status, 0, 4, st);
    if (e != hipSuccess) return e;
    if (view.n) hipLaunchKernelGGL(bank_pick_kernel, grid_threads(view.n * 256u, 256), dim3(256), 0, st, bank, d_choice, view, status);
    return hipGetLastError();
}

hipError_t launch_gather(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, const uint32_t *d_group, uint32_t k, const GatherBufs &g,
                         const int *stop, hipStream_t st) {
    const uint64_t nb = (n + SORT_BLOCK - 1) / SORT_BLOCK;
    if (nb) hipLaunchKernelGGL(bank_sort_count_kernel, dim3(uint32_t(nb)), dim3(256), 0, st, d_group, n, k, g.bcnt, stop);
    hipLaunchKernelGGL(bank_sort_base_kernel, dim3(1), dim3(BANK_MAX), 0, st, g.bcnt, nb, k, g.summary, stop);
    hipLaunchKernelGGL(bank_sort_place_kernel, dim3(uint32_t(nb + (n % SORT_BLOCK == 0 ? 1 : 0))), dim3(SORT_BLOCK), 0, st, d_group, d_in_off, n,
                       k, g.bcnt, g.perm, g.goff, stop);
    hipError_t e = scan_exclusive(g.goff, n + 1, g.sums, stop, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bank_group_base_kernel, dim3(1), dim3(1), 0, st, g.goff, k, g.summary, stop);
    if (n) hipLaunchKernelGGL(bank_gather_kernel, dim3(grid_for(n, 1, 16)), dim3(256), 0, st, d_data, d_in_off, n, d_group, k, g.perm, g.goff,
                              g.summary, g.gdata, g.coff, stop);
    return hipGetLastError();
}

hipError_t launch_changed(const uint32_t *d_old, const uint32_t *d_new, const uint32_t *d_remap, uint64_t n, unsigned long long *changed,
                          hipStream_t st) {
    hipError_t e = hipMemsetAsync(changed, 0, 8, st);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(bank_changed_kernel, grid_threads(n, 256), dim3(256), 0, st, d_old, d_new, d_remap, n, changed);
    return hipGetLastError();
}

}  // namespace mhbank
