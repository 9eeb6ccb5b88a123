// mh_select.hip — a new compressed batch from picked streams of up to eight compressed batches, undecoded (include/mh.h,
// "SELECTING RECORDS OF BATCHES").  Every stream of a batch is byte-aligned and self-contained, so a pick's payload is
// copied as it is; its index slice is copied entry for entry as well, but to another place: slice j of the output sits at
// out_sym_off_j / chunk + j, which depends on every symbol count in front of it.
//   select_check_kernel     one thread per offset entry of every source (mhb::offsets_bad, as the batch decoders check) and one
//                           per pick: its payload bytes and symbols into the workspace's `lens`, the addresses of its first
//                           payload byte and index entry into `from` / `ifrom`, out_nbits and the pick's status
//   scan_exclusive          once, over bytes and symbol counts in one array (mh_select.h, SelectLayout)
//   select_finish_kernel    one thread per pick: out_off, out_sym_off and the two capacity verdicts
//   select_gather_kernel    the payloads.  Work is numbered over the OUTPUT: a wave takes one aligned 1 KiB window of the output
//                           bytes of one pick (window numbers of pick j from out_off_j / 1024 + j, found by mhb::find_stream;
//                           GATHER_RUN numbers in a row per wave, one search and then a step each), a lane one aligned 16-byte
//                           word of it.  A word that lies inside the pick is one 16-byte store fed by mhb::load16 from the
//                           unaligned source; a word that the pick shares with its neighbours is written with byte stores,
//                           every byte by the one lane whose pick owns it.  A long stream is spread over the device, six 3-byte
//                           streams in one word are six lanes, and no lane loops over a stream.
//   select_index_kernel     one thread per output entry number under the same numbering over out_sym_off with the chunk
//                           shift: 8 bytes copied, gap entries left alone
//   picks_flag_kernel, scan_exclusive, picks_scatter_kernel     the pick list of a predicate: kept streams ascending, then
//                           MH_SELECT_NONE, and the count
// The grids of the gather and the index kernel are capped and stride over window / entry numbers whose end is read on the
// device, so the launches do not depend on the data.  Nothing is written at or beyond out_off[n] or the caps: the finish
// kernel stops the call when either output does not fit.
#include "mh_select.h"
#include "mh_batch_dev.hpp"
#include "../../include/mh.h"

namespace mhs {

using mhb::BATCH_STATUS_ARG;

namespace {

using mhb::fail;
using mhb::find_stream;
using mhb::grid_for;
using mhb::grid_threads;
using mhb::gtid;
using mhb::stopped;

__global__ __launch_bounds__(256) void select_check_kernel(SelectParams p, unsigned long long *lens, unsigned long long *from,
                                                           unsigned long long *ifrom, int *status, int *stop) {
    const uint64_t t = gtid();
    if (t < p.checks) {
        for (uint32_t s = 0; s < p.n_sources; ++s) {
            const Source &b = p.src[s];
            if (t < b.first || t > b.first + b.n) continue;
            bool bad = mhb::offsets_bad(b.pay_off, b.n, b.pay_total, t - b.first);
            if (b.sym_off) bad |= mhb::offsets_bad(b.sym_off, b.n, b.sym_total, t - b.first);
            if (bad) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
        }
        return;
    }
    const uint64_t j = t - p.checks;
    if (j > p.n) return;
    if (j == p.n) { lens[p.n] = 0; lens[2 * p.n + 1] = 0; return; }
    const uint64_t pick = p.picks[j];
    const uint64_t s = pick >> SRC_SHIFT, i = pick & STREAM_MASK;
    unsigned long long bytes = 0, syms = 0, nb = 0, at = 0, iat = 0;
    int verdict = MH_OK;
    if (pick != NONE) {
        if (s >= p.n_sources || i >= p.src[s].n) verdict = MH_ERR_ARG;
        else {
            const Source &b = p.src[s];
            const uint64_t a = b.pay_off[i];
            nb = b.nbits[i];
            if (nb > (b.pay_off[i + 1] - a) * 8u) { verdict = MH_ERR_ARG; nb = 0; }     // check_batch's rule for one stream
            else {
                bytes = (nb + 7) >> 3;
                at = reinterpret_cast<uintptr_t>(b.payload) + a;
                if (p.have_sym) {
                    const uint64_t so = b.sym_off[i];
                    syms = b.sym_off[i + 1] - so;
                    if (b.index) iat = reinterpret_cast<uintptr_t>(b.index + (so >> p.chunk_shift) + i);
                }
            }
        }
    }
    lens[j] = bytes;
    lens[p.n + 1 + j] = syms;
    from[j] = at;
    ifrom[j] = iat;
    p.out_nbits[j] = nb;
    p.pick_status[j] = verdict;
    if (verdict != MH_OK) fail(status, BATCH_STATUS_ARG);
}

__global__ __launch_bounds__(256) void select_finish_kernel(SelectParams p, const unsigned long long *lens, unsigned long long *osym, int *status,
                                                            int *stop) {
    if (stopped(stop)) return;
    const uint64_t j = gtid();
    if (j > p.n) return;
    const unsigned long long ob = lens[j], os = lens[p.n + 1 + j] - lens[p.n + 1];
    p.out_off[j] = ob;
    osym[j] = os;
    if (p.out_sym_off) p.out_sym_off[j] = os;
    if (j == p.n) {
        const bool pay = p.out && ob > p.cap;
        const bool idx = p.out_index && (os >> p.chunk_shift) + p.n + 1 > p.index_cap;
        if (pay || idx) { fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
    }
}

__global__ __launch_bounds__(256) void select_gather_kernel(const unsigned long long *oo, uint64_t n, const unsigned long long *from, uint8_t *out,
                                                            const int *stop) {
    if (stopped(stop)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwin = (oo[n] >> PIECE_SHIFT) + n;              // the first window number behind the last pick
    const uint64_t wave = uint64_t(blockIdx.x) * 4u + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    // a wave takes GATHER_RUN window numbers in a row: one search for the first, and the owner of the next is this pick or the
    // one behind it (the bases out_off_j / PIECE + j grow strictly with j)
    for (uint64_t u0 = wave * GATHER_RUN; u0 < nwin; u0 += uint64_t(gridDim.x) * 4u * GATHER_RUN) {
        uint64_t j = find_stream(oo, n, PIECE_SHIFT, u0);         // (wave-uniform; j < n as u0 < nwin)
        uint64_t o0 = oo[j], o1 = oo[j + 1];
        const uint64_t end = u0 + GATHER_RUN < nwin ? u0 + GATHER_RUN : nwin;
        for (uint64_t u = u0; u < end; ++u) {
            if (u != u0 && (o1 >> PIECE_SHIFT) + j + 1 <= u) { ++j; o0 = o1; o1 = oo[j + 1]; }
            const uint64_t w0 = ((u - j) << PIECE_SHIFT) + 16u * lane;   // window (o0 / PIECE + u - base_j) of the output, this lane's word
            const uint64_t lo = w0 > o0 ? w0 : o0, hi = w0 + 16u < o1 ? w0 + 16u : o1;
            if (lo >= hi) continue;
            const uint32_t cnt = uint32_t(hi - lo);
            uint32_t x[4];
            mhb::load16(reinterpret_cast<const uint8_t *>(uintptr_t(from[j])) + (lo - o0), cnt, x);
            if (cnt == 16u) *reinterpret_cast<uint4 *>(out + lo) = make_uint4(x[0], x[1], x[2], x[3]);
            else for (uint32_t t = 0; t < cnt; ++t) out[lo + t] = uint8_t(mhb::byte_of(x, t));
        }
    }
}

__global__ __launch_bounds__(256) void select_index_kernel(const unsigned long long *osym, uint64_t n, uint32_t cs, const unsigned long long *ifrom,
                                                           unsigned long long *out_index, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t nent = (osym[n] >> cs) + n;                     // the first entry number behind the last pick
    for (uint64_t w = gtid(); w < nent; w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t j = find_stream(osym, n, cs, w);
        const uint64_t a = osym[j], m = osym[j + 1] - a;
        const uint64_t k = w - ((a >> cs) + j);
        if ((k << cs) >= m) continue;                              // a gap: left untouched
        out_index[w] = reinterpret_cast<const unsigned long long *>(uintptr_t(ifrom[j]))[k];
    }
}

__global__ __launch_bounds__(256) void picks_flag_kernel(PicksParams p, unsigned long long *keep) {
    const uint64_t i = gtid();
    if (i > p.n) return;
    bool k = i < p.n;
    if (k && p.hit_off) k = (p.hit_off[i + 1] > p.hit_off[i]) != bool(p.flags & WITHOUT_HITS);
    if (k && p.stream_status) k = p.stream_status[i] == MH_OK;
    keep[i] = k ? 1u : 0u;
}

// keep: scanned.  Stream i goes to place keep[i] when it is kept (keep[i + 1] > keep[i]); place i >= keep[n] gets MH_SELECT_NONE.
__global__ __launch_bounds__(256) void picks_scatter_kernel(PicksParams p, const unsigned long long *keep) {
    const uint64_t i = gtid();
    if (i > p.n) return;
    const unsigned long long kept = keep[p.n];
    if (i == p.n) { *p.n_kept = kept; return; }
    if (keep[i + 1] > keep[i]) p.picks[keep[i]] = (uint64_t(p.source) << SRC_SHIFT) | i;
    if (i >= kept) p.picks[i] = NONE;
}

}  // namespace

hipError_t launch_select(const SelectParams &p, void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const SelectLayout L = select_layout(p.n);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    unsigned long long *lens = reinterpret_cast<unsigned long long *>(ws + L.off_lens);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    unsigned long long *osym = reinterpret_cast<unsigned long long *>(ws + L.off_osym);
    unsigned long long *from = reinterpret_cast<unsigned long long *>(ws + L.off_from);
    unsigned long long *ifrom = reinterpret_cast<unsigned long long *>(ws + L.off_ifrom);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(select_check_kernel, grid_threads(p.checks + p.n + 1, 256), dim3(256), 0, st, p, lens, from, ifrom, status, stop);
    if ((e = mhb::scan_exclusive(lens, 2 * (p.n + 1), sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(select_finish_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p, lens, osym, status, stop);
    // at most cap bytes and index_cap entries are written, so these bound the window and entry numbers
    if (p.out)
        hipLaunchKernelGGL(select_gather_kernel, dim3(grid_for((p.cap >> PIECE_SHIFT) + p.n + 1, 4 * GATHER_RUN, 16)), dim3(256), 0, st, lens, p.n, from, p.out,
                           stop);
    if (p.out_index)
        hipLaunchKernelGGL(select_index_kernel, dim3(grid_for(p.index_cap + 1, 256, 8)), dim3(256), 0, st, osym, p.n, p.chunk_shift, ifrom,
                           p.out_index, stop);
    return hipGetLastError();
}

hipError_t launch_picks(const PicksParams &p, void *d_ws, hipStream_t st) {
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const PicksLayout L = picks_layout(p.n);
    int *stop = reinterpret_cast<int *>(ws) + 1;
    unsigned long long *keep = reinterpret_cast<unsigned long long *>(ws + L.off_keep);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    hipError_t e = hipMemsetAsync(ws, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(picks_flag_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p, keep);
    if ((e = mhb::scan_exclusive(keep, p.n + 1, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(picks_scatter_kernel, grid_threads(p.n + 1, 256), dim3(256), 0, st, p, keep);
    return hipGetLastError();
}

}  // namespace mhs
