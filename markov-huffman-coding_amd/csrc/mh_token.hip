// mh_token.hip — a replacement table computed from the matched bytes of a compressed batch (include/mh.h, "TOKENS FROM
// MATCHED BYTES"): span r's entry is its format's prefix, hex digits of the keyed SipHash-2-4 of the span's bytes, and the
// suffix.  The bytes are decoded into a register, absorbed and dropped: none is stored.
//   token_check_kernel               thread i <= n: the batch's offsets as the batch decoders check them, span_off as any
//                                    offsets, stream i's verdict (MH_OK; MH_ERR_ARG for nbits beyond its payload or a list that
//                                    breaks the table splice's span rule) judged by the one lane that owns the stream; thread k:
//                                    entry k of the formats; more spans than table entries: MHK_STATUS_CAPACITY
//   token_digest_kernel<Tables, I>   indexed: one lane per span on a grid-stride loop up to span_off[n] (read on the device).
//                                    The lane starts at the index entry of the span's first chunk, decodes and drops the
//                                    symbols in front, absorbs the span's and decodes on over chunk boundaries; at each one,
//                                    and at len(x), its bit position must be the next entry's (nbits at the end), which is
//                                    lookup_kernel's `exact` test.  Index-free: one lane per stream with spans walks from bit 0
//                                    in prev0, digests the spans in list order (they ascend) and walks on to nbits for the
//                                    batch decoder's verdict.
//   token_lens_kernel                entry r's length (0 for a failed stream and behind the last span) and rep_tag[r] = r
//   mhb::scan_exclusive              rep_off, in the caller's array
//   token_emit_kernel                one thread per byte of the table, entry found by item_of over rep_off
// The symbol decoders, item_of and tables_room are mh_range_dev.hpp's; the launch rule of the shared model is the lookups'.
#include "mh_token.h"
#include "mh_range_dev.hpp"

namespace mht {

using mhb::BATCH_STATUS_ARG;
using mhb::Model;
using mhk::BitCursor;
using mhk::BitSrc;

namespace {

using mhb::fail;
using mhb::grid_for;
using mhb::gtid;
using mhb::stopped;
using mhq::item_of;

__device__ __forceinline__ void stream_fail(const TokenParams &p, int *status, uint64_t i, int mh_code, int dev_code) {
    p.stream_status[i] = mh_code;
    fail(status, dev_code);
}

__global__ __launch_bounds__(256) void token_check_kernel(TokenParams p, int *status, int *stop) {
    const uint64_t n = p.b.n_streams, stride = uint64_t(gridDim.x) * blockDim.x;
    const unsigned long long *off = p.span_off;
    const uint64_t total = off[n];
    if (gtid() == 0) {
        if (total > p.n_reps) { fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
        else if (total && !p.n_formats) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
    }
    for (uint64_t k = gtid(); k <= 2 * p.n_formats; k += stride)
        if (format_entry_bad(p.fmt_off, p.hex_digits, p.n_formats, k)) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
    for (uint64_t i = gtid(); i <= n; i += stride) {
        bool bad = mhb::offsets_bad(p.b.pay_off, n, p.pay_total, i) || mhb::offsets_bad(off, n, total, i);
        if (p.b.index) bad |= mhb::offsets_bad(p.b.sym_off, n, p.sym_total, i);
        if (bad) { fail(status, BATCH_STATUS_ARG); atomicExch(stop, 1); }
        if (i == n) continue;
        p.stream_status[i] = MH_OK;
        const uint64_t q0 = off[i], q1 = off[i + 1];
        // (offsets that fail above stop the call; a list is read only where it lies inside the table's entries)
        if (bad || q0 >= q1 || q1 > p.n_reps) continue;
        bool arg = p.b.nbits[i] > (p.b.pay_off[i + 1] - p.b.pay_off[i]) * 8u;
        unsigned long long prev_end = 0;
        for (uint64_t r = q0; r < q1 && !arg; ++r) {
            const unsigned long long b = p.spans[2 * r], e = p.spans[2 * r + 1];
            arg = b > e || b < prev_end || (p.span_tag && p.span_tag[r] >= p.n_formats);
            prev_end = e;
        }
        if (arg) stream_fail(p, status, i, MH_ERR_ARG, BATCH_STATUS_ARG);
    }
}

template <typename Tables, bool INDEXED>
__global__ __launch_bounds__(Tables::BOUND) void token_digest_kernel(TokenParams p, unsigned long long *digest, int *status, const int *stop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (stopped(stop)) return;
    Tables tb;
    tb.init(p.b, smem);
    const uint64_t n = p.b.n_streams, stride = uint64_t(gridDim.x) * blockDim.x;
    if (!n) return;
    const unsigned long long *off = p.span_off;
    if (INDEXED) {
        const uint64_t total = off[n];
        const uint32_t cs = p.b.chunk_shift;
        const uint64_t U = uint64_t(1) << cs;
        for (uint64_t r = gtid(); r < total; r += stride) {
            const uint64_t i = item_of(off, n, r);
            Sip h;
            h.init(p.k0, p.k1);
            if (p.stream_status[i] == MH_ERR_ARG) continue;
            const uint64_t ni = p.b.sym_off[i + 1] - p.b.sym_off[i];
            const uint64_t b = p.spans[2 * r];
            const uint64_t e = p.spans[2 * r + 1] < ni ? p.spans[2 * r + 1] : ni;
            if (b < e) {
                const uint64_t nb = p.b.nbits[i];
                const uint64_t g0 = (p.b.sym_off[i] >> cs) + i;       // the stream's first entry in the batch index
                const uint64_t c = b >> cs;
                const uint64_t ent = p.b.index[g0 + c];
                uint64_t s = ent & Tables::POS;
                if (s > nb || (c > 0 && s < (p.b.index[g0 + c - 1] & Tables::POS))) {
                    stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                    continue;
                }
                tb.stream(p.b, i);
                uint64_t bit0;
                const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[i], nb, bit0);
                BitCursor bc;
                bc.init(src, bit0 + s);
                uint32_t ctx = Tables::entry_ctx(ent), used = 0;
                bool bad = false;
                uint64_t t = c << cs;
                for (; t < b && !bad; ++t) tb.next(p.b, src, bc, ctx, used, bad);
                while (t < e && !bad) {
                    const uint32_t sym = tb.next(p.b, src, bc, ctx, used, bad);
                    if (bad) break;
                    h.put(sym, p.fold);
                    ++t;
                    // a boundary crossed or reached, and the end of the message: exactly the bits up to the next entry
                    if ((t & (U - 1)) == 0 || t == ni) {
                        const uint64_t next = t == ni ? nb : (p.b.index[g0 + (t >> cs)] & Tables::POS);
                        if (s + used != next) { bad = true; break; }
                        s = next;
                        used = 0;
                    }
                }
                if (bad || s + used > nb) {
                    stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
                    continue;
                }
            }
            digest[r] = h.finish();
        }
    } else {
        for (uint64_t i = gtid(); i < n; i += stride) {
            const uint64_t q0 = off[i], q1 = off[i + 1];
            if (q0 == q1 || p.stream_status[i] != MH_OK) continue;
            const uint64_t nb = p.b.nbits[i];
            if (nb > p.b.walk_max_bits) { stream_fail(p, status, i, MH_ERR_ARG, BATCH_STATUS_ARG); continue; }
            tb.stream(p.b, i);
            uint64_t bit0;
            const BitSrc src = mhb::stream_src(p.b.payload, p.b.pay_off[i], nb, bit0);
            BitCursor bc;
            bc.init(src, bit0);
            // (nb <= walk_max_bits < 2^32, and every code has at least one bit: at most nb steps)
            uint32_t ctx = p.b.prev0, used = 0;
            bool bad = false;
            uint64_t t = 0;
            for (uint64_t q = q0; q < q1 && !bad; ++q) {
                const uint64_t b = p.spans[2 * q], e = p.spans[2 * q + 1];
                for (; t < b && used < nb && !bad; ++t) tb.next(p.b, src, bc, ctx, used, bad);
                Sip h;
                h.init(p.k0, p.k1);
                while (t < e && used < nb && !bad) {
                    const uint32_t sym = tb.next(p.b, src, bc, ctx, used, bad);
                    if (bad) break;
                    h.put(sym, p.fold);
                    ++t;
                }
                digest[q] = h.finish();
            }
            // the rest of the stream, for the verdict of the batch decoder's walk: the stream ends exactly at nbits
            while (used < nb && !bad) tb.next(p.b, src, bc, ctx, used, bad);
            if (bad || used != nb) stream_fail(p, status, i, MH_ERR_CORRUPT, mhk::MHK_STATUS_CORRUPT);
        }
    }
}

// span r's format
__device__ __forceinline__ uint64_t format_of(const TokenParams &p, uint64_t r) { return p.span_tag ? p.span_tag[r] : 0u; }

__global__ __launch_bounds__(256) void token_lens_kernel(TokenParams p, const int *stop) {
    if (stopped(stop)) return;
    const uint64_t n = p.b.n_streams, total = n ? p.span_off[n] : 0;
    for (uint64_t r = gtid(); r <= p.n_reps; r += uint64_t(gridDim.x) * blockDim.x) {
        unsigned long long len = 0;
        if (r < total && p.stream_status[item_of(p.span_off, n, r)] == MH_OK) {
            const uint64_t f = format_of(p, r);
            len = p.fmt_off[2 * f + 2] - p.fmt_off[2 * f] + p.hex_digits[f];
        }
        p.rep_off[r] = len;
        if (r < p.n_reps) p.rep_tag[r] = uint32_t(r);
    }
}

__global__ __launch_bounds__(256) void token_emit_kernel(TokenParams p, const unsigned long long *digest, int *status, int *stop) {
    if (stopped(stop)) return;
    const uint64_t bytes = p.rep_off[p.n_reps];
    if (!p.rep_bytes) return;                                       // count only
    if (bytes > p.rep_cap) {
        if (gtid() == 0) fail(status, mhk::MHK_STATUS_CAPACITY);
        return;
    }
    for (uint64_t w = gtid(); w < bytes; w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t r = item_of(p.rep_off, p.n_reps, w);        // (empty entries share their successor's offset)
        const uint64_t f = format_of(p, r);
        const uint64_t k = w - p.rep_off[r], pre = p.fmt_off[2 * f + 1] - p.fmt_off[2 * f], hex = p.hex_digits[f];
        uint8_t c;
        if (k < pre) c = p.fmt_bytes[p.fmt_off[2 * f] + k];
        else if (k < pre + hex) {
            const uint32_t nib = uint32_t(digest[r] >> (60u - 4u * uint32_t(k - pre))) & 15u;   // "%016x", from the left
            c = uint8_t(nib < 10u ? '0' + nib : 'a' + (nib - 10u));
        } else c = p.fmt_bytes[p.fmt_off[2 * f + 1] + (k - pre - hex)];
        p.rep_bytes[w] = c;
    }
}

template <typename Tables>
hipError_t launch(const TokenParams &p, void *d_ws, hipStream_t st) {
    size_t lds;
    hipError_t e = mhq::tables_room<Tables>(p.b, {reinterpret_cast<const void *>(token_digest_kernel<Tables, true>),
                                                  reinterpret_cast<const void *>(token_digest_kernel<Tables, false>)}, lds);
    if (e != hipSuccess) return e;
    unsigned char *ws = static_cast<unsigned char *>(d_ws);
    const TokenLayout L = token_layout(p.n_reps);
    int *status = reinterpret_cast<int *>(ws), *stop = status + 1;
    auto *digest = reinterpret_cast<unsigned long long *>(ws + L.off_digest);
    auto *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    if ((e = hipMemsetAsync(ws, 0, 64, st)) != hipSuccess) return e;
    const uint64_t checks = std::max<uint64_t>(p.b.n_streams + 1, 2 * p.n_formats + 1);
    hipLaunchKernelGGL(token_check_kernel, dim3(grid_for(checks, 256, 8)), dim3(256), 0, st, p, status, stop);
    // lanes: the spans the table has room for (their number is on the device), or the streams; the shared model's workgroups
    // as the lookups size them
    const uint64_t lanes = p.b.index ? p.n_reps : p.b.n_streams;
    const int threads = Tables::LDS && lanes >= uint64_t(mhk::cu_count()) * mhq::SPREAD ? Tables::BOUND : 256;
    if (p.b.index)
        hipLaunchKernelGGL((token_digest_kernel<Tables, true>), dim3(grid_for(lanes, uint64_t(threads), Tables::PER_CU)), dim3(threads), lds, st, p,
                           digest, status, stop);
    else
        hipLaunchKernelGGL((token_digest_kernel<Tables, false>), dim3(grid_for(lanes, uint64_t(threads), Tables::PER_CU)), dim3(threads), lds, st, p,
                           digest, status, stop);
    hipLaunchKernelGGL(token_lens_kernel, dim3(grid_for(p.n_reps + 1, 256, 8)), dim3(256), 0, st, p, stop);
    if ((e = mhb::scan_exclusive(p.rep_off, p.n_reps + 1, sums, stop, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(token_emit_kernel, dim3(grid_for(p.rep_bytes ? p.rep_cap : 1, 256, 8)), dim3(256), 0, st, p, digest, status, stop);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_span_tokens(const TokenParams &p, Model model, void *d_ws, hipStream_t st) {
    switch (model) {
    case Model::Shared: return launch<mhq::SharedTables>(p, d_ws, st);
    case Model::Set: return launch<mhq::SetTables>(p, d_ws, st);
    case Model::Shared2: return launch<mhq::Shared2Tables>(p, d_ws, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mht
