// mh_recode_dev.hpp — the kernels of a re-coding call that never decode, shared by mh_recode.hip and mh_recode_o2.hip: they
// read the source batch and the outputs (mhr::RecodeIO) and neither model.
//   histc_check_kernel       the batch checks (mhb::check_batch) of a coded histogram
//   recode_check_kernel      the batch checks; out_off, nbits and dropped zeroed
//   recode_sizes_kernel      stream i: nbits from the scanned chunk bits, its bytes into out_off
//   recode_cap_kernel        index-free: more symbols than the destination index was sized for -> MHK_STATUS_CAPACITY
//   recode_zero_kernel       clears the payload (edge words are OR-ed) or reports that it does not fit
//   recode_tail_kernel       the bytes of the last, partial dword
// Everything is in an unnamed namespace: each of the two kernel files gets its own copy.
#pragma once

#include "mh_recode.h"
#include "mh_batch_dev.hpp"

namespace mhr {
namespace {

__global__ __launch_bounds__(256) void histc_check_kernel(Src s, int *status, int *stop) {
    const uint64_t i = mhb::gtid();
    if (i > s.b.n) return;
    mhb::check_batch(s.b, i, status, stop);
}

__global__ __launch_bounds__(256) void recode_check_kernel(RecodeIO p, int *status, int *stop) {
    const uint64_t i = mhb::gtid();
    const uint64_t n = p.s.b.n;
    if (i > n) return;
    p.out_off[i] = 0;
    if (!p.s.b.index) p.s.b.sym_off[i] = 0;
    if (i < n) {
        p.out_nbits[i] = 0;
        if (p.dropped) p.dropped[i] = 0;
    }
    mhb::check_batch(p.s.b, i, status, stop);
}

// stream i: payload bits (indexed: from the scanned chunk bits; index-free: the count pass wrote them), bytes into out_off
__global__ __launch_bounds__(256) void recode_sizes_kernel(RecodeIO p, const unsigned long long *cbase, const int *stop) {
    if (mhb::stopped(stop)) return;
    const uint64_t i = mhb::gtid();
    const uint64_t n = p.s.b.n;
    if (i > n) return;
    if (i == n) { p.out_off[i] = 0; return; }
    unsigned long long bits;
    if (p.s.b.index) {
        const uint32_t cs = p.s.b.chunk_shift;
        const uint64_t w0 = (p.s.b.sym_off[i] >> cs) + i, w1 = (p.s.b.sym_off[i + 1] >> cs) + i + 1;
        bits = cbase[w1] - cbase[w0];
        p.out_nbits[i] = bits;
    } else {
        bits = p.out_nbits[i];
    }
    p.out_off[i] = (bits + 7) >> 3;
}

// index-free: the destination index was sized from sym_total; more symbols than that do not fit it (after the scans: offsets
// and lengths are complete)
__global__ void recode_cap_kernel(RecodeIO p, int *status, int *stop) {
    if (mhb::stopped(stop)) return;
    if (p.s.b.sym_off[p.s.b.n] > p.s.b.sym_total) { mhb::fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
}

// zeroes the payload bytes (codes are OR-ed into shared edge dwords) or reports that they do not fit
__global__ __launch_bounds__(256) void recode_zero_kernel(RecodeIO p, int *status, int *stop, uint32_t *tail) {
    if (mhb::stopped(stop)) return;
    const uint64_t bytes = p.out_off[p.s.b.n];
    if (bytes > p.cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { mhb::fail(status, mhk::MHK_STATUS_CAPACITY); atomicExch(stop, 1); }
        return;
    }
    const uint64_t nfull = bytes >> 2;
    uint32_t *o = reinterpret_cast<uint32_t *>(p.out);
    for (uint64_t k = mhb::gtid(); k < nfull; k += uint64_t(gridDim.x) * blockDim.x) o[k] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *tail = 0u;
}

__global__ void recode_tail_kernel(RecodeIO p, const uint32_t *tail, const int *stop) {
    if (mhb::stopped(stop)) return;
    const uint64_t bytes = p.out_off[p.s.b.n];
    if (!(bytes & 3u)) return;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(tail);
    for (uint64_t b = bytes & ~uint64_t(3); b < bytes; ++b) p.out[b] = t[b & 3u];
}

}  // namespace
}  // namespace mhr
