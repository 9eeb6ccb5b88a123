// mh_recode_o2.h — launch interface of the coded histogram and the re-coding with an order-2 side (include/mh.h, "ORDER 2 IN
// SEARCH AND RE-CODING"; kernels: mh_recode_o2.hip).  The source is mhr::Src of mh_recode.h: an order-0/1 shared model (b's
// tables go to LDS, b.prev0 is a byte, entries carry one context byte) or, with src2, an order-2 shared model (b's tables are
// the order-2 tables in L2, b.prev0 is the 16-bit start context, entries carry two context bytes).
#pragma once

#include "mh_recode.h"

namespace mhr {

// the destination model's encoder tables at (ctx & mask) << 8 | sym: order 2 keeps both context bytes and may have the
// packed table enc64 (len << 56 | code; len 255: longer than 56 bits, read len8 / code64), order 1 the last byte, order 0 none
struct Dst2 {
    const uint8_t *len8;
    const unsigned long long *code64;
    const unsigned long long *enc64;    // order 2 only, may be nullptr
    uint32_t order;
};

// re-code workspace: status block (status, stop, -, -, tail word) | per-stream status (when the caller passes none) | per
// chunk number: destination bits (u64, W + 1, scanned in place), dropped symbols (u32), head bits (u32: the next chunk's first
// symbol under dst) and closing context (u32: the chunk's last two symbols) | scan block sums
struct Recode2Layout {
    size_t off_status, off_bits, off_drop, off_head, off_close, off_sums, total;
};
inline Recode2Layout recode2_layout(uint64_t n_streams, uint64_t nwork) {
    Recode2Layout l;
    const uint64_t len = (nwork > n_streams ? nwork : n_streams) + 1;
    l.off_status = 64;
    l.off_bits = (l.off_status + size_t(n_streams) * 4 + 15) & ~size_t(15);
    l.off_drop = l.off_bits + size_t(nwork + 1) * 8;
    l.off_head = l.off_drop + size_t(nwork) * 4;
    l.off_close = l.off_head + size_t(nwork) * 4;
    l.off_sums = (l.off_close + size_t(nwork) * 4 + 15) & ~size_t(15);
    l.total = (l.off_sums + size_t(mhb::scan_blocks(len) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

struct Hist2Params {
    Src s;
    bool src2;                      // the source model is order 2
    uint32_t order;                 // of the histogram: 0 (256 counts), 1 (65 536) or 2 (1 << 24)
    unsigned long long *counts;
};

struct Recode2Params : RecodeIO {
    bool src2;
    Dst2 dst;
};

hipError_t launch_histogram_coded_o2(const Hist2Params &p, void *d_ws, hipStream_t st);
hipError_t launch_recode_o2(const Recode2Params &p, void *d_ws, hipStream_t st);

}  // namespace mhr
