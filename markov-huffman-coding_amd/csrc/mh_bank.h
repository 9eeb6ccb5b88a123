// mh_bank.h — launch interface between the bank calls of the C ABI (mh_api_bank.cpp) and their kernels (mh_bank.hip): K shared
// order-0/1 models, each stream coded under the one that suits it best (include/mh.h, "BANKS OF SHARED MODELS").  A bank is a
// model set (mh_each.h, SetDev) whose K streams are the shared models; the batch layouts are those of mh_batch.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"
#include "mh_each.h"

namespace mhbank {

constexpr uint32_t BANK_MAX = 64;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t IMG_BYTES = 65536;          // one entry's length image: len[ctx][sym], 0 = no code
constexpr uint32_t G = 2;                      // entry images per workgroup of the select kernel (128 KiB of LDS)

// select workspace: status block | K length images | nbits per (stream, entry) | uncovered entries per stream (bit k)
struct SelLayout {
    size_t off_img, off_sums, off_miss, total;
};
inline SelLayout sel_layout(uint64_t k, uint64_t n) {
    SelLayout l;
    l.off_img = 256;
    l.off_sums = l.off_img + size_t(k) * IMG_BYTES;
    l.off_miss = l.off_sums + size_t(n) * size_t(k) * 8;
    l.total = (l.off_miss + size_t(n) * 8 + 255) & ~size_t(255);
    return l;
}

hipError_t launch_select(const mhe::SetDev &bank, const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, uint64_t total,
                         uint32_t prev0, uint32_t *d_choice, unsigned long long *d_nbits, void *d_ws, hipStream_t st);

// offsets check alone: status block of d_ws (status, stop), as the batch kernels report it
hipError_t launch_check(const uint64_t *d_in_off, uint64_t n, uint64_t total, void *d_ws, hipStream_t st);

// the view's rows from the bank's entries; a choice >= K sets *status to mhb::BATCH_STATUS_ARG
hipError_t launch_pick(const mhe::SetDev &bank, const uint32_t *d_choice, const mhe::SetDev &view, int *status, hipStream_t st);

// Training: streams sorted by group (stable) and gathered, each group's bytes from a 16-byte aligned base.
//   gdata    gathered bytes (total + 16 K + 16)
//   goff     n + 1: exclusive scan of the sorted lengths (u64); sums: its scan block sums
//   coff     n + K: group c's n_c + 1 offsets, re-based to the group's first byte, from entry start_c + c
//   perm     n: sorted position -> stream; bcnt: per (block of 1024 streams, group) counts, scanned to bases
//   summary  3 (K + 1) u64: start_c (streams), gbase_c (byte base of group c in gdata, 16-aligned), bytes_c; c = 0 .. K
struct GatherBufs {
    uint8_t *gdata;
    unsigned long long *goff, *sums, *coff, *summary;
    uint32_t *perm, *bcnt;
};
constexpr uint32_t SORT_BLOCK = 1024;
hipError_t launch_gather(const uint8_t *d_data, const uint64_t *d_in_off, uint64_t n, const uint32_t *d_group, uint32_t k,
                         const GatherBufs &g, const int *stop, hipStream_t st);
// *changed = the streams whose new choice differs from remap[old group] (remap: K entries, NONE for a dropped group)
hipError_t launch_changed(const uint32_t *d_old, const uint32_t *d_new, const uint32_t *d_remap, uint64_t n, unsigned long long *changed,
                          hipStream_t st);

}  // namespace mhbank
