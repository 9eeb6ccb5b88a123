// mh_find.h — the pattern set (host object) and the launch interface between the search calls of the C ABI
// (mh_api_find.cpp) and their kernels (mh_find.hip): which streams of a batch contain which byte strings, and where, found
// on the decoded symbols while they sit in a register (include/mh.h, "SEARCH IN BATCHES").  The batch layouts (packed
// payloads, closed-form index slices) are those of mh_batch.h; the per-stream models those of mh_each.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_batch.h"
#include "mh_dict.h"
#include "mh_each.h"

// The Shift-And automaton of a pattern set over one 64-bit word: pattern j owns len_j consecutive bits, ascending with j;
// mask[c] has a bit where that position accepts byte c, `first` the lowest bit of every pattern, `last` the highest.  Per
// symbol c: D = ((D << 1) | first) & mask[c]; the patterns that end at c are D & last.  A bit that leaves one pattern's top
// lands on the next pattern's lowest bit, which `first` sets anyway.
struct mh_pattern_set {
    uint64_t mask[256];
    uint64_t first = 0, last = 0;
    uint32_t n = 0, max_len = 0, flags = 0;
};

namespace mhf {

// the automaton as a kernel argument: only the check kernel takes it, and copies the masks into the workspace
struct Automaton {
    uint64_t mask[256];
};

// workspace: status block | mask u64[256] | per-stream status (when the caller passes none) | per chunk: end state D (u64),
// own count (u32), tail count (u32) | hits that end in the chunk (u64, W + 1, scanned in place) | scan block sums
struct FindLayout {
    size_t off_mask, off_status, off_state, off_own, off_tail, off_cnt, off_sums, total;
};
inline FindLayout find_layout(uint64_t n_streams, uint64_t nwork) {
    FindLayout l;
    const uint64_t len = (nwork > n_streams ? nwork : n_streams) + 1;
    l.off_mask = 64;
    l.off_status = l.off_mask + 2048;
    l.off_state = (l.off_status + size_t(n_streams) * 4 + 15) & ~size_t(15);
    l.off_own = l.off_state + size_t(nwork) * 8;
    l.off_tail = l.off_own + size_t(nwork) * 4;
    l.off_cnt = (l.off_tail + size_t(nwork) * 4 + 15) & ~size_t(15);
    l.off_sums = l.off_cnt + size_t(nwork + 1) * 8;
    l.total = (l.off_sums + size_t(mhb::scan_blocks(len) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

struct FindParams {
    mhb::DecBatchParams b;          // the batch and, under a shared model, its decode tables (out / out_cap unused; sym_off read only)
    mhe::SetDev set;                // the models under a set
    uint64_t first, last;           // the automaton's words (the masks travel through the workspace)
    uint32_t max_len;
    unsigned long long *hit_off;    // n + 1 (written)
    unsigned long long *hits;       // 3 x hit_cap, or nullptr: count only
    uint32_t *hit_pattern;          // hit_cap, or nullptr
    uint64_t hit_cap;
};

// model: what the batch was coded under (mhb::Model, mh_batch.h); b's tables and b.prev0 as that model's batch decoder takes them
using mhb::Model;
hipError_t launch_find(const FindParams &p, const Automaton &a, Model model, void *d_ws, hipStream_t st);
// the same search with a dictionary's DFA as the matcher (mh_dict.h): p.first / last / max_len unused, same workspace
hipError_t launch_find_dict(const FindParams &p, const mhd::DictDev &d, Model model, void *d_ws, hipStream_t st);

}  // namespace mhf
