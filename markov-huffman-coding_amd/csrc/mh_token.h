// mh_token.h — launch interface between the span-token call of the C ABI (mh_api_token.cpp) and its kernels (mh_token.hip)
// (include/mh.h, "TOKENS FROM MATCHED BYTES").  The token itself, SipHash-2-4 and the format rules, is mh_token_sip.hpp's:
// plain C++ that host and device share.  The batch is a LookupParams (mh_range.h): the lookups' view of a batch under any
// model kind, whose lookup and output fields stay unused.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mh_range.h"
#include "mh_token_sip.hpp"

namespace mht {

// ---------------------------------------------------------------------------------------------------- the device call

// workspace: status block (int32 status at 0, stop at 4) | digests (u64, one per table entry) | scan block sums
struct TokenLayout {
    size_t off_digest, off_sums, total;
};
inline TokenLayout token_layout(uint64_t n_reps) {
    TokenLayout l;
    l.off_digest = 64;
    l.off_sums = l.off_digest + size_t(n_reps) * 8;
    l.total = (l.off_sums + size_t(mhb::scan_blocks(n_reps + 1) + 1) * 8 + 255) & ~size_t(255);
    return l;
}

struct TokenParams {
    mhq::LookupParams b;                  // the batch and its model (lookups, out, out_at, status unused)
    uint64_t pay_total, sym_total;
    int *stream_status;                   // n_streams
    const unsigned long long *span_off;   // n_streams + 1
    const unsigned long long *spans;      // 2 per span
    const uint32_t *span_tag;             // nullptr: format 0
    uint64_t k0, k1;
    bool fold;
    const uint64_t *fmt_off;              // 2 * n_formats + 1
    const uint8_t *fmt_bytes;
    const uint8_t *hex_digits;            // n_formats
    uint64_t n_formats;
    uint64_t n_reps;                      // entries of the table written: span r's is entry r, the rest are empty
    unsigned long long *rep_off;          // n_reps + 1 (written)
    uint8_t *rep_bytes;                   // nullptr: count only
    uint64_t rep_cap;
    uint32_t *rep_tag;                    // n_reps (written): r
};

hipError_t launch_span_tokens(const TokenParams &p, mhb::Model model, void *d_ws, hipStream_t st);

}  // namespace mht
