// mh_token_host.cpp — the token of a byte string and the format rules on the host (include/mh.h, "TOKENS FROM MATCHED
// BYTES"): plain C++, no HIP, no device.  The sanitizer fuzz (sanitize/fuzz_tokens.cpp) links this file alone.
#include "mh_token_sip.hpp"

#include "../../include/mh.h"

namespace mht {

int formats_check(const uint64_t *fmt_off, const uint8_t *fmt_bytes, const uint8_t *hex_digits, size_t n_formats) {
    if (!fmt_off || (n_formats && !hex_digits)) return MH_ERR_ARG;
    for (uint64_t k = 0; k <= 2 * uint64_t(n_formats); ++k)
        if (format_entry_bad(fmt_off, hex_digits, n_formats, k)) return MH_ERR_ARG;
    if (fmt_off[2 * n_formats] && !fmt_bytes) return MH_ERR_ARG;
    return MH_OK;
}

}  // namespace mht

extern "C" uint64_t mh_span_token_digest(const uint8_t *key, const uint8_t *bytes, size_t n, uint32_t flags) {
    if (!key || (!bytes && n)) return 0;
    mht::Sip h;
    h.init(mht::load_le64(key), mht::load_le64(key + 8));
    const bool fold = (flags & MH_TOKEN_FOLD) != 0;
    for (size_t k = 0; k < n; ++k) h.put(bytes[k], fold);
    return h.finish();
}
