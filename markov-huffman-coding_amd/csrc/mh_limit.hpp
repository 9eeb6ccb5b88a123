// mh_limit.hpp — length-limited models: a context whose reference tree is deeper than the limit is re-coded
// by package-merge with canonical codewords; every other context keeps its reference tree.  Host build (mh_limit_host.cpp) and
// device build (mh_limit.hip) give the same trees, node for node.
// (Files of their own, and nothing added to mh_model.hpp / mh_kernels.h / mh_tree.hip: those are hashed into every committed
// counter figure, see provenance.py, and no existing kernel changes with this feature.)
#pragma once

#include <cstdint>

#include "mh_kernels.h"
#include "mh_model.hpp"

namespace mh {

constexpr int LIMIT_MIN_LEN = 8, LIMIT_MAX_LEN = 64;
constexpr uint64_t LIMIT_MAX_TOTAL = 1ull << 56;     // package weights (<= 64 context totals) stay below 2^62
inline bool limit_valid(int max_len) { return max_len == 0 || (max_len >= LIMIT_MIN_LEN && max_len <= LIMIT_MAX_LEN); }

// ContextCoder::build_from_counts with a limit.  max_len = 0: the reference tree.  Otherwise (LIMIT_MIN_LEN..LIMIT_MAX_LEN) a
// tree deeper than max_len is replaced by the optimal code of at most max_len bits; false (and an empty context) when
// that needs a context total of LIMIT_MAX_TOTAL or more.
bool build_context_limited(ContextCoder &c, const uint64_t *counts256, int max_len);
// Model::build_from_counts with a limit (order 0 / 1).
bool build_model_limited(Model &m, const uint64_t *counts, int order, int max_len);

}  // namespace mh

namespace mhk {
// behind launch_tree_build on the same stream: re-codes, in place, every context whose longest code (ctx_meta[2]) exceeds
// max_len bits; the others exit at once
hipError_t launch_tree_limit(const unsigned long long *d_counts, int nctx, uint32_t max_len, const TreeBuildOut &o, hipStream_t st);
}  // namespace mhk
