// mh_find_o2.h — launch interface of the search in batches of order-2 streams (include/mh.h, "ORDER 2 IN SEARCH AND
// RE-CODING"; kernels: mh_find_o2.hip).  Pattern set, parameters and workspace layout are those of mh_find.h; the batch is
// described as for launch_decode_batch_o2 (mh_batch_o2.h): b.prev0 is the 16-bit start context, b's tables are the model's
// order-2 tables (general form, L2), index entries carry the context in bits 48..63.
#pragma once

#include "mh_find.h"

namespace mhf {

hipError_t launch_find_o2(const FindParams &p, const Automaton &a, void *d_ws, hipStream_t st);

}  // namespace mhf
