// sparse_args.hpp — the part of the sparse getters (sparse.cpp) that runs without a device: the argument checks every
// entry point makes before it looks at its handle, and the cap / growth arithmetic.  It includes no HIP header, so
// tools/sparse_args_check.cpp builds it alone under a sanitizer.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/pprhip.h"

namespace pprhip {
void set_error(const char* fmt, ...);

namespace detail {

// threshold finite and >= 0 (NaN fails the test), order in {0, 1}, a count pointer (have_offsets: false when
// pprhip_results_fetch_sparse_all got no offsets_out), no output buffer with cap == 0
inline int sparse_check_args(const char* fn, double threshold, int order, const void* ids_out, const void* vals_out,
                             uint64_t cap, const void* count_out, bool have_offsets) {
  if (!(threshold >= 0.0 && std::isfinite(threshold))) {
    set_error("%s: threshold = %g must be finite and >= 0", fn, threshold);
    return PPRHIP_ERR_INVALID;
  }
  if (order != PPRHIP_SPARSE_BY_ID && order != PPRHIP_SPARSE_BY_VALUE) {
    set_error("%s: order = %d must be 0 (by id) or 1 (by value)", fn, order);
    return PPRHIP_ERR_INVALID;
  }
  if (!count_out) {
    set_error("%s: null count pointer", fn);
    return PPRHIP_ERR_INVALID;
  }
  if (!have_offsets) {
    set_error("%s: null offsets_out", fn);
    return PPRHIP_ERR_INVALID;
  }
  if (cap == 0 && (ids_out || vals_out)) {
    set_error("%s: an output buffer with cap = 0", fn);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

// entries a call writes: the first min(cap, total) of the ordered sequence; none when no buffer was given
inline uint64_t sparse_take(uint64_t cap, uint64_t total, bool have_buffer) {
  if (!have_buffer) return 0;
  return cap < total ? cap : total;
}

// capacity to allocate when `need` entries do not fit: an eighth more, so that a run of slowly growing supports does not
// allocate every time; saturates instead of wrapping
inline size_t sparse_grown(size_t need) {
  const size_t extra = need / 8 + 64;
  return need > SIZE_MAX - extra ? SIZE_MAX : need + extra;
}

}  // namespace detail
}  // namespace pprhip
