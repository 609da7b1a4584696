// Host idioms of the entry points, each defined once: the status after a launch, pointer alignment, the log-det mode.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/vcnf_hip.h"

namespace vcnf {

static inline bool ok_ld(int m) { return m == VCNF_LD_STORE || m == VCNF_LD_ACCUM; }
static inline int launched() { return hipGetLastError() == hipSuccess ? VCNF_OK : VCNF_ERR_LAUNCH; }
static inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

static inline bool all_aligned(std::initializer_list<const void*> ps, uintptr_t n) {
  for (const void* p : ps)
    if (!aligned(p, n)) return false;
  return true;
}

}  // namespace vcnf
