// Host idioms of the entry points, each defined once: the dispatch from a run-time count or code (with_listed_only,
// launch_listed) and from run-time booleans (with_flags) to a kernel instance, the status after a launch, pointer
// alignment, the log-det mode, the dynamic-LDS limit of a kernel, the launch end of a tiled kernel (launch_tiled).
// The first part is plain C++17 (rqs_host.hpp includes it and is compiled without HIP by tests/c_host/); the rest needs
// the HIP runtime.
#pragma once

#include <stdint.h>

#include <initializer_list>
#include <type_traits>
#include <utility>

#include "../../include/vcnf_hip.h"

namespace vcnf {

// Run-time integers that have kernel instances of their own (bin counts, k-step counts).
template <int... Ns>
using IntList = std::integer_sequence<int, Ns...>;

template <int First, int... Is>
constexpr IntList<(First + Is)...> int_range_from(std::integer_sequence<int, Is...>) { return {}; }
// First, First + 1, ..., First + Count - 1
template <int First, int Count>
using IntRange = decltype(int_range_from<First>(std::make_integer_sequence<int, Count>{}));

template <int... Ns>
inline bool in_list(IntList<Ns...>, int n) {
  return ((n == Ns) || ...);
}

// f(std::integral_constant<int, n>{}) if n is one of Ns (true), else nothing (false)
template <int... Ns, class F>
inline bool with_listed_only(IntList<Ns...>, int n, F&& f) {
  return ((n == Ns && (f(std::integral_constant<int, Ns>{}), true)) || ...);
}

// f(std::bool_constant<b>{}...) for the run-time booleans b..., in their order, and what f returns (a status)
template <class F>
inline auto with_flags(F&& f) {
  return f();
}
template <class F, class... Bools>
inline auto with_flags(F&& f, bool b, Bools... rest) {
  if (b) return with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
  return with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

}  // namespace vcnf

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace vcnf {

static inline bool ok_ld(int m) { return m == VCNF_LD_STORE || m == VCNF_LD_ACCUM; }
static inline int launched() { return hipGetLastError() == hipSuccess ? VCNF_OK : VCNF_ERR_LAUNCH; }
static inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

static inline bool all_aligned(std::initializer_list<const void*> ps, uintptr_t n) {
  for (const void* p : ps)
    if (!aligned(p, n)) return false;
  return true;
}

// VCNF_ERR_UNSUPPORTED unless n is listed; else launch(std::integral_constant<int, n>{})'s status
template <int... Ns, class F>
inline int launch_listed(IntList<Ns...> list, int n, F&& launch) {
  int rc = VCNF_ERR_UNSUPPORTED;
  with_listed_only(list, n, [&](auto N) { rc = launch(N); });
  return rc;
}

// Dynamic LDS a kernel may be launched with before its limit has been raised; a unit that sizes its LDS at run time
// (made_sample.hip) stays below it, so that it needs no per-instance flag.
constexpr size_t kDynamicLdsDefault = 64 * 1024;

// Raises Kernel's dynamic-LDS limit to ``bytes`` on its first launch (above 64 KiB the runtime wants to be told); the
// flag is per kernel instance, so ``bytes`` must be a constant of the instance.  False if the runtime refuses: the
// caller returns VCNF_ERR_LAUNCH.
template <auto Kernel>
inline bool lds_limit_once(size_t bytes) {
  static bool done = false;
  if (!done)
    done = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes) == hipSuccess;
  return done;
}

// The launch end of a kernel that walks the batch in tiles of TILE samples and has an instance per direction: raises the
// instance's dynamic-LDS limit once where LDS exceeds 64 KiB (VCNF_ERR_LAUNCH if the runtime refuses), one workgroup of
// BLOCK threads per tile up to ``max_grid`` (what the chip holds at once), launches KInv or KFwd on ``args``.
template <auto KInv, auto KFwd, int TILE, int BLOCK, size_t LDS, class... Args>
inline int launch_tiled(int inverse, long long batch, long long max_grid, hipStream_t st, const Args&... args) {
  if constexpr (LDS > kDynamicLdsDefault) {
    if (!(inverse ? lds_limit_once<KInv>(LDS) : lds_limit_once<KFwd>(LDS))) return VCNF_ERR_LAUNCH;
  }
  const long long ntiles = (batch + TILE - 1) / TILE;
  const dim3 grid((unsigned)(ntiles < max_grid ? ntiles : max_grid));
  if (inverse)
    hipLaunchKernelGGL(KInv, grid, dim3(BLOCK), LDS, st, args...);
  else
    hipLaunchKernelGGL(KFwd, grid, dim3(BLOCK), LDS, st, args...);
  return launched();
}

}  // namespace vcnf
#endif  // __HIPCC__
