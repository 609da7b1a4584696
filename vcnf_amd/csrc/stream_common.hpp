// What the stream kernels share (affine_kernels.hip, class_cond_gaussian.hip, gaussian_mixture.hip, heavy_tail.hip,
// mvn_base.hip, planar_radial.hip, target_density.hip, stochastic.hip, vae_ends.hip, periodic.hip, logit.hip): a group of
// G <= 64 lanes (a power of two) owns a sample, streams its row in packs of up to 16 bytes and sums with a shuffle
// butterfly.
// Each unit keeps its kernels, argument structs and tuning constants (block sizes, grid caps, packs per lane) in its own
// namespace; this header holds the scaffolding around them, each piece defined once.  On the host side that is the
// choice of lanes, pack and grid, and the way from run-time values to a kernel instance: with_pack for the pack width,
// host_common.hpp's with_flags for booleans and launch_listed for a family code.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/vcnf_hip.h"
#include "host_common.hpp"

namespace vcnf_stream {

// ------------------------------------------------------------------ device side
// V elements moved by one load / store
template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
  T v[V];
};

// A row cut into chunks of 16 bytes' worth of columns (vae_ends.hip, periodic.hip): which lane owns which chunk is fixed
// by the shape, and only how a chunk is moved - one pack of 16 bytes, two of 8, or scalars - follows the alignment.
template <typename T>
constexpr int chunk_width() { return 16 / (int)sizeof(T); }

// the first cnt columns of the chunk at src (cnt a multiple of V) in packs of V
template <typename T, int V>
__device__ __forceinline__ void load_chunk(T* d, const T* __restrict__ src, int cnt) {
  constexpr int W = chunk_width<T>();
#pragma unroll
  for (int k = 0; k < W / V; ++k)
    if (k * V < cnt) {
      const Pack<T, V> q = *reinterpret_cast<const Pack<T, V>*>(src + k * V);
#pragma unroll
      for (int j = 0; j < V; ++j) d[k * V + j] = q.v[j];
    }
}

template <typename T, int V>
__device__ __forceinline__ void store_chunk(T* __restrict__ dst, const T* s, int cnt) {
  constexpr int W = chunk_width<T>();
#pragma unroll
  for (int k = 0; k < W / V; ++k)
    if (k * V < cnt) {
      Pack<T, V> q;
#pragma unroll
      for (int j = 0; j < V; ++j) q.v[j] = s[k * V + j];
      *reinterpret_cast<Pack<T, V>*>(dst + k * V) = q;
    }
}

__device__ __forceinline__ float exp_(float v) { return expf(v); }
__device__ __forceinline__ double exp_(double v) { return exp(v); }
__device__ __forceinline__ float log_(float v) { return logf(v); }
__device__ __forceinline__ double log_(double v) { return log(v); }
__device__ __forceinline__ float log1p_(float v) { return log1pf(v); }
__device__ __forceinline__ double log1p_(double v) { return log1p(v); }
__device__ __forceinline__ float sqrt_(float v) { return sqrtf(v); }
__device__ __forceinline__ double sqrt_(double v) { return sqrt(v); }
__device__ __forceinline__ float abs_(float v) { return fabsf(v); }
__device__ __forceinline__ double abs_(double v) { return fabs(v); }
__device__ __forceinline__ void sincos_(float v, float& s, float& c) { sincosf(v, &s, &c); }
__device__ __forceinline__ void sincos_(double v, double& s, double& c) { sincos(v, &s, &c); }
// 1 / (1 + exp(-v)) without an overflowing exp
template <typename T>
__device__ __forceinline__ T sigmoid_(T v) {
  const T e = exp_(-abs_(v));
  return v >= T(0) ? T(1) / (T(1) + e) : e / (T(1) + e);
}

// ld[b] = v (VCNF_LD_STORE) or ld[b] + v (VCNF_LD_ACCUM)
template <typename T>
__device__ __forceinline__ void put_ld(T* ld, long long b, T v, int mode) {
  ld[b] = mode ? ld[b] + v : v;
}

// The two butterflies differ in rounding and each caller's choice is part of its result: never swap one for the other.
// Ascending: sum over the lanes whose index differs in the bits [from, to) - inside a lane group (1, G) or across the
// groups of a wave (G, 64)
template <typename T>
__device__ __forceinline__ T lanes_sum(T v, int from, int to) {
  for (int m = from; m < to; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Descending: sum over the lanes of a group of G, widest exchange first
template <typename T>
__device__ __forceinline__ T lanes_sum_descending(T v, int G) {
  for (int m = G >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// *dest(e) = sum over the blocks k < groups of partials[k][e] for the n elements e of a block: slice s of a workgroup
// adds its run of blocks in ascending order, the slices are added in ascending order.  Dest maps the flat element
// index to where its sum is stored.
constexpr int kRedEl = 16, kRedSl = 16;       // elements x group slices per workgroup

template <typename T, typename Dest>
__global__ __launch_bounds__(kRedEl * kRedSl) void reduce_partials_kernel(const T* __restrict__ partials, long long groups,
                                                                         long long n, const Dest dest) {
  __shared__ T part[kRedSl][kRedEl];
  const int el = threadIdx.x % kRedEl, sl = threadIdx.x / kRedEl;
  const long long e = (long long)blockIdx.x * kRedEl + el;
  const long long len = (groups + kRedSl - 1) / kRedSl;
  const long long k0 = sl * len, k1 = (k0 + len < groups) ? k0 + len : groups;
  T acc = 0;
  if (e < n)
    for (long long k = k0; k < k1; ++k) acc += partials[k * n + e];
  part[sl][el] = acc;
  __syncthreads();
  if (sl == 0 && e < n) {
    T s = part[0][el];
    for (int k = 1; k < kRedSl; ++k) s += part[k][el];
    *dest(e) = s;
  }
}

// ------------------------------------------------------------------ host side
using vcnf::aligned;          // host_common.hpp
using vcnf::all_aligned;
using vcnf::in_list;
using vcnf::IntList;
using vcnf::launch_listed;
using vcnf::launched;
using vcnf::ok_ld;
using vcnf::with_flags;

// lanes per group for n items (elements or packs)
static inline int pick_lanes(long long n) {
  int G = 1;
  while (G < 64 && G < n) G <<= 1;
  return G;
}

// widest pack (in elements) that divides the rows and that every streamed buffer is aligned to
template <typename T>
static inline int pick_pack(int32_t D, std::initializer_list<const void*> bufs) {
  for (int V = 16 / (int)sizeof(T); V > 1; V >>= 1)
    if (D % V == 0 && all_aligned(bufs, V * sizeof(T))) return V;
  return 1;
}

// launch(std::integral_constant<int, V>{}) for that V, and its status; an 8-byte T has no instance with V = 4
template <typename T, typename F>
static inline int with_pack(int32_t D, std::initializer_list<const void*> bufs, F&& launch) {
  const int V = pick_pack<T>(D, bufs);
  if constexpr (sizeof(T) == 4) {
    if (V == 4) return launch(std::integral_constant<int, 4>{});
  }
  if (V == 2) return launch(std::integral_constant<int, 2>{});
  return launch(std::integral_constant<int, 1>{});
}

// one lane group per item, block / G groups per workgroup, between 1 and max_blocks workgroups
static inline dim3 grid_for(long long groups, int G, int block, long long max_blocks) {
  const long long per_block = block / G;
  long long blocks = (groups + per_block - 1) / per_block;
  if (blocks > max_blocks) blocks = max_blocks;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

template <typename T, typename Dest>
static inline int launch_reduce_partials(const T* partials, long long groups, long long n, Dest dest, void* stream) {
  hipLaunchKernelGGL((reduce_partials_kernel<T, Dest>), dim3((unsigned)((n + kRedEl - 1) / kRedEl)), dim3(kRedEl * kRedSl), 0,
                     (hipStream_t)stream, partials, groups, n, dest);
  return launched();
}

}  // namespace vcnf_stream
