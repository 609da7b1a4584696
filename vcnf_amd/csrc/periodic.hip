// Circular flows for MI355X (gfx950, wave64): the periodic maps of normflow 1.2's flows/periodic.py (PeriodicWrap,
// PeriodicShift) and its UniformGaussian base (distributions/base.py).  Rows of D = features contiguous columns.
//   periodic        out = z on a column with half[j] == 0; elsewhere, with bound = half[j] and s = sign shift[j] (0
//                   without a shift table), each step rounded once in the element type:
//                     a = (z + s) + bound,  r = fmod(a, 2 bound),  r += 2 bound where r < 0,  out = r - bound
//                   which is torch.remainder(z + s + bound, 2 bound) - bound to the bit
//   log_prob        logp = const_term - 1/2 sum_j (z inv_scale_g[j])^2, inv_scale_g 0 on a uniform column
//   sample          z = scale[j] (eps[src[j]] - offset[j]) and the log_prob of that z
//   log_prob_bwd    d_z = -g z inv_scale_g[j]^2
//
// A group of G <= 64 lanes owns a row.  The row is cut into chunks of 16 bytes' worth of columns and lane g owns the
// chunks g, g + G, ...; the sums add a lane's columns in ascending order and the group sums with the ascending
// butterfly.  How a chunk moves - one 16-byte pack, two 8-byte packs or scalars, by what D and the base pointers allow
// - changes neither which lane owns which column nor the order of a sum, and the unit is compiled without contraction
// into fused multiply-adds: the access width never shows in the result bits.  A lane reads its chunk of z before it
// writes the same chunk of out and no other lane touches it, so out may be z.
// The grids are sized to the work and no kernel loops over the grid: the row index is formed in 64 bits from the
// workgroup index, and a shape that would need more than 2^31 - 1 workgroups is refused.  The per-column tables are a
// few hundred bytes read by every row: they stay in the cache and nothing is staged in LDS.
#include "stream_common.hpp"

#pragma clang fp contract(off)

namespace vcnf_periodic {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr long long kMaxGrid = 2147483647LL;

__device__ __forceinline__ float fmod_(float a, float b) { return fmodf(a, b); }
__device__ __forceinline__ double fmod_(double a, double b) { return fmod(a, b); }

// the row of this lane's group, or -1 past the last row (whole groups leave: a butterfly stays inside a group)
__device__ __forceinline__ long long group_row(int lg, long long rows) {
  const long long n = (long long)blockIdx.x * (kBlock >> lg) + (threadIdx.x >> lg);
  return n < rows ? n : -1;
}

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void periodic_kernel(const T* z, const T* __restrict__ half,
                                                          const T* __restrict__ shift, T* out, long long rows, int D,
                                                          int lg, T sign) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  const long long n = group_row(lg, rows);
  if (n < 0) return;
  const T* zr = z + n * D;
  T* outr = out + n * D;
  for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
    const int cnt = D - c < W ? (int)(D - c) : W;
    T vz[W], vh[W], vs[W];
    load_chunk<T, V>(vz, zr + c, cnt);
    load_chunk<T, V>(vh, half + c, cnt);
    if (shift) load_chunk<T, V>(vs, shift + c, cnt);
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < cnt && vh[j] != T(0)) {
        const T bound = vh[j], period = T(2) * bound;
        const T s = shift ? sign * vs[j] : T(0);
        const T a = (vz[j] + s) + bound;
        T r = fmod_(a, period);
        if (r != T(0) && r < T(0)) r += period;
        vz[j] = r - bound;
      }
    store_chunk<T, V>(outr + c, vz, cnt);
  }
}

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void ug_log_prob_kernel(const T* __restrict__ z, const T* __restrict__ inv,
                                                             T* __restrict__ logp, long long rows, int D, int lg, T cst,
                                                             int mode) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  const long long n = group_row(lg, rows);
  if (n < 0) return;
  const T* __restrict__ zr = z + n * D;
  T s = 0;
  for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
    const int cnt = D - c < W ? (int)(D - c) : W;
    T vz[W], vi[W];
    load_chunk<T, V>(vz, zr + c, cnt);
    load_chunk<T, V>(vi, inv + c, cnt);
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < cnt) {
        const T u = vz[j] * vi[j];
        s += u * u;
      }
  }
  s = lanes_sum(s, 1, G);
  if (g == 0) put_ld(logp, n, cst - T(0.5) * s, mode);
}

// eps is gathered through src, one element at a time; a src outside the row gives NaN, never a read beyond it
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void ug_sample_kernel(const T* __restrict__ eps, const int32_t* __restrict__ src,
                                                           const T* __restrict__ offset, const T* __restrict__ scale,
                                                           const T* __restrict__ inv, T* __restrict__ z,
                                                           T* __restrict__ logp, long long rows, int D, int lg, T cst) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  const long long n = group_row(lg, rows);
  if (n < 0) return;
  const T* __restrict__ er = eps + n * D;
  T* __restrict__ zr = z + n * D;
  T s = 0;
  for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
    const int cnt = D - c < W ? (int)(D - c) : W;
    T vz[W], vo[W], vc[W], vi[W];
    load_chunk<T, V>(vo, offset + c, cnt);
    load_chunk<T, V>(vc, scale + c, cnt);
    load_chunk<T, V>(vi, inv + c, cnt);
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < cnt) {
        const uint32_t from = (uint32_t)src[c + j];
        const T e = from < (uint32_t)D ? er[from] : T(NAN);
        vz[j] = vc[j] * (e - vo[j]);
        const T u = vz[j] * vi[j];
        s += u * u;
      }
    store_chunk<T, V>(zr + c, vz, cnt);
  }
  s = lanes_sum(s, 1, G);
  if (g == 0) logp[n] = cst - T(0.5) * s;
}

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void ug_log_prob_bwd_kernel(const T* __restrict__ z, const T* __restrict__ inv,
                                                                 const T* __restrict__ g_lp, T* __restrict__ d_z,
                                                                 long long rows, int D, int lg) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  const long long n = group_row(lg, rows);
  if (n < 0) return;
  const T* __restrict__ zr = z + n * D;
  T* __restrict__ dr = d_z + n * D;
  const T minus_g = -g_lp[n];
  for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
    const int cnt = D - c < W ? (int)(D - c) : W;
    T vz[W], vi[W];
    load_chunk<T, V>(vz, zr + c, cnt);
    load_chunk<T, V>(vi, inv + c, cnt);
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < cnt) vz[j] = (minus_g * vz[j]) * (vi[j] * vi[j]);
    store_chunk<T, V>(dr + c, vz, cnt);
  }
}

// ------------------------------------------------------------------ host side
static inline bool ok_rows(int64_t rows, int32_t D) { return rows >= 0 && D >= 1 && rows <= INT64_MAX / D; }

// log2 of the lanes per row and the workgroups for `rows` rows of D columns; false when they exceed a grid
template <typename T>
static inline bool plan(int64_t rows, int32_t D, int& lg, long long& blocks) {
  constexpr int W = chunk_width<T>();
  const int G = pick_lanes(((long long)D + W - 1) / W);
  lg = 0;
  while ((1 << lg) < G) ++lg;
  const long long per_block = kBlock / G;
  blocks = (rows + per_block - 1) / per_block;
  return blocks <= kMaxGrid;
}

template <typename T>
static int periodic(const T* z, const T* half, const T* shift, T* out, int64_t rows, int32_t D, T sign, void* stream) {
  if (!z || !half || !out) return VCNF_ERR_NULL;
  int lg;
  long long blocks;
  if (!ok_rows(rows, D) || !plan<T>(rows, D, lg, blocks)) return VCNF_ERR_SHAPE;
  if (rows == 0) return VCNF_OK;
  if (!all_aligned({z, half, shift, out}, sizeof(T))) return VCNF_ERR_ALIGN;
  return with_pack<T>(D, {z, half, shift, out}, [&](auto V) {
    hipLaunchKernelGGL((periodic_kernel<T, V()>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, z, half,
                       shift, out, (long long)rows, D, lg, sign);
    return launched();
  });
}

template <typename T>
static int log_prob(const T* z, const T* inv, T cst, T* logp, int64_t rows, int32_t D, int ld_mode, void* stream) {
  if (!z || !inv || !logp) return VCNF_ERR_NULL;
  int lg;
  long long blocks;
  if (!ok_rows(rows, D) || !plan<T>(rows, D, lg, blocks)) return VCNF_ERR_SHAPE;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (rows == 0) return VCNF_OK;
  if (!all_aligned({z, inv, logp}, sizeof(T))) return VCNF_ERR_ALIGN;
  return with_pack<T>(D, {z, inv}, [&](auto V) {
    hipLaunchKernelGGL((ug_log_prob_kernel<T, V()>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, z, inv,
                       logp, (long long)rows, D, lg, cst, ld_mode);
    return launched();
  });
}

template <typename T>
static int sample(const T* eps, const int32_t* src, const T* offset, const T* scale, T cst, const T* inv, T* z, T* logp,
                  int64_t rows, int32_t D, void* stream) {
  if (!eps || !src || !offset || !scale || !inv || !z || !logp) return VCNF_ERR_NULL;
  int lg;
  long long blocks;
  if (!ok_rows(rows, D) || !plan<T>(rows, D, lg, blocks)) return VCNF_ERR_SHAPE;
  if (rows == 0) return VCNF_OK;
  if (!all_aligned({eps, offset, scale, inv, z, logp}, sizeof(T)) || !aligned(src, sizeof(int32_t))) return VCNF_ERR_ALIGN;
  return with_pack<T>(D, {offset, scale, inv, z}, [&](auto V) {
    hipLaunchKernelGGL((ug_sample_kernel<T, V()>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, eps, src,
                       offset, scale, inv, z, logp, (long long)rows, D, lg, cst);
    return launched();
  });
}

template <typename T>
static int log_prob_bwd(const T* z, const T* inv, const T* g, T* d_z, int64_t rows, int32_t D, void* stream) {
  if (!z || !inv || !g || !d_z) return VCNF_ERR_NULL;
  int lg;
  long long blocks;
  if (!ok_rows(rows, D) || !plan<T>(rows, D, lg, blocks)) return VCNF_ERR_SHAPE;
  if (rows == 0) return VCNF_OK;
  if (!all_aligned({z, inv, g, d_z}, sizeof(T))) return VCNF_ERR_ALIGN;
  return with_pack<T>(D, {z, inv, d_z}, [&](auto V) {
    hipLaunchKernelGGL((ug_log_prob_bwd_kernel<T, V()>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, z,
                       inv, g, d_z, (long long)rows, D, lg);
    return launched();
  });
}

}  // namespace vcnf_periodic

#define VCNF_PERIODIC_ENTRY_POINTS(T, SFX)                                                                             \
  extern "C" int vcnf_periodic_##SFX(const T* z, const T* half, const T* shift, T* out, int64_t n_rows,                \
                                     int32_t features, T sign, void* stream) {                                         \
    return vcnf_periodic::periodic<T>(z, half, shift, out, n_rows, features, sign, stream);                            \
  }                                                                                                                    \
  extern "C" int vcnf_uniform_gaussian_log_prob_##SFX(const T* z, const T* inv_scale_g, T const_term, T* logp,         \
                                                      int64_t batch, int32_t features, int ld_mode, void* stream) {    \
    return vcnf_periodic::log_prob<T>(z, inv_scale_g, const_term, logp, batch, features, ld_mode, stream);             \
  }                                                                                                                    \
  extern "C" int vcnf_uniform_gaussian_sample_##SFX(const T* eps, const int32_t* src, const T* offset, const T* scale, \
                                                    T const_term, const T* inv_scale_g, T* z, T* logp, int64_t batch,  \
                                                    int32_t features, void* stream) {                                  \
    return vcnf_periodic::sample<T>(eps, src, offset, scale, const_term, inv_scale_g, z, logp, batch, features,        \
                                    stream);                                                                           \
  }                                                                                                                    \
  extern "C" int vcnf_uniform_gaussian_log_prob_bwd_##SFX(const T* z, const T* inv_scale_g, const T* g, T* d_z,        \
                                                          int64_t batch, int32_t features, void* stream) {             \
    return vcnf_periodic::log_prob_bwd<T>(z, inv_scale_g, g, d_z, batch, features, stream);                            \
  }

VCNF_PERIODIC_ENTRY_POINTS(float, f32)
VCNF_PERIODIC_ENTRY_POINTS(double, f64)
