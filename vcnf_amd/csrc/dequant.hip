// Categorical columns for MI355X (gfx950, wave64): the end caps of uniform and variational dequantisation (Ho et al.
// 2019) per column, and the reverse map to integer codes.  Rows x [B, D]; slot [D] int32 gives a column's index c into
// the [B, C] operands, or -1 for a continuous column; levels [C] int32 gives K_c >= 1.  With a = alpha in [0, 1), k the
// row's code in column c (a floating value) and K = T(K_c), every step rounded once in the element type:
//   prepare    s = a/2 + (1 - a) u,  ls = log(s),  lv = log(1 - s),  v = ls - lv
//              ctx = 2 k / (K - 1) - 1   (0 where K = 1)
//              ld = sum_c ((log(1 - a) - ls) - lv)
//   merge      n = 1 / (1 + exp(-w)),  ln = -|w| - 2 log1p(exp(-|w|))        (w is logit noise)
//              n = w,                  ln = 0                                (w is the noise itself)
//              y = (k + n) / K,  s = a/2 + (1 - a) y,  ls = log(s),  lv = log(1 - s),  out = ls - lv
//              ld = sum_c ln + sum_c (((log(1 - a) - log(K)) - ls) - lv)
//   merge_bwd  d_n = ((1 - a) / K) / (s (1 - s)) * (g_out - g_ld (1 - 2 s))
//              d_w = d_n n (1 - n) + g_ld (1 - 2 n)   (logit noise),   d_w = d_n   (the noise itself)
//              d_x = g_out on a continuous column, 0 on a categorical one
//   quantize   t = z[:, col_c],  sg = 1 / (1 + exp(-t)),  y = (sg - a/2) / (1 - a)
//              code = min(max(floor(y K), 0), K - 1)
//              ld = sum_c (((-|t| - 2 log1p(exp(-|t|))) - log(1 - a)) + log(K))
// a/2, 1 - a and log(1 - a) are formed in fp64 and rounded to the element type once, as torch rounds a Python scalar
// operand.  A continuous column of out is the input's, bit for bit.  The VJP recomputes n and s from x and w.
//
// A group of G <= 64 lanes owns a row of D columns, cut into chunks of 16 bytes' worth of elements; lane g owns the chunks
// g, g + G, ... and looks each of its columns up in slot.  The [B, D] buffers move as one 16-byte pack, two 8-byte packs
// or scalars, by what D and the base pointers allow; the [B, C] operands move one element at a time at the slot's
// index.  The sums add a lane's elements in ascending column order and the group sums with the ascending butterfly:
// the access width changes neither which lane owns which element nor the order of a sum, and the unit is compiled
// without contraction into fused multiply-adds, so it never shows in the result bits.  At most kMaxBlocks workgroups
// are started; a lane group takes the rows r, r + trip, ... where trip = rows per workgroup x workgroups is formed on
// the host in 64 bits.  No atomics, nothing random, no allocation.
#include "stream_common.hpp"

#pragma clang fp contract(off)

namespace vcnf_dequant {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 256 * 16;

template <typename T>
struct Consts {
  T half_a, oma, log_oma, ld_sign;          // a/2, 1 - a, log(1 - a)
};

// -|v| - 2 log1p(exp(-|v|)) = logsigmoid(v) + logsigmoid(-v)
template <typename T>
__device__ __forceinline__ T log_sigmoid_pair(T v) {
  const T a = abs_(v);
  return -a - T(2) * log1p_(exp_(-a));
}

// 1 / (1 + exp(-v)): exactly 0 where exp(-v) overflows, exactly 1 where it vanishes beside 1
template <typename T>
__device__ __forceinline__ T sigmoid_plain(T v) {
  return T(1) / (T(1) + exp_(-v));
}

// the first row of this lane's group
__device__ __forceinline__ long long first_row(int lg) {
  return (long long)blockIdx.x * (kBlock >> lg) + (threadIdx.x >> lg);
}

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void prepare_kernel(const T* __restrict__ x, const int32_t* __restrict__ slot,
                                                         const int32_t* __restrict__ levels, const T* __restrict__ u,
                                                         T* __restrict__ v, T* __restrict__ ctx, T* __restrict__ logdet,
                                                         long long rows, long long trip, int D, int C, int lg,
                                                         Consts<T> k, int mode) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  for (long long n = first_row(lg); n < rows; n += trip) {
    const T* xr = x + n * D;
    const long long cr = n * C;
    T acc = 0;
    for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
      const int cnt = D - c < W ? (int)(D - c) : W;
      T vx[W];
      load_chunk<T, V>(vx, xr + c, cnt);
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (j < cnt) {
          const int sl = slot[c + j];
          if (sl >= 0) {
            const T K = T(levels[sl]);
            const T s = k.half_a + k.oma * u[cr + sl];
            const T ls = log_(s), lv = log_(T(1) - s);
            v[cr + sl] = ls - lv;
            ctx[cr + sl] = K > T(1) ? (T(2) * vx[j]) / (K - T(1)) - T(1) : T(0);
            acc += (k.log_oma - ls) - lv;
          }
        }
    }
    acc = lanes_sum(acc, 1, G);
    if (g == 0) put_ld(logdet, n, k.ld_sign * acc, mode);
  }
}

// LOGIT: w is logit noise; else the noise itself
template <typename T, int V, bool LOGIT>
__global__ __launch_bounds__(kBlock) void merge_kernel(const T* __restrict__ x, const int32_t* __restrict__ slot,
                                                       const int32_t* __restrict__ levels, const T* __restrict__ w,
                                                       T* __restrict__ out, T* __restrict__ logdet, long long rows,
                                                       long long trip, int D, int C, int lg, Consts<T> k, int mode) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  for (long long n = first_row(lg); n < rows; n += trip) {
    const T* xr = x + n * D;
    T* orow = out + n * D;
    const long long cr = n * C;
    T acc_n = 0, acc_s = 0;
    for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
      const int cnt = D - c < W ? (int)(D - c) : W;
      T vx[W];
      load_chunk<T, V>(vx, xr + c, cnt);
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (j < cnt) {
          const int sl = slot[c + j];
          if (sl >= 0) {
            const T K = T(levels[sl]);
            T nz = w[cr + sl];
            if constexpr (LOGIT) {
              acc_n += log_sigmoid_pair(nz);
              nz = sigmoid_plain(nz);
            }
            const T y = (vx[j] + nz) / K;
            const T s = k.half_a + k.oma * y;
            const T ls = log_(s), lv = log_(T(1) - s);
            vx[j] = ls - lv;
            acc_s += ((k.log_oma - log_(K)) - ls) - lv;
          }
        }
      store_chunk<T, V>(orow + c, vx, cnt);
    }
    T acc = LOGIT ? acc_n + acc_s : acc_s;
    acc = lanes_sum(acc, 1, G);
    if (g == 0) put_ld(logdet, n, k.ld_sign * acc, mode);
  }
}

// g_out [B, D], g_ld [B] and d_x [B, D] may be NULL
template <typename T, int V, bool LOGIT>
__global__ __launch_bounds__(kBlock) void merge_bwd_kernel(const T* __restrict__ x, const int32_t* __restrict__ slot,
                                                           const int32_t* __restrict__ levels, const T* __restrict__ w,
                                                           const T* __restrict__ g_out, const T* __restrict__ g_ld,
                                                           T* __restrict__ d_w, T* __restrict__ d_x, long long rows,
                                                           long long trip, int D, int C, int lg, Consts<T> k) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  for (long long n = first_row(lg); n < rows; n += trip) {
    const T* xr = x + n * D;
    const long long cr = n * C;
    const T gl = g_ld ? g_ld[n] : T(0);
    for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
      const int cnt = D - c < W ? (int)(D - c) : W;
      T vx[W], vg[W];
      load_chunk<T, V>(vx, xr + c, cnt);
      if (g_out) load_chunk<T, V>(vg, g_out + n * D + c, cnt);
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (j < cnt) {
          const T go = g_out ? vg[j] : T(0);
          const int sl = slot[c + j];
          vg[j] = go;
          if (sl >= 0) {
            const T K = T(levels[sl]);
            const T wv = w[cr + sl];
            const T nz = LOGIT ? sigmoid_plain(wv) : wv;
            const T y = (vx[j] + nz) / K;
            const T s = k.half_a + k.oma * y;
            const T dn = (k.oma / K) / (s * (T(1) - s)) * (go - gl * (T(1) - T(2) * s));
            d_w[cr + sl] = LOGIT ? dn * (nz * (T(1) - nz)) + gl * (T(1) - T(2) * nz) : dn;
            vg[j] = T(0);
          }
        }
      if (d_x) store_chunk<T, V>(d_x + n * D + c, vg, cnt);
    }
  }
}

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void quantize_kernel(const T* __restrict__ z, const int32_t* __restrict__ slot,
                                                          const int32_t* __restrict__ levels, T* __restrict__ out,
                                                          T* __restrict__ logdet, long long rows, long long trip, int D,
                                                          int lg, Consts<T> k, int mode) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  for (long long n = first_row(lg); n < rows; n += trip) {
    const T* zr = z + n * D;
    T* orow = out + n * D;
    T acc = 0;
    for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
      const int cnt = D - c < W ? (int)(D - c) : W;
      T vz[W];
      load_chunk<T, V>(vz, zr + c, cnt);
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (j < cnt) {
          const int sl = slot[c + j];
          if (sl >= 0) {
            const T K = T(levels[sl]);
            const T t = vz[j];
            const T y = (sigmoid_plain(t) - k.half_a) / k.oma;
            const T f = floor(y * K);
            vz[j] = f < T(0) ? T(0) : f > K - T(1) ? K - T(1) : f;          // a NaN stays a NaN
            acc += (log_sigmoid_pair(t) - k.log_oma) + log_(K);
          }
        }
      store_chunk<T, V>(orow + c, vz, cnt);
    }
    acc = lanes_sum(acc, 1, G);
    if (g == 0) put_ld(logdet, n, k.ld_sign * acc, mode);
  }
}

// ------------------------------------------------------------------ host side
static inline bool ok_shape(int64_t rows, int32_t D, int32_t C) {
  return rows >= 0 && D >= 1 && C >= 0 && C <= D && rows <= INT64_MAX / D;
}

// log2 of the lanes per row, the workgroups and the rows of one trip of the whole grid
template <typename T>
static inline void plan(int64_t rows, int32_t D, int& lg, dim3& grid, long long& trip) {
  constexpr int W = chunk_width<T>();
  const int G = pick_lanes(((long long)D + W - 1) / W);
  lg = 0;
  while ((1 << lg) < G) ++lg;
  grid = grid_for(rows, G, kBlock, kMaxBlocks);
  trip = (long long)grid.x * (kBlock / G);
}

template <typename T>
static inline Consts<T> consts(double alpha, T ld_sign) {
  return Consts<T>{(T)(alpha / 2), (T)(1.0 - alpha), (T)log(1.0 - alpha), ld_sign};
}

template <typename T>
static int prepare(const T* x, const int32_t* slot, const int32_t* levels, const T* u, double alpha, T* v, T* ctx,
                   T* logdet, int64_t rows, int32_t D, int32_t C, int ld_mode, T ld_sign, void* stream) {
  if (!x || !slot || !levels || !u || !v || !ctx || !logdet) return VCNF_ERR_NULL;
  if (!ok_shape(rows, D, C)) return VCNF_ERR_SHAPE;
  if (!all_aligned({x, u, v, ctx, logdet}, sizeof(T)) || !all_aligned({slot, levels}, sizeof(int32_t))) return VCNF_ERR_ALIGN;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (rows == 0) return VCNF_OK;
  int lg;
  dim3 grid;
  long long trip;
  plan<T>(rows, D, lg, grid, trip);
  const Consts<T> k = consts<T>(alpha, ld_sign);
  return with_pack<T>(D, {x}, [&](auto V) {
    hipLaunchKernelGGL((prepare_kernel<T, V()>), grid, dim3(kBlock), 0, (hipStream_t)stream, x, slot, levels, u, v, ctx,
                       logdet, (long long)rows, trip, D, C, lg, k, ld_mode);
    return launched();
  });
}

template <typename T>
static int merge(const T* x, const int32_t* slot, const int32_t* levels, const T* w, int noise_is_logit, double alpha,
                 T* out, T* logdet, int64_t rows, int32_t D, int32_t C, int ld_mode, T ld_sign, void* stream) {
  if (!x || !slot || !levels || !w || !out || !logdet) return VCNF_ERR_NULL;
  if (!ok_shape(rows, D, C)) return VCNF_ERR_SHAPE;
  if (!all_aligned({x, w, out, logdet}, sizeof(T)) || !all_aligned({slot, levels}, sizeof(int32_t))) return VCNF_ERR_ALIGN;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (rows == 0) return VCNF_OK;
  int lg;
  dim3 grid;
  long long trip;
  plan<T>(rows, D, lg, grid, trip);
  const Consts<T> k = consts<T>(alpha, ld_sign);
  return with_pack<T>(D, {x, out}, [&](auto V) {
    return with_flags([&](auto LOGIT) {
      hipLaunchKernelGGL((merge_kernel<T, V(), LOGIT()>), grid, dim3(kBlock), 0, (hipStream_t)stream, x, slot, levels, w,
                         out, logdet, (long long)rows, trip, D, C, lg, k, ld_mode);
      return launched();
    }, noise_is_logit != 0);
  });
}

template <typename T>
static int merge_bwd(const T* x, const int32_t* slot, const int32_t* levels, const T* w, int noise_is_logit, double alpha,
                     const T* g_out, const T* g_ld, T* d_w, T* d_x, int64_t rows, int32_t D, int32_t C, void* stream) {
  if (!x || !slot || !levels || !w || !d_w) return VCNF_ERR_NULL;
  if (!ok_shape(rows, D, C)) return VCNF_ERR_SHAPE;
  if (!all_aligned({x, w, g_out, g_ld, d_w, d_x}, sizeof(T)) || !all_aligned({slot, levels}, sizeof(int32_t)))
    return VCNF_ERR_ALIGN;
  if (rows == 0) return VCNF_OK;
  int lg;
  dim3 grid;
  long long trip;
  plan<T>(rows, D, lg, grid, trip);
  const Consts<T> k = consts<T>(alpha, T(1));
  return with_pack<T>(D, {x, g_out, d_x}, [&](auto V) {
    return with_flags([&](auto LOGIT) {
      hipLaunchKernelGGL((merge_bwd_kernel<T, V(), LOGIT()>), grid, dim3(kBlock), 0, (hipStream_t)stream, x, slot, levels,
                         w, g_out, g_ld, d_w, d_x, (long long)rows, trip, D, C, lg, k);
      return launched();
    }, noise_is_logit != 0);
  });
}

template <typename T>
static int quantize(const T* z, const int32_t* slot, const int32_t* levels, double alpha, T* out, T* logdet, int64_t rows,
                    int32_t D, int32_t C, int ld_mode, T ld_sign, void* stream) {
  if (!z || !slot || !levels || !out || !logdet) return VCNF_ERR_NULL;
  if (!ok_shape(rows, D, C)) return VCNF_ERR_SHAPE;
  if (!all_aligned({z, out, logdet}, sizeof(T)) || !all_aligned({slot, levels}, sizeof(int32_t))) return VCNF_ERR_ALIGN;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (rows == 0) return VCNF_OK;
  int lg;
  dim3 grid;
  long long trip;
  plan<T>(rows, D, lg, grid, trip);
  const Consts<T> k = consts<T>(alpha, ld_sign);
  return with_pack<T>(D, {z, out}, [&](auto V) {
    hipLaunchKernelGGL((quantize_kernel<T, V()>), grid, dim3(kBlock), 0, (hipStream_t)stream, z, slot, levels, out, logdet,
                       (long long)rows, trip, D, lg, k, ld_mode);
    return launched();
  });
}

}  // namespace vcnf_dequant

#define VCNF_DEQUANT_ENTRY_POINTS(T, SFX)                                                                              \
  extern "C" int vcnf_dequant_prepare_##SFX(const T* x, const int32_t* slot, const int32_t* levels, const T* u,        \
                                            double alpha, T* v, T* ctx, T* logdet, int64_t batch, int32_t features,    \
                                            int32_t n_cat, int ld_mode, T ld_sign, void* stream) {                     \
    return vcnf_dequant::prepare<T>(x, slot, levels, u, alpha, v, ctx, logdet, batch, features, n_cat, ld_mode,        \
                                    ld_sign, stream);                                                                  \
  }                                                                                                                    \
  extern "C" int vcnf_dequant_merge_##SFX(const T* x, const int32_t* slot, const int32_t* levels, const T* w,          \
                                          int noise_is_logit, double alpha, T* out, T* logdet, int64_t batch,          \
                                          int32_t features, int32_t n_cat, int ld_mode, T ld_sign, void* stream) {     \
    return vcnf_dequant::merge<T>(x, slot, levels, w, noise_is_logit, alpha, out, logdet, batch, features, n_cat,      \
                                  ld_mode, ld_sign, stream);                                                           \
  }                                                                                                                    \
  extern "C" int vcnf_dequant_merge_bwd_##SFX(const T* x, const int32_t* slot, const int32_t* levels, const T* w,      \
                                              int noise_is_logit, double alpha, const T* g_out, const T* g_ld, T* d_w, \
                                              T* d_x, int64_t batch, int32_t features, int32_t n_cat, void* stream) {  \
    return vcnf_dequant::merge_bwd<T>(x, slot, levels, w, noise_is_logit, alpha, g_out, g_ld, d_w, d_x, batch,         \
                                      features, n_cat, stream);                                                        \
  }                                                                                                                    \
  extern "C" int vcnf_quantize_##SFX(const T* z, const int32_t* slot, const int32_t* levels, double alpha, T* out,     \
                                     T* logdet, int64_t batch, int32_t features, int32_t n_cat, int ld_mode,           \
                                     T ld_sign, void* stream) {                                                        \
    return vcnf_dequant::quantize<T>(z, slot, levels, alpha, out, logdet, batch, features, n_cat, ld_mode, ld_sign,    \
                                     stream);                                                                          \
  }

VCNF_DEQUANT_ENTRY_POINTS(float, f32)
VCNF_DEQUANT_ENTRY_POINTS(double, f64)
