// Image data end caps for MI355X (gfx950, wave64): the Logit transform of normflow 1.2's transforms.py and the byte
// ingest in front of it.  Rows of D = features contiguous elements (all axes of an item but the first), alpha in
// [0, 0.5), beta = 1 - 2 alpha, every step rounded once in the element type:
//   inverse      u = alpha + beta x (a multiply, then an add),  lu = log(u),  lv = log(1 - u),  z = lu - lv
//                log_det = (D log(beta) - sum lu) - sum lv
//   forward      s = sigmoid(z),  y = (s - alpha) / beta
//                log_det = -D log(beta) + sum (-|z| - 2 log1p(exp(-|z|)))     (= logsigmoid(z) + logsigmoid(-z))
//   inverse_u8   x = ((T(byte) / 255) + noise * jitter) * scale, then as inverse: bytes are read, x is never stored
//   inverse_bwd  d_x = beta / (u (1 - u)) * (g_z - g_ld (1 - 2 u))
//   forward_bwd  d_z = g_y * (s (1 - s) / beta) + g_ld (1 - 2 s)
// The VJPs recompute u or s from the saved input; a NULL cotangent drops its term.
//
// A group of G <= 64 lanes owns a row.  The row is cut into chunks of 16 bytes' worth of elements and lane g owns the
// chunks g, g + G, ...; the sums add a lane's elements in ascending order and the group sums with the ascending
// butterfly.  How a chunk moves - one 16-byte pack, two 8-byte packs or scalars (bytes: 4, 2 or 1 per access), by what D
// and the base pointers allow - changes neither which lane owns which element nor the order of a sum, and the unit is
// compiled without contraction into fused multiply-adds: the access width never shows in the result bits.  A lane reads
// its chunk before it writes the same chunk of the output and no other lane touches it, so the output may be the input.
// The grids are sized to the work and no kernel loops over the grid: the row index is formed in 64 bits from the
// workgroup index, and a shape that would need more than 2^31 - 1 workgroups is refused.
#include "stream_common.hpp"

#pragma clang fp contract(off)

namespace vcnf_logit {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr long long kMaxGrid = 2147483647LL;

// the row of this lane's group, or -1 past the last row (whole groups leave: a butterfly stays inside a group)
__device__ __forceinline__ long long group_row(int lg, long long rows) {
  const long long n = (long long)blockIdx.x * (kBlock >> lg) + (threadIdx.x >> lg);
  return n < rows ? n : -1;
}

// the first cnt bytes of the chunk at src (cnt a multiple of V) in accesses of V bytes, as elements
template <typename T, int V>
__device__ __forceinline__ void load_bytes(T* d, const uint8_t* __restrict__ src, int cnt) {
  constexpr int W = chunk_width<T>();
#pragma unroll
  for (int k = 0; k < W / V; ++k)
    if (k * V < cnt) {
      const Pack<uint8_t, V> q = *reinterpret_cast<const Pack<uint8_t, V>*>(src + k * V);
#pragma unroll
      for (int j = 0; j < V; ++j) d[k * V + j] = T(q.v[j]);
    }
}

// alpha, beta and the constant of the log-det (D log(beta), negated for the sampling direction), in the element type
template <typename T>
struct Consts {
  T alpha, beta, cst, ld_sign;
};

// x [rows, D] (or bytes and noise, U8) -> z and the row's log-det
template <typename T, int V, bool U8>
__global__ __launch_bounds__(kBlock) void inverse_kernel(const T* x, const uint8_t* __restrict__ bytes, T jitter, T scale,
                                                         T* z, T* __restrict__ logdet, long long rows, int D, int lg,
                                                         Consts<T> k, int mode) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  const long long n = group_row(lg, rows);
  if (n < 0) return;
  const T* xr = x + n * D;          // U8: the noise
  T* zr = z + n * D;
  T su = 0, sv = 0;
  for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
    const int cnt = D - c < W ? (int)(D - c) : W;
    T vx[W], vb[W];
    load_chunk<T, V>(vx, xr + c, cnt);
    if constexpr (U8) load_bytes<T, V>(vb, bytes + n * D + c, cnt);
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < cnt) {
        T v = vx[j];
        if constexpr (U8) v = ((vb[j] / T(255)) + v * jitter) * scale;
        const T u = k.alpha + k.beta * v;
        const T lu = log_(u), lv = log_(T(1) - u);
        vx[j] = lu - lv;
        su += lu;
        sv += lv;
      }
    store_chunk<T, V>(zr + c, vx, cnt);
  }
  su = lanes_sum(su, 1, G);
  sv = lanes_sum(sv, 1, G);
  if (g == 0) put_ld(logdet, n, k.ld_sign * ((k.cst - su) - sv), mode);
}

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void forward_kernel(const T* z, T* y, T* __restrict__ logdet, long long rows, int D,
                                                         int lg, Consts<T> k, int mode) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  const long long n = group_row(lg, rows);
  if (n < 0) return;
  const T* zr = z + n * D;
  T* yr = y + n * D;
  T acc = 0;
  for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
    const int cnt = D - c < W ? (int)(D - c) : W;
    T vz[W];
    load_chunk<T, V>(vz, zr + c, cnt);
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < cnt) {
        const T a = abs_(vz[j]), e = exp_(-a);
        const T s = (vz[j] >= T(0) ? T(1) : e) / (T(1) + e);          // sigmoid_ with its one division stated once
        acc += -a - T(2) * log1p_(e);
        vz[j] = (s - k.alpha) / k.beta;
      }
    store_chunk<T, V>(yr + c, vz, cnt);
  }
  acc = lanes_sum(acc, 1, G);
  if (g == 0) put_ld(logdet, n, k.ld_sign * (k.cst + acc), mode);
}

// FWD: the VJP of forward from z; else the VJP of inverse from x.  g_out / g_ld may be NULL
template <typename T, int V, bool FWD>
__global__ __launch_bounds__(kBlock) void bwd_kernel(const T* __restrict__ in, const T* __restrict__ g_out,
                                                     const T* __restrict__ g_ld, T* __restrict__ d_in, long long rows,
                                                     int D, int lg, Consts<T> k) {
  constexpr int W = chunk_width<T>();
  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  const long long n = group_row(lg, rows);
  if (n < 0) return;
  const T* __restrict__ ir = in + n * D;
  T* __restrict__ dr = d_in + n * D;
  const T gl = g_ld ? g_ld[n] : T(0);
  for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
    const int cnt = D - c < W ? (int)(D - c) : W;
    T vi[W], vg[W];
    load_chunk<T, V>(vi, ir + c, cnt);
    if (g_out) load_chunk<T, V>(vg, g_out + n * D + c, cnt);
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < cnt) {
        const T go = g_out ? vg[j] : T(0);
        if (FWD) {
          const T s = sigmoid_(vi[j]);
          vi[j] = go * (s * (T(1) - s) / k.beta) + gl * (T(1) - T(2) * s);
        } else {
          const T u = k.alpha + k.beta * vi[j];
          vi[j] = k.beta / (u * (T(1) - u)) * (go - gl * (T(1) - T(2) * u));
        }
      }
    store_chunk<T, V>(dr + c, vi, cnt);
  }
}

// ------------------------------------------------------------------ host side
static inline bool ok_rows(int64_t rows, int32_t D) { return rows >= 0 && D >= 1 && rows <= INT64_MAX / D; }

// log2 of the lanes per row and the workgroups for `rows` rows of D elements; false when they exceed a grid
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

// alpha and beta = 1 - 2 alpha are rounded to the element type from fp64 once, as torch rounds a Python scalar operand
template <typename T>
static inline Consts<T> consts(double alpha, int32_t D, bool sampling, T ld_sign) {
  const double beta = 1.0 - 2.0 * alpha, c = (double)D * log(beta);
  return Consts<T>{(T)alpha, (T)beta, (T)(sampling ? -c : c), ld_sign};
}

template <typename T>
static int inverse(const T* x, const uint8_t* bytes, double jitter, double scale, double alpha, T* z, T* logdet,
                   int64_t rows, int32_t D, int ld_mode, T ld_sign, bool u8, void* stream) {
  if (!x || !z || !logdet || (u8 && !bytes)) return VCNF_ERR_NULL;
  int lg;
  long long blocks;
  if (!ok_rows(rows, D) || !plan<T>(rows, D, lg, blocks)) return VCNF_ERR_SHAPE;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (rows == 0) return VCNF_OK;
  if (!all_aligned({x, z, logdet}, sizeof(T))) return VCNF_ERR_ALIGN;
  const Consts<T> k = consts<T>(alpha, D, false, ld_sign);
  // bytes ride in accesses of V bytes where the elements ride in packs of V; their base is held to the packs' alignment
  return with_pack<T>(D, {x, z, u8 ? (const void*)bytes : (const void*)x}, [&](auto V) {
    if (u8)
      hipLaunchKernelGGL((inverse_kernel<T, V(), true>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, x,
                         bytes, (T)jitter, (T)scale, z, logdet, (long long)rows, D, lg, k, ld_mode);
    else
      hipLaunchKernelGGL((inverse_kernel<T, V(), false>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, x,
                         bytes, T(0), T(0), z, logdet, (long long)rows, D, lg, k, ld_mode);
    return launched();
  });
}

template <typename T>
static int forward(const T* z, double alpha, T* y, T* logdet, int64_t rows, int32_t D, int ld_mode, T ld_sign,
                   void* stream) {
  if (!z || !y || !logdet) return VCNF_ERR_NULL;
  int lg;
  long long blocks;
  if (!ok_rows(rows, D) || !plan<T>(rows, D, lg, blocks)) return VCNF_ERR_SHAPE;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (rows == 0) return VCNF_OK;
  if (!all_aligned({z, y, logdet}, sizeof(T))) return VCNF_ERR_ALIGN;
  const Consts<T> k = consts<T>(alpha, D, true, ld_sign);
  return with_pack<T>(D, {z, y}, [&](auto V) {
    hipLaunchKernelGGL((forward_kernel<T, V()>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, z, y,
                       logdet, (long long)rows, D, lg, k, ld_mode);
    return launched();
  });
}

template <typename T, bool FWD>
static int bwd(const T* in, double alpha, const T* g_out, const T* g_ld, T* d_in, int64_t rows, int32_t D, void* stream) {
  if (!in || !d_in) return VCNF_ERR_NULL;
  int lg;
  long long blocks;
  if (!ok_rows(rows, D) || !plan<T>(rows, D, lg, blocks)) return VCNF_ERR_SHAPE;
  if (rows == 0) return VCNF_OK;
  if (!all_aligned({in, g_out, g_ld, d_in}, sizeof(T))) return VCNF_ERR_ALIGN;
  const Consts<T> k = consts<T>(alpha, D, FWD, T(1));
  return with_pack<T>(D, {in, g_out, d_in}, [&](auto V) {
    hipLaunchKernelGGL((bwd_kernel<T, V(), FWD>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, in, g_out,
                       g_ld, d_in, (long long)rows, D, lg, k);
    return launched();
  });
}

}  // namespace vcnf_logit

#define VCNF_LOGIT_ENTRY_POINTS(T, SFX)                                                                                \
  extern "C" int vcnf_logit_inverse_##SFX(const T* x, double alpha, T* z, T* logdet, int64_t batch, int32_t features,  \
                                          int ld_mode, T ld_sign, void* stream) {                                      \
    return vcnf_logit::inverse<T>(x, nullptr, 0.0, 0.0, alpha, z, logdet, batch, features, ld_mode, ld_sign, false,    \
                                  stream);                                                                             \
  }                                                                                                                    \
  extern "C" int vcnf_logit_forward_##SFX(const T* z, double alpha, T* y, T* logdet, int64_t batch, int32_t features,  \
                                          int ld_mode, T ld_sign, void* stream) {                                      \
    return vcnf_logit::forward<T>(z, alpha, y, logdet, batch, features, ld_mode, ld_sign, stream);                     \
  }                                                                                                                    \
  extern "C" int vcnf_logit_inverse_bwd_##SFX(const T* x, double alpha, const T* g_z, const T* g_ld, T* d_x,           \
                                              int64_t batch, int32_t features, void* stream) {                         \
    return vcnf_logit::bwd<T, false>(x, alpha, g_z, g_ld, d_x, batch, features, stream);                               \
  }                                                                                                                    \
  extern "C" int vcnf_logit_forward_bwd_##SFX(const T* z, double alpha, const T* g_y, const T* g_ld, T* d_z,           \
                                              int64_t batch, int32_t features, void* stream) {                         \
    return vcnf_logit::bwd<T, true>(z, alpha, g_y, g_ld, d_z, batch, features, stream);                                \
  }                                                                                                                    \
  extern "C" int vcnf_logit_inverse_u8_##SFX(const uint8_t* bytes, const T* noise, double jitter, double scale,        \
                                             double alpha, T* z, T* logdet, int64_t batch, int32_t features,           \
                                             int ld_mode, T ld_sign, void* stream) {                                   \
    return vcnf_logit::inverse<T>(noise, bytes, jitter, scale, alpha, z, logdet, batch, features, ld_mode, ld_sign,    \
                                  true, stream);                                                                       \
  }

VCNF_LOGIT_ENTRY_POINTS(float, f32)
VCNF_LOGIT_ENTRY_POINTS(double, f64)
