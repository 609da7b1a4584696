// End caps of the flow VAE for MI355X (gfx950, wave64): the amortised Gaussian encoder and the Gaussian / Bernoulli
// decoders of NormalizingFlowVAE.  N = B S rows of D columns; row n belongs to data item n / S, and what the S rows of
// an item share (the net's output for the item, or the data) is read through that division, never repeated in memory.
// A parameter row is h = [mean (D) | lv (D)], 2 D contiguous values (lv = log variance).
//   encode          z = mean + exp(lv / 2) eps,   logq = -D/2 log 2 pi - sum_j (lv / 2 + eps^2 / 2)
//   gauss_log_prob  logp = -D/2 log 2 pi - 1/2 sum_j (lv + (v - mean)^2 exp(-lv))
//   bernoulli       logp = sum_j (x ls(a) + (1 - x) ls(-a)),   ls(a) = -max(-a, 0) - log1p(exp(-|a|))
//
// Forward: a group of G <= 64 lanes owns a row.  The row is cut into chunks of 16 bytes' worth of columns and lane g
// owns the chunks g, g + G, ...; it adds its columns in ascending order and the group sums with the ascending
// butterfly.  How a chunk is loaded - one 16-byte pack, two 8-byte packs or scalars, by what D and the base pointers
// allow - does not change which lane adds which column in which order, and the unit is compiled without contraction
// into fused multiply-adds: the access width never shows in the result bits.
// VJPs: a lane owns one (item, column) and walks the item's S rows in ascending order.  The gradient of the per-row
// operand is written at each step, the gradient of the shared operand is kept in a register and written once: a
// fixed-order sum without atomics or workspace.
// The grids are sized to the work and no kernel loops over the grid: the row (element) index is formed in 64 bits from
// the workgroup index, and a shape that would need more than 2^31 - 1 workgroups is refused.
#include "stream_common.hpp"

#pragma clang fp contract(off)

namespace vcnf_vae {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr long long kMaxGrid = 2147483647LL;
constexpr double kLog2Pi = 1.8378770664093454835606594728112353;

enum { ENCODE = 0, GAUSS = 1, BERNOULLI = 2 };

// ------------------------------------------------------------------ forward
// ENCODE:    a = eps [N, D] (a_div 1),  h [N / h_div, 2 D],  z [N, D],  out = logq
// GAUSS:     a = v [N / a_div, D],      h [N / h_div, 2 D],             out = logp
// BERNOULLI: a = score [N, D] (a_div 1), h = x [N / h_div, D],          out = logp
template <typename T>
struct FwdArgs {
  const T *a, *h;
  T *z, *out;
  long long N;
  int a_div, h_div, D, G;
  T cst;                    // -D/2 log 2 pi
};

template <typename T, int V, int OP>
__global__ __launch_bounds__(kBlock) void vae_fwd_kernel(const FwdArgs<T> p) {
  constexpr int W = chunk_width<T>();
  const int D = p.D, G = p.G, g = threadIdx.x & (G - 1), per_block = kBlock / G;
  const long long n = (long long)blockIdx.x * per_block + threadIdx.x / G;
  if (n >= p.N) return;                               // whole lane groups leave: the butterfly stays inside a group
  const T* __restrict__ a = p.a + (p.a_div == 1 ? n : n / p.a_div) * D;
  const T* __restrict__ h = p.h + (p.h_div == 1 ? n : n / p.h_div) * (OP == BERNOULLI ? (long long)D : 2LL * D);
  T* __restrict__ z = OP == ENCODE ? p.z + n * D : nullptr;
  T s = 0;
  for (long long c = (long long)g * W; c < D; c += (long long)G * W) {
    const int cnt = D - c < W ? (int)(D - c) : W;
    T va[W], vm[W], vl[W], vz[W];
    load_chunk<T, V>(va, a + c, cnt);
    load_chunk<T, V>(vm, h + c, cnt);
    if (OP != BERNOULLI) load_chunk<T, V>(vl, h + D + c, cnt);
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < cnt) {
        if (OP == ENCODE) {
          vz[j] = vm[j] + exp_(T(0.5) * vl[j]) * va[j];
          s += T(0.5) * vl[j] + T(0.5) * (va[j] * va[j]);
        } else if (OP == GAUSS) {
          const T d = va[j] - vm[j];
          s += vl[j] + d * d * exp_(-vl[j]);
        } else {
          const T sc = va[j], x = vm[j];
          const T t = log1p_(exp_(-abs_(sc)));
          const T lpos = -(sc < T(0) ? -sc : T(0)) - t, lneg = -(sc > T(0) ? sc : T(0)) - t;
          s += x * lpos + (T(1) - x) * lneg;
        }
      }
    if (OP == ENCODE) store_chunk<T, V>(z + c, vz, cnt);
  }
  s = lanes_sum(s, 1, G);
  if (g == 0) p.out[n] = OP == ENCODE ? p.cst - s : OP == GAUSS ? p.cst - T(0.5) * s : s;
}

// ------------------------------------------------------------------ the VJPs: lane t owns item b = t / D, column t % D
template <typename T>
__global__ __launch_bounds__(kBlock) void vae_encode_bwd_kernel(const T* __restrict__ h, const T* __restrict__ eps,
                                                                const T* __restrict__ g_z, const T* __restrict__ g_lq,
                                                                T* __restrict__ d_h, long long B, int S, int D) {
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= B * D) return;
  const long long b = t / D, j = t - b * D;
  const T half_sd = T(0.5) * exp_(T(0.5) * h[b * 2 * D + D + j]);
  T dm = 0, dl = 0;
  for (long long n = b * S; n < (b + 1) * S; ++n) {
    T term = 0;
    if (g_z) {
      const T gz = g_z[n * D + j];
      dm += gz;
      term = half_sd * eps[n * D + j] * gz;
    }
    dl += term - T(0.5) * (g_lq ? g_lq[n] : T(0));
  }
  d_h[b * 2 * D + j] = dm;
  d_h[b * 2 * D + D + j] = dl;
}

// SHARED_V false: h [B, 2 D] is shared by the S rows of v [B S, D] (the encoder's log_prob(z, x)); true: v [B, D] is
// shared by the S rows of h [B S, 2 D] (the Gaussian decoder).  With r = (v - mean) exp(-lv):
//   d_v = -g r,  d_mean = g r,  d_lv = g (r (v - mean) / 2 - 1 / 2)
template <typename T, bool SHARED_V>
__global__ __launch_bounds__(kBlock) void vae_gauss_bwd_kernel(const T* __restrict__ v, const T* __restrict__ h,
                                                               const T* __restrict__ g, T* __restrict__ d_v,
                                                               T* __restrict__ d_h, long long B, int S, int D) {
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= B * D) return;
  const long long b = t / D, j = t - b * D;
  if (!SHARED_V) {
    const T mean = h[b * 2 * D + j], inv = exp_(-h[b * 2 * D + D + j]);
    T dm = 0, dl = 0;
    for (long long n = b * S; n < (b + 1) * S; ++n) {
      const T gn = g[n], d = v[n * D + j] - mean, r = d * inv;
      if (d_v) d_v[n * D + j] = -gn * r;
      dm += gn * r;
      dl += gn * (T(0.5) * r * d - T(0.5));
    }
    if (d_h) {
      d_h[b * 2 * D + j] = dm;
      d_h[b * 2 * D + D + j] = dl;
    }
  } else {
    const T vv = v[b * D + j];
    T dv = 0;
    for (long long n = b * S; n < (b + 1) * S; ++n) {
      const T gn = g[n], d = vv - h[n * 2 * D + j], r = d * exp_(-h[n * 2 * D + D + j]);
      if (d_h) {
        d_h[n * 2 * D + j] = gn * r;
        d_h[n * 2 * D + D + j] = gn * (T(0.5) * r * d - T(0.5));
      }
      dv += -gn * r;
    }
    if (d_v) d_v[b * D + j] = dv;
  }
}

// d_score = g (x - sigmoid(a)); the sigmoid never exponentiates a positive number
template <typename T>
__global__ __launch_bounds__(kBlock) void vae_bernoulli_bwd_kernel(const T* __restrict__ x, const T* __restrict__ score,
                                                                   const T* __restrict__ g, T* __restrict__ d_score,
                                                                   long long B, int S, int D) {
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= B * D) return;
  const long long b = t / D, j = t - b * D;
  const T xv = x[b * D + j];
  for (long long n = b * S; n < (b + 1) * S; ++n) {
    const T a = score[n * D + j], e = exp_(-abs_(a));
    const T sig = a >= T(0) ? T(1) / (T(1) + e) : e / (T(1) + e);
    d_score[n * D + j] = g[n] * (xv - sig);
  }
}

// ------------------------------------------------------------------ host side
// workgroups of `items` pieces of work at per_block a workgroup, or 0 when they exceed a grid (per_block <= kBlock)
static inline long long blocks_for(long long items, int per_block) {
  const long long blocks = (items + per_block - 1) / per_block;
  return blocks > kMaxGrid ? 0 : blocks;
}

// lanes of the VJP of `rows` items of D columns: 0 when they exceed a grid
static inline long long bwd_blocks(long long rows, int32_t D) {
  if (rows > kMaxGrid * kBlock / D) return 0;
  return blocks_for(rows * D, kBlock);
}

template <typename T, int OP>
static int launch_fwd(FwdArgs<T> p, void* stream) {
  constexpr int W = chunk_width<T>();
  p.G = pick_lanes(((long long)p.D + W - 1) / W);
  const long long blocks = blocks_for(p.N, kBlock / p.G);
  if (!blocks) return VCNF_ERR_SHAPE;
  p.cst = (T)(-0.5 * (double)p.D * kLog2Pi);
  return with_pack<T>(p.D, {p.a, p.h, p.z}, [&](auto V) {
    hipLaunchKernelGGL((vae_fwd_kernel<T, V(), OP>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, p);
    return launched();
  });
}

static inline bool ok_rows(int64_t B, int32_t S, int32_t D) { return B >= 0 && S >= 1 && D >= 1 && B <= INT64_MAX / S; }

// N rows read through the divisors a and b, one of which is 1
static inline bool ok_divisors(int64_t N, int32_t a, int32_t b, int32_t D) {
  return N >= 0 && D >= 1 && a >= 1 && b >= 1 && (a == 1 || b == 1) && N % a == 0 && N % b == 0;
}

template <typename T>
static int encode(const T* h, const T* eps, T* z, T* logq, int64_t B, int32_t S, int32_t D, void* stream) {
  if (!h || !eps || !z || !logq) return VCNF_ERR_NULL;
  if (!ok_rows(B, S, D)) return VCNF_ERR_SHAPE;
  if (B == 0) return VCNF_OK;
  if (!all_aligned({h, eps, z, logq}, sizeof(T))) return VCNF_ERR_ALIGN;
  return launch_fwd<T, ENCODE>(FwdArgs<T>{eps, h, z, logq, B * S, 1, S, D, 1, T(0)}, stream);
}

template <typename T>
static int encode_bwd(const T* h, const T* eps, const T* g_z, const T* g_lq, T* d_h, int64_t B, int32_t S, int32_t D,
                      void* stream) {
  if (!h || !eps || !d_h || (!g_z && !g_lq)) return VCNF_ERR_NULL;
  if (!ok_rows(B, S, D)) return VCNF_ERR_SHAPE;
  if (B == 0) return VCNF_OK;
  const long long blocks = bwd_blocks(B, D);
  if (!blocks) return VCNF_ERR_SHAPE;
  if (!all_aligned({h, eps, g_z, g_lq, d_h}, sizeof(T))) return VCNF_ERR_ALIGN;
  if (S > VCNF_VAE_MAX_SAMPLES) return VCNF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((vae_encode_bwd_kernel<T>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, h, eps, g_z,
                     g_lq, d_h, (long long)B, S, D);
  return launched();
}

template <typename T>
static int gauss_log_prob(const T* v, const T* h, T* logp, int64_t N, int32_t v_div, int32_t h_div, int32_t D, void* stream) {
  if (!v || !h || !logp) return VCNF_ERR_NULL;
  if (!ok_divisors(N, v_div, h_div, D)) return VCNF_ERR_SHAPE;
  if (N == 0) return VCNF_OK;
  if (!all_aligned({v, h, logp}, sizeof(T))) return VCNF_ERR_ALIGN;
  return launch_fwd<T, GAUSS>(FwdArgs<T>{v, h, nullptr, logp, N, v_div, h_div, D, 1, T(0)}, stream);
}

template <typename T>
static int gauss_log_prob_bwd(const T* v, const T* h, const T* g, T* d_v, T* d_h, int64_t N, int32_t v_div, int32_t h_div,
                              int32_t D, void* stream) {
  if (!v || !h || !g || (!d_v && !d_h)) return VCNF_ERR_NULL;
  if (!ok_divisors(N, v_div, h_div, D)) return VCNF_ERR_SHAPE;
  if (N == 0) return VCNF_OK;
  const int32_t S = v_div > h_div ? v_div : h_div;
  const long long B = N / S, blocks = bwd_blocks(B, D);
  if (!blocks) return VCNF_ERR_SHAPE;
  if (!all_aligned({v, h, g, d_v, d_h}, sizeof(T))) return VCNF_ERR_ALIGN;
  if (S > VCNF_VAE_MAX_SAMPLES) return VCNF_ERR_UNSUPPORTED;
  return with_flags([&](auto SHARED_V) {
    hipLaunchKernelGGL((vae_gauss_bwd_kernel<T, SHARED_V()>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       v, h, g, d_v, d_h, B, S, D);
    return launched();
  }, v_div > 1);
}

template <typename T>
static int bernoulli_log_prob(const T* x, const T* score, T* logp, int64_t N, int32_t x_div, int32_t D, void* stream) {
  if (!x || !score || !logp) return VCNF_ERR_NULL;
  if (!ok_divisors(N, 1, x_div, D)) return VCNF_ERR_SHAPE;
  if (N == 0) return VCNF_OK;
  if (!all_aligned({x, score, logp}, sizeof(T))) return VCNF_ERR_ALIGN;
  return launch_fwd<T, BERNOULLI>(FwdArgs<T>{score, x, nullptr, logp, N, 1, x_div, D, 1, T(0)}, stream);
}

template <typename T>
static int bernoulli_log_prob_bwd(const T* x, const T* score, const T* g, T* d_score, int64_t N, int32_t x_div, int32_t D,
                                  void* stream) {
  if (!x || !score || !g || !d_score) return VCNF_ERR_NULL;
  if (!ok_divisors(N, 1, x_div, D)) return VCNF_ERR_SHAPE;
  if (N == 0) return VCNF_OK;
  const long long B = N / x_div, blocks = bwd_blocks(B, D);
  if (!blocks) return VCNF_ERR_SHAPE;
  if (!all_aligned({x, score, g, d_score}, sizeof(T))) return VCNF_ERR_ALIGN;
  if (x_div > VCNF_VAE_MAX_SAMPLES) return VCNF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((vae_bernoulli_bwd_kernel<T>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, x, score, g,
                     d_score, B, x_div, D);
  return launched();
}

}  // namespace vcnf_vae

using namespace vcnf_vae;

#define VCNF_VAE_ENTRY_POINTS(T, SFX)                                                                                  \
  extern "C" int vcnf_vae_encode_##SFX(const T* h, const T* eps, T* z, T* logq, int64_t batch, int32_t samples,        \
                                       int32_t features, void* stream) {                                               \
    return encode<T>(h, eps, z, logq, batch, samples, features, stream);                                               \
  }                                                                                                                    \
  extern "C" int vcnf_vae_encode_bwd_##SFX(const T* h, const T* eps, const T* g_z, const T* g_lq, T* d_h,              \
                                           int64_t batch, int32_t samples, int32_t features, void* stream) {           \
    return encode_bwd<T>(h, eps, g_z, g_lq, d_h, batch, samples, features, stream);                                    \
  }                                                                                                                    \
  extern "C" int vcnf_vae_gauss_log_prob_##SFX(const T* v, const T* h, T* logp, int64_t rows, int32_t v_div,           \
                                               int32_t h_div, int32_t features, void* stream) {                        \
    return gauss_log_prob<T>(v, h, logp, rows, v_div, h_div, features, stream);                                        \
  }                                                                                                                    \
  extern "C" int vcnf_vae_gauss_log_prob_bwd_##SFX(const T* v, const T* h, const T* g_lp, T* d_v, T* d_h,              \
                                                   int64_t rows, int32_t v_div, int32_t h_div, int32_t features,       \
                                                   void* stream) {                                                     \
    return gauss_log_prob_bwd<T>(v, h, g_lp, d_v, d_h, rows, v_div, h_div, features, stream);                          \
  }                                                                                                                    \
  extern "C" int vcnf_vae_bernoulli_log_prob_##SFX(const T* x, const T* score, T* logp, int64_t rows, int32_t x_div,   \
                                                   int32_t features, void* stream) {                                   \
    return bernoulli_log_prob<T>(x, score, logp, rows, x_div, features, stream);                                       \
  }                                                                                                                    \
  extern "C" int vcnf_vae_bernoulli_log_prob_bwd_##SFX(const T* x, const T* score, const T* g_lp, T* d_score,          \
                                                       int64_t rows, int32_t x_div, int32_t features, void* stream) {  \
    return bernoulli_log_prob_bwd<T>(x, score, g_lp, d_score, rows, x_div, features, stream);                          \
  }

VCNF_VAE_ENTRY_POINTS(float, f32)
VCNF_VAE_ENTRY_POINTS(double, f64)
