// Affine coupling, masked affine, per-channel affine, column gather and
// diagonal-Gaussian end caps for MI355X (gfx950, wave64), with their C-ABI entry
// points.  All of these are HBM-bound elementwise maps with a per-sample row
// reduction: one group of G lanes (power of two <= 64) owns a sample, strides over
// its row with coalesced accesses, and the log|det| partials are combined with
// wave shuffles - no second pass over the data and no atomics.
#include <type_traits>

#include "stream_common.hpp"

namespace vcnf {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 256 * 16;

static inline dim3 grid_for(long long groups, int G) { return vcnf_stream::grid_for(groups, G, kBlock, kMaxBlocks); }

// The kernels below that the reference's fp64 drivers reach (runadultvdeq.py:101-108,183: model.double() over
// MaskedAffineFlow / ActNorm / DiagGaussian stacks) are templates on the scalar type; the fp32 instantiations are the
// code they always were, the fp64 ones use the double-precision library functions.
// Row sums are lanes_sum_descending throughout this unit.

// torch.sigmoid and log(sigmoid) evaluated like the reference does
// (flows/affine/coupling.py:128-136): sigma = 1/(1+exp(-v)), then log(sigma).
__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ double sigmoid_f(double v) { return 1.0 / (1.0 + exp(-v)); }

// ------------------------------------------------------------------ affine coupling
template <typename T>
struct AffineArgsT {
  const T* z;
  const T* param;
  T* out;
  T* logdet;
  long long B;
  int C, inner, t_off, d_t;
  int scale_map, inverse, G, ld_mode;
  T ld_sign;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void affine_coupling_kernel(const AffineArgsT<T> a) {
  const int g = threadIdx.x & (a.G - 1);
  const int per_block = kBlock / a.G;
  const long long row = (long long)a.C * a.inner;          // elements of one sample
  const long long t_lo = (long long)a.t_off * a.inner;     // transformed span inside a row
  const long long t_n = (long long)a.d_t * a.inner;
  const int npar = a.scale_map == VCNF_SCALE_NONE ? 1 : 2;
  for (long long b = (long long)blockIdx.x * per_block + threadIdx.x / a.G; b < a.B;
       b += (long long)gridDim.x * per_block) {
    const T* zr = a.z + b * row;
    T* orow = a.out + b * row;
    const T* pr = a.param + b * (long long)npar * t_n;
    T acc = 0;
    for (long long e = g; e < row; e += a.G) {
      T v = zr[e];
      const long long te = e - t_lo;
      if (te >= 0 && te < t_n) {
        if (npar == 1) {                                   // coupling.py:139-141 / :165-167
          const T p = pr[te];
          v = a.inverse ? v - p : v + p;
        } else {
          const long long c = te / a.inner, i = te - c * a.inner;
          const T shift = pr[(2 * c) * a.inner + i];   // param[:, 0::2]
          const T sc = pr[(2 * c + 1) * a.inner + i];  // param[:, 1::2]
          if (a.scale_map == VCNF_SCALE_EXP) {             // :124-126 / :150-152
            if (a.inverse) { v = (v - shift) * exp_(-sc); acc -= sc; }
            else { v = v * exp_(sc) + shift; acc += sc; }
          } else {
            const T sg = sigmoid_f(sc + T(2));
            const T lg = log_(sg);
            const bool divide = (a.scale_map == VCNF_SCALE_SIGMOID) != (a.inverse != 0);
            if (a.inverse) v = divide ? (v - shift) / sg : (v - shift) * sg;
            else v = divide ? v / sg + shift : v * sg + shift;
            acc += divide ? -lg : lg;
          }
        }
      }
      orow[e] = v;
    }
    acc = lanes_sum_descending(acc, a.G);
    if (g == 0 && a.logdet) put_ld(a.logdet, b, a.ld_sign * acc, a.ld_mode);
  }
}

// ------------------------------------------------------------------ autoregressive affine (MAF)
// flows/affine/autoregressive.py:75-103: params [B, D, 2] = (unconstrained scale, shift) per feature from a MADE pass,
// scale = sigmoid(u + 2) + 1e-3; density direction y = scale x + shift, log|det| = sum log scale; the other direction
// y = (x - shift) / scale, log|det| = -sum log scale (called D times by the sampling loop, :29-36).
template <typename T>
struct MafArgsT {
  const T* x;
  const T* param;
  T* out;
  T* logdet;
  long long B;
  int D, inverse, G, ld_mode;
  T ld_sign;
};

// one (scale logit, shift) pair per 8 / 16-byte load
template <typename T> struct Pair;
template <> struct Pair<float> { using type = float2; };
template <> struct Pair<double> { using type = double2; };

template <typename T>
__global__ __launch_bounds__(kBlock) void maf_affine_kernel(const MafArgsT<T> a) {
  using P2 = typename Pair<T>::type;
  const int g = threadIdx.x & (a.G - 1);
  const int per_block = kBlock / a.G;
  for (long long b = (long long)blockIdx.x * per_block + threadIdx.x / a.G; b < a.B;
       b += (long long)gridDim.x * per_block) {
    const P2* pr = reinterpret_cast<const P2*>(a.param) + b * a.D;
    T acc = 0;
    for (int j = g; j < a.D; j += a.G) {
      const P2 p = pr[j];
      const T scale = sigmoid_f(p.x + T(2)) + T(1e-3);
      const T v = a.x[b * a.D + j];
      a.out[b * a.D + j] = a.inverse ? (v - p.y) / scale : scale * v + p.y;
      acc += log_(scale);
    }
    acc = lanes_sum_descending(acc, a.G);
    if (g == 0) put_ld(a.logdet, b, a.ld_sign * (a.inverse ? -acc : acc), a.ld_mode);
  }
}

// ------------------------------------------------------------------ masked affine
template <typename T>
struct MaskedArgsT {
  const T *z, *s, *t, *b;
  T* out;
  T* logdet;
  long long B;
  int D, inverse, G, ld_mode;
  T ld_sign;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void masked_affine_kernel(const MaskedArgsT<T> a) {
  const int g = threadIdx.x & (a.G - 1);
  const int per_block = kBlock / a.G;
  const T nanv = (T)__builtin_nanf("");
  for (long long r = (long long)blockIdx.x * per_block + threadIdx.x / a.G; r < a.B;
       r += (long long)gridDim.x * per_block) {
    T acc = 0;
    for (int j = g; j < a.D; j += a.G) {
      const long long e = r * a.D + j;
      const T m = a.b[j];
      const T zv = a.z[e];
      T sc = a.s ? a.s[e] : T(0);
      T tr = a.t ? a.t[e] : T(0);
      sc = isfinite(sc) ? sc : nanv;                       // coupling.py:205-208
      tr = isfinite(tr) ? tr : nanv;
      const T zm = m * zv;
      const T om = T(1) - m;
      T v;
      if (a.inverse) v = zm + om * (zv - tr) * exp_(-sc);  // :220
      else v = zm + om * (zv * exp_(sc) + tr);             // :209
      a.out[e] = v;
      acc += om * sc;                                      // :210 / :221
    }
    acc = lanes_sum_descending(acc, a.G);
    if (g == 0) put_ld(a.logdet, r, a.ld_sign * (a.inverse ? -acc : acc), a.ld_mode);
  }
}

// ------------------------------------------------------------------ per-channel affine, gather
template <typename T>
struct ConstArgsT {
  const T *z, *s, *t;
  T* out;
  long long total;
  int C, inner, inverse;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void affine_const_kernel(const ConstArgsT<T> a) {
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.total; e += (long long)gridDim.x * kBlock) {
    const int c = (int)((e / a.inner) % a.C);
    const T s = a.s ? a.s[c] : T(0), t = a.t ? a.t[c] : T(0);
    const T v = a.z[e];
    a.out[e] = a.inverse ? (v - t) * exp_(-s) : v * exp_(s) + t;   // coupling.py:38 / :47
  }
}

template <typename T>
struct PermArgsT {
  const T* z;
  const int32_t* idx;
  T* out;
  long long total;
  int C, inner;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void permute_kernel(const PermArgsT<T> a) {
  const long long row = (long long)a.C * a.inner;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.total; e += (long long)gridDim.x * kBlock) {
    const long long b = e / row;
    const long long r = e - b * row;
    const int c = (int)(r / a.inner);
    const int i = (int)(r - (long long)c * a.inner);
    a.out[e] = a.z[b * row + (long long)a.idx[c] * a.inner + i];
  }
}

// The channel partition of a coupling as two tensors and back (the training path's gather / scatter,
// flows/neural_spline/coupling.py:86-88 and :122-124): idx lists the columns of the first part, then those of the
// second.  One pass each way - no [B, C] intermediate, no slice copies, and each direction is the other's VJP.
template <typename T>
struct SplitArgsT {
  const T* z;          // split: source [B, C]; merge: unused
  T* out;              // merge: destination [B, C]; split: unused
  T* a;                // [B, na]
  T* b;                // [B, C - na]
  const int32_t* idx;  // split: column of z that gathered position c reads; merge: gathered position that column c reads
  long long total;     // B * C
  int C, na;
};

template <typename T, bool MERGE>
__global__ __launch_bounds__(kBlock) void split_merge_kernel(const SplitArgsT<T> a) {
  const int nb = a.C - a.na;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.total; e += (long long)gridDim.x * kBlock) {
    const long long r = e / a.C;
    const int c = (int)(e - r * a.C);
    if (MERGE) {
      const int p = a.idx[c];
      a.out[e] = p < a.na ? a.a[r * a.na + p] : a.b[r * nb + (p - a.na)];
    } else {
      const T v = a.z[r * a.C + a.idx[c]];
      if (c < a.na) a.a[r * a.na + c] = v;
      else a.b[r * nb + (c - a.na)] = v;
    }
  }
}

// ------------------------------------------------------------------ diagonal Gaussian
template <typename T>
struct GaussArgsT {
  const T *in, *loc, *log_scale;
  T* z;
  T* logp;
  long long B;
  int D, G, ld_mode, sample;
  T log_temp, ld_sign, norm;   // norm = -0.5 * D * log(2 pi)
};

template <typename T>
__global__ __launch_bounds__(kBlock) void diag_gaussian_kernel(const GaussArgsT<T> a) {
  const int g = threadIdx.x & (a.G - 1);
  const int per_block = kBlock / a.G;
  for (long long r = (long long)blockIdx.x * per_block + threadIdx.x / a.G; r < a.B;
       r += (long long)gridDim.x * per_block) {
    T acc = 0;
    for (int j = g; j < a.D; j += a.G) {
      const T ls = a.log_scale[j] + a.log_temp;
      const T v = a.in[r * a.D + j];
      if (a.sample) {                                      // base.py:639-641
        a.z[r * a.D + j] = a.loc[j] + exp_(ls) * v;
        acc += ls + T(0.5) * v * v;
      } else {                                             // base.py:649-651
        const T u = (v - a.loc[j]) / exp_(ls);
        acc += ls + T(0.5) * u * u;
      }
    }
    acc = lanes_sum_descending(acc, a.G);
    if (g == 0) put_ld(a.logp, r, a.ld_sign * (a.norm - acc), a.ld_mode);
  }
}

// Same arithmetic for D <= NC * G (a lane owns at most NC fixed columns): the per-column constants - and the exp()
// of the scale - are computed once per lane instead of once per element (the loads from log_scale may alias the
// outputs, so the compiler cannot hoist them out of the row loop above), and two rows are in flight per lane group.
// 1M x 64: 201 -> 151 us per call (HBM floor 32 us); the four-columns-per-lane kernel below takes the aligned shapes.
template <int NC>
__global__ __launch_bounds__(kBlock) void diag_gaussian_cols_kernel(const GaussArgsT<float> a) {
  const int g = threadIdx.x & (a.G - 1);
  const int per_block = kBlock / a.G;
  float ls[NC], sc[NC], lc[NC];
  bool have[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int j = g + c * a.G;
    have[c] = j < a.D;
    ls[c] = have[c] ? a.log_scale[j] + a.log_temp : 0.f;
    sc[c] = expf(ls[c]);
    lc[c] = have[c] ? a.loc[j] : 0.f;
  }
  const long long step = (long long)gridDim.x * per_block;
  for (long long r = (long long)blockIdx.x * per_block + threadIdx.x / a.G; r < a.B; r += 2 * step) {
    const long long r2 = r + step;
    const bool two = r2 < a.B;
    float v0[NC], v1[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      v0[c] = have[c] ? a.in[r * a.D + g + c * a.G] : 0.f;
      v1[c] = (have[c] && two) ? a.in[r2 * a.D + g + c * a.G] : 0.f;
    }
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (have[c]) {
        if (a.sample) {
          a.z[r * a.D + g + c * a.G] = lc[c] + sc[c] * v0[c];
          if (two) a.z[r2 * a.D + g + c * a.G] = lc[c] + sc[c] * v1[c];
          acc0 += ls[c] + 0.5f * v0[c] * v0[c];
          acc1 += ls[c] + 0.5f * v1[c] * v1[c];
        } else {
          const float u0 = (v0[c] - lc[c]) / sc[c], u1 = (v1[c] - lc[c]) / sc[c];
          acc0 += ls[c] + 0.5f * u0 * u0;
          acc1 += ls[c] + 0.5f * u1 * u1;
        }
      }
    }
    acc0 = lanes_sum_descending(acc0, a.G);
    acc1 = lanes_sum_descending(acc1, a.G);
    if (g == 0) {
      put_ld(a.logp, r, a.ld_sign * (a.norm - acc0), a.ld_mode);
      if (two) put_ld(a.logp, r2, a.ld_sign * (a.norm - acc1), a.ld_mode);
    }
  }
}

// D % 4 == 0, D <= 256, 16-byte aligned rows: a lane owns FOUR ADJACENT columns (one 16-byte load / store per row), a
// row is shared by G = pow2 >= D / 4 lanes, so the log2(G) shuffle steps of the row sum are paid once per four elements
// (with one column per lane a 64-feature row spent more instructions in the reduction than in the density).
__global__ __launch_bounds__(kBlock) void diag_gaussian_vec4_kernel(const GaussArgsT<float> a) {
  const int g = threadIdx.x & (a.G - 1);
  const int per_block = kBlock / a.G;
  const bool have = 4 * g < a.D;
  float ls[4], sc[4], lc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    ls[c] = have ? a.log_scale[4 * g + c] + a.log_temp : 0.f;
    sc[c] = expf(ls[c]);
    lc[c] = have ? a.loc[4 * g + c] : 0.f;
  }
  const long long step = (long long)gridDim.x * per_block;
  const int d4 = a.D >> 2;
  for (long long r = (long long)blockIdx.x * per_block + threadIdx.x / a.G; r < a.B; r += 2 * step) {
    const long long r2 = r + step;
    const bool two = r2 < a.B;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 p0 = have ? reinterpret_cast<const float4*>(a.in)[r * d4 + g] : z4;
    const float4 p1 = (have && two) ? reinterpret_cast<const float4*>(a.in)[r2 * d4 + g] : z4;
    const float v0[4] = {p0.x, p0.y, p0.z, p0.w}, v1[4] = {p1.x, p1.y, p1.z, p1.w};
    float acc0 = 0.f, acc1 = 0.f;
    float o0[4], o1[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (a.sample) {
        o0[c] = lc[c] + sc[c] * v0[c];
        o1[c] = lc[c] + sc[c] * v1[c];
        acc0 += ls[c] + 0.5f * v0[c] * v0[c];
        acc1 += ls[c] + 0.5f * v1[c] * v1[c];
      } else {
        const float u0 = (v0[c] - lc[c]) / sc[c], u1 = (v1[c] - lc[c]) / sc[c];
        acc0 += ls[c] + 0.5f * u0 * u0;
        acc1 += ls[c] + 0.5f * u1 * u1;
      }
    }
    if (a.sample && have) {
      reinterpret_cast<float4*>(a.z)[r * d4 + g] = make_float4(o0[0], o0[1], o0[2], o0[3]);
      if (two) reinterpret_cast<float4*>(a.z)[r2 * d4 + g] = make_float4(o1[0], o1[1], o1[2], o1[3]);
    }
    acc0 = lanes_sum_descending(have ? acc0 : 0.f, a.G);
    acc1 = lanes_sum_descending(have ? acc1 : 0.f, a.G);
    if (g == 0) {
      put_ld(a.logp, r, a.ld_sign * (a.norm - acc0), a.ld_mode);
      if (two) put_ld(a.logp, r2, a.ld_sign * (a.norm - acc1), a.ld_mode);
    }
  }
}


// ------------------------------------------------------------------ host side: one function per entry point, T = float / double
template <typename T>
static int affine_coupling(const T* z, const T* param, T* out, T* logdet, int64_t batch, int32_t channels, int32_t inner,
                           int32_t t_off, int32_t d_t, int scale_map, int inverse, int ld_mode, T ld_sign, void* stream) {
  if (batch < 0 || channels < 1 || inner < 1 || t_off < 0 || d_t < 0 || t_off + d_t > channels) return VCNF_ERR_SHAPE;
  if (scale_map < VCNF_SCALE_EXP || scale_map > VCNF_SCALE_NONE) return VCNF_ERR_UNSUPPORTED;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!z || !out || (d_t > 0 && !param)) return VCNF_ERR_NULL;
  if (scale_map != VCNF_SCALE_NONE && !logdet) return VCNF_ERR_NULL;
  AffineArgsT<T> a{z, param, out, logdet, batch, channels, inner, t_off, d_t, scale_map, inverse ? 1 : 0,
                   pick_lanes((long long)channels * inner), ld_mode, ld_sign};
  hipLaunchKernelGGL(affine_coupling_kernel<T>, grid_for(batch, a.G), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  return launched();
}

template <typename T>
static int maf_affine(const T* x, const T* params, T* out, T* logdet, int64_t batch, int32_t features, int inverse,
                      int ld_mode, T ld_sign, void* stream) {
  if (batch < 0 || features < 1) return VCNF_ERR_SHAPE;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!x || !params || !out || !logdet) return VCNF_ERR_NULL;
  if (reinterpret_cast<uintptr_t>(params) & (2 * sizeof(T) - 1)) return VCNF_ERR_ALIGN;   // float2 / double2 loads
  MafArgsT<T> a{x, params, out, logdet, batch, features, inverse ? 1 : 0, pick_lanes(features), ld_mode, ld_sign};
  hipLaunchKernelGGL(maf_affine_kernel<T>, grid_for(batch, a.G), dim3(kBlock), 0, (hipStream_t)stream, a);
  return launched();
}

template <typename T>
static int masked_affine(const T* z, const T* s, const T* t, const T* b, T* out, T* logdet, int64_t batch,
                         int32_t features, int inverse, int ld_mode, T ld_sign, void* stream) {
  if (batch < 0 || features < 1) return VCNF_ERR_SHAPE;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!z || !b || !out || !logdet) return VCNF_ERR_NULL;
  MaskedArgsT<T> a{z, s, t, b, out, logdet, batch, features, inverse ? 1 : 0, pick_lanes(features), ld_mode, ld_sign};
  hipLaunchKernelGGL(masked_affine_kernel<T>, grid_for(batch, a.G), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  return launched();
}

template <typename T>
static int affine_const(const T* z, const T* s, const T* t, T* out, int64_t batch, int32_t channels, int32_t inner,
                        int inverse, void* stream) {
  if (batch < 0 || channels < 1 || inner < 1) return VCNF_ERR_SHAPE;
  if (batch == 0) return VCNF_OK;
  if (!z || !out) return VCNF_ERR_NULL;
  ConstArgsT<T> a{z, s, t, out, batch * (long long)channels * inner, channels, inner, inverse ? 1 : 0};
  hipLaunchKernelGGL(affine_const_kernel<T>, grid_for(a.total, 1), dim3(kBlock), 0, (hipStream_t)stream, a);
  return launched();
}

template <typename T>
static int permute(const T* z, const int32_t* idx, T* out, int64_t batch, int32_t channels, int32_t inner, void* stream) {
  if (batch < 0 || channels < 1 || inner < 1) return VCNF_ERR_SHAPE;
  if (batch == 0) return VCNF_OK;
  if (!z || !idx || !out) return VCNF_ERR_NULL;
  PermArgsT<T> a{z, idx, out, batch * (long long)channels * inner, channels, inner};
  hipLaunchKernelGGL(permute_kernel<T>, grid_for(a.total, 1), dim3(kBlock), 0, (hipStream_t)stream, a);
  return launched();
}

template <typename T, bool MERGE>
static int split_merge(const T* z, T* out, T* pa, T* pb, const int32_t* idx, int64_t batch, int32_t channels,
                       int32_t first, void* stream) {
  if (batch < 0 || channels < 1 || first < 0 || first > channels) return VCNF_ERR_SHAPE;
  if (batch == 0) return VCNF_OK;
  if (!(MERGE ? (const void*)out : (const void*)z) || !idx || (first > 0 && !pa) || (first < channels && !pb)) return VCNF_ERR_NULL;
  SplitArgsT<T> a{z, out, pa, pb, idx, batch * (long long)channels, channels, first};
  hipLaunchKernelGGL((split_merge_kernel<T, MERGE>), grid_for(a.total, 1), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  return launched();
}

// fp32 rows of at most 4 columns per lane take the kernels that keep the column constants in registers; everything
// else, and fp64 always, takes the generic kernel
template <typename T>
static int gauss(const T* in, const T* loc, const T* log_scale, T log_temperature, T* z, T* logp, int64_t batch,
                 int32_t features, int ld_mode, T ld_sign, int sample, void* stream) {
  if (batch < 0 || features < 1) return VCNF_ERR_SHAPE;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!in || !loc || !log_scale || !logp || (sample && !z)) return VCNF_ERR_NULL;
  GaussArgsT<T> a{in, loc, log_scale, z, logp, batch, features, pick_lanes(features), ld_mode, sample,
                  log_temperature, ld_sign, (T)(-0.5 * (double)features * log(2.0 * M_PI))};
  hipStream_t st = (hipStream_t)stream;
  const bool vec4 = std::is_same<T, float>::value && features % 4 == 0 && features <= 256 &&
                    all_aligned({in, sample ? z : nullptr}, 16);
  if (vec4) a.G = pick_lanes(features / 4);
  const dim3 grid = grid_for(batch, a.G);
  if constexpr (std::is_same<T, float>::value) {
    if (vec4) {
      hipLaunchKernelGGL(diag_gaussian_vec4_kernel, grid, dim3(kBlock), 0, st, a);
      return launched();
    }
    switch ((features + a.G - 1) / a.G) {
      case 1: hipLaunchKernelGGL(diag_gaussian_cols_kernel<1>, grid, dim3(kBlock), 0, st, a); return launched();
      case 2: hipLaunchKernelGGL(diag_gaussian_cols_kernel<2>, grid, dim3(kBlock), 0, st, a); return launched();
      case 3: hipLaunchKernelGGL(diag_gaussian_cols_kernel<3>, grid, dim3(kBlock), 0, st, a); return launched();
      case 4: hipLaunchKernelGGL(diag_gaussian_cols_kernel<4>, grid, dim3(kBlock), 0, st, a); return launched();
    }
  }
  hipLaunchKernelGGL(diag_gaussian_kernel<T>, grid, dim3(kBlock), 0, st, a);
  return launched();
}

}  // namespace vcnf

using namespace vcnf;

extern "C" int vcnf_abi_version(void) { return VCNF_ABI_VERSION; }

extern "C" const char* vcnf_status_string(int status) {
  switch (status) {
    case VCNF_OK: return "ok";
    case VCNF_ERR_NULL: return "required pointer is NULL";
    case VCNF_ERR_SHAPE: return "inconsistent or unsupported sizes";
    case VCNF_ERR_ALIGN: return "buffer not 4-byte aligned";
    case VCNF_ERR_VALUE: return "minimal bin width/height too large for the number of bins";
    case VCNF_ERR_UNSUPPORTED: return "unsupported mode";
    case VCNF_ERR_LAUNCH: return "kernel launch failed";
    default: return "unknown status";
  }
}

#define VCNF_AFFINE_ENTRY_POINTS(T, SFX)                                                                               \
  extern "C" int vcnf_affine_coupling_##SFX(const T* z, const T* param, T* out, T* logdet, int64_t batch,              \
                                            int32_t channels, int32_t inner, int32_t t_off, int32_t d_t,               \
                                            int scale_map, int inverse, int ld_mode, T ld_sign, void* stream) {        \
    return affine_coupling<T>(z, param, out, logdet, batch, channels, inner, t_off, d_t, scale_map, inverse, ld_mode,  \
                              ld_sign, stream);                                                                        \
  }                                                                                                                    \
  extern "C" int vcnf_maf_affine_##SFX(const T* x, const T* params, T* out, T* logdet, int64_t batch,                  \
                                       int32_t features, int inverse, int ld_mode, T ld_sign, void* stream) {          \
    return maf_affine<T>(x, params, out, logdet, batch, features, inverse, ld_mode, ld_sign, stream);                  \
  }                                                                                                                    \
  extern "C" int vcnf_masked_affine_##SFX(const T* z, const T* s, const T* t, const T* b, T* out, T* logdet,           \
                                          int64_t batch, int32_t features, int inverse, int ld_mode, T ld_sign,        \
                                          void* stream) {                                                              \
    return masked_affine<T>(z, s, t, b, out, logdet, batch, features, inverse, ld_mode, ld_sign, stream);              \
  }                                                                                                                    \
  extern "C" int vcnf_affine_const_##SFX(const T* z, const T* s, const T* t, T* out, int64_t batch, int32_t channels,  \
                                         int32_t inner, int inverse, void* stream) {                                   \
    return affine_const<T>(z, s, t, out, batch, channels, inner, inverse, stream);                                     \
  }                                                                                                                    \
  extern "C" int vcnf_permute_##SFX(const T* z, const int32_t* idx, T* out, int64_t batch, int32_t channels,           \
                                    int32_t inner, void* stream) {                                                     \
    return permute<T>(z, idx, out, batch, channels, inner, stream);                                                    \
  }                                                                                                                    \
  extern "C" int vcnf_split_columns_##SFX(const T* z, const int32_t* idx, T* first_part, T* second_part,               \
                                          int64_t batch, int32_t channels, int32_t first, void* stream) {              \
    return split_merge<T, false>(z, nullptr, first_part, second_part, idx, batch, channels, first, stream);            \
  }                                                                                                                    \
  extern "C" int vcnf_merge_columns_##SFX(const T* first_part, const T* second_part, const int32_t* idx, T* out,       \
                                          int64_t batch, int32_t channels, int32_t first, void* stream) {              \
    return split_merge<T, true>(nullptr, out, const_cast<T*>(first_part), const_cast<T*>(second_part), idx, batch,     \
                                channels, first, stream);                                                              \
  }                                                                                                                    \
  extern "C" int vcnf_diag_gaussian_log_prob_##SFX(const T* z, const T* loc, const T* log_scale, T log_temperature,    \
                                                   T* logp, int64_t batch, int32_t features, int ld_mode, T ld_sign,   \
                                                   void* stream) {                                                     \
    return gauss<T>(z, loc, log_scale, log_temperature, nullptr, logp, batch, features, ld_mode, ld_sign, 0, stream);  \
  }                                                                                                                    \
  extern "C" int vcnf_diag_gaussian_sample_##SFX(const T* eps, const T* loc, const T* log_scale, T log_temperature,    \
                                                 T* z, T* logp, int64_t batch, int32_t features, void* stream) {       \
    return gauss<T>(eps, loc, log_scale, log_temperature, z, logp, batch, features, VCNF_LD_STORE, T(1), 1, stream);   \
  }

VCNF_AFFINE_ENTRY_POINTS(float, f32)
VCNF_AFFINE_ENTRY_POINTS(double, f64)
