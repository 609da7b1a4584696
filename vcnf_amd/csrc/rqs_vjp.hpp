// Adjoint of the rational-quadratic map inside one bin, templated on the scalar type: the fp32 VJP kernels
// (rqs_backward.hip) and the fp64 one (rqs_f64.hip) share this arithmetic.  ``B`` is the selected bin: any struct
// with members xl, w, yl, h, d0, d1 of type T.  Nothing here sets a floating-point pragma: each including file keeps
// its own contraction setting (rqs_backward.hip inherits rqs_math.hpp's ``fp contract(off)``).  Also here, shared by
// both precisions: the addressing of per-element interval limits and their adjoint (tensor left / right / bottom / top).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vcnf_hip.h"

namespace vcnf {

// Gradients w.r.t. the point and the bin: x, left x knot, width, left y knot, height, knot derivatives.
template <typename T>
struct BinGradT {
  T gx, gxl, gw, gyl, gh, gd0, gd1;
};

// Adjoint of the bin-coordinate map  (t, s, h, d0, d1) -> (y - yl, lad):
//   y - yl = h (s t^2 + d0 t(1-t)) / Q,   Q = s + (d0 + d1 - 2 s) t(1-t)
//   lad    = log(s^2 (d1 t^2 + 2 s t(1-t) + d0 (1-t)^2)) - 2 log Q          (splines.py:179-191)
// gh is the direct dependence on h (through the numerator), not the one through s = h / w.
template <typename T>
struct CoreGradT {
  T gt, gs, gh, gd0, gd1;
};

template <typename T>
__device__ __forceinline__ CoreGradT<T> bin_core_vjp(T t, T s, T h, T d0, T d1, T gy, T gl) {
  const T omt = T(1) - t;
  const T a = t * omt;
  const T e = d0 + d1 - T(2) * s;
  const T inner = s * t * t + d0 * a;
  const T N = h * inner;
  const T Q = s + e * a;
  const T M = d1 * t * t + T(2) * s * a + d0 * omt * omt;
  const T rQ = T(1) / Q;
  const T g_dn = gl / (s * s * M);
  const T g_Q = -T(2) * gl * rQ - gy * N * rQ * rQ;
  const T g_N = gy * rQ;
  const T g_M = s * s * g_dn;
  const T g_in = h * g_N;
  const T g_e = a * g_Q;
  const T g_a = T(2) * s * g_M + e * g_Q + d0 * g_in;
  const T g_omt = T(2) * d0 * omt * g_M + t * g_a;
  CoreGradT<T> r;
  r.gs = T(2) * s * M * g_dn + T(2) * a * g_M + g_Q + t * t * g_in - T(2) * g_e;
  r.gt = T(2) * d1 * t * g_M + T(2) * s * t * g_in + omt * g_a - g_omt;
  r.gh = inner * g_N;
  r.gd0 = omt * omt * g_M + a * g_in + g_e;
  r.gd1 = t * t * g_M + g_e;
  return r;
}

// Density direction: y = F(x), lad = log F'(x), with t = (x - xl) / w and s = h / w.
template <typename T, typename B>
__device__ __forceinline__ BinGradT<T> bin_forward_vjp(T x, const B& b, T gy, T gl) {
  const T rw = T(1) / b.w;
  const T s = b.h * rw;
  const T t = (x - b.xl) * rw;
  const CoreGradT<T> c = bin_core_vjp<T>(t, s, b.h, b.d0, b.d1, gy, gl);
  BinGradT<T> r;
  r.gx = c.gt * rw;
  r.gxl = -r.gx;
  r.gw = -(c.gt * t + c.gs * s) * rw;
  r.gh = c.gh + c.gs * rw;
  r.gyl = gy;
  r.gd0 = c.gd0;
  r.gd1 = c.gd1;
  return r;
}

// Sampling direction: v = xl + w r with r the root of  h phi(r; s, d0, d1) = u - yl,  lad = -log F'(v).
// The root is differentiated implicitly IN BIN COORDINATES (dr/du = 1 / (h phi_r), dr/ds = -phi_s / phi_r,
// ...): written per unit x the width gradient is a difference of two terms of size L_t / w that
// agree to several digits in narrow bins; in r they never appear.  ``r`` is the root, rw = 1 / w, s = h / w.
template <typename T, typename B>
__device__ __forceinline__ BinGradT<T> bin_inverse_vjp_at_root(T r, T rw, T s, const B& b, T gy, T gl) {
  const CoreGradT<T> F = bin_core_vjp<T>(r, s, b.h, b.d0, b.d1, T(1), T(0));
  const CoreGradT<T> L = bin_core_vjp<T>(r, s, b.h, b.d0, b.d1, T(0), T(1));
  const T gr = gy * b.w - gl * L.gt;
  const T gu = gr / F.gt;
  const T gs = -gu * F.gs - gl * L.gs;
  BinGradT<T> o;
  o.gx = gu;
  o.gyl = -gu;
  o.gxl = gy;
  o.gw = gy * r - gs * s * rw;
  o.gh = -gu * F.gh + gs * rw;
  o.gd0 = -gu * F.gd0 - gl * L.gd0;
  o.gd1 = -gu * F.gd1 - gl * L.gd1;
  return o;
}

// ---- per-element interval limits (vcnf_rqs_elementwise_limits_*): the knots of one side are
// x_k = lo + (hi - lo) c_k with the cumulative fractions c_0 = 0, c_K = 1 exact (the end knots are the limits).
// Broadcast addressing of limit j: element i reads lim[j][(i / inner[j]) % period[j]] (include/vcnf_hip.h).
// n / d for every 32-bit n by one high multiply, two shifts and two adds (Granlund & Montgomery, "Division by invariant
// integers using multiplication", 1994): the multiplier and shifts are computed once on the host, 1 <= d <= 2^31.
struct FastDivU32 {
  unsigned d, m, s1, s2;
  __device__ __forceinline__ unsigned div(unsigned n) const {
    const unsigned t = __umulhi(n, m);
    return (t + ((n - t) >> s1)) >> s2;
  }
};

inline FastDivU32 make_fastdiv(unsigned d) {
  unsigned l = 0;
  while ((1ull << l) < d) ++l;                     // ceil(log2 d) <= 31
  FastDivU32 f;
  f.d = d;
  f.m = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
  f.s1 = l < 1 ? l : 1;
  f.s2 = l > 1 ? l - 1 : 0;
  return f;
}

template <typename T>
struct LimitsT {
  const T* lim[4];                 // left, right, bottom, top
  long long period[4], inner[4];
  FastDivU32 dp[4], di[4];         // narrow: the divisions by period and inner
  int narrow;                      // every element index below 2^32, every period / inner at most 2^31
  int same_prev[4];                // limit j is addressed like limit j - 1: its index is reused
  template <bool NARROW>
  __device__ __forceinline__ long long index(int j, long long i) const {
    if (NARROW) {
      const unsigned q = di[j].div((unsigned)i);
      return q - dp[j].d * dp[j].div(q);
    }
    return (i / inner[j]) % period[j];
  }
  // the four limits of element i; NARROW: the caller has checked ``narrow`` (no 64-bit division in the code)
  template <bool NARROW>
  __device__ __forceinline__ void load_as(long long i, T (&v)[4]) const {
    long long q = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j == 0 || !same_prev[j]) q = index<NARROW>(j, i);
      v[j] = lim[j][q];
    }
  }
  __device__ __forceinline__ void load(long long i, T (&v)[4]) const {
    if (narrow) load_as<true>(i, v);
    else load_as<false>(i, v);
  }
};

// Gradients of one side's two limits from the selected bin: knot gradients g(x_b) = g_xl - g_w (left knot) and
// g(x_b+1) = g_w (right knot), dx_k / dlo = 1 - c_k, dx_k / dhi = c_k.
template <typename T>
__device__ __forceinline__ void limit_vjp(T g_knot0, T g_knot1, T c0, T c1, T& g_lo, T& g_hi) {
  g_lo = g_knot0 * (T(1) - c0) + g_knot1 * (T(1) - c1);
  g_hi = g_knot0 * c0 + g_knot1 * c1;
}

// Host side of the four vcnf_rqs_elementwise_limits_* entry points.  Validation in this order: cfg, K, tails (the
// functional spline has none), bin minima, sizes, broadcast layout; the caller then returns VCNF_OK for n == 0
// before it looks at the data pointers.
template <class Cfg>
inline int limits_validate(const Cfg* cfg, int64_t n, int64_t ld_w, int64_t ld_h, int64_t ld_d,
                           const vcnf_rqs_limit_bcast* bc) {
  if (!cfg) return VCNF_ERR_NULL;
  const int K = cfg->num_bins;
  if (K < 1 || K > 64) return VCNF_ERR_SHAPE;
  if (cfg->tails != VCNF_TAILS_NONE) return VCNF_ERR_UNSUPPORTED;
  if ((double)cfg->min_bin_width * K > 1.0 || (double)cfg->min_bin_height * K > 1.0) return VCNF_ERR_VALUE;
  if (n < 0 || ld_w < 0 || ld_h < 0 || ld_d < 0) return VCNF_ERR_SHAPE;
  if (!bc) return VCNF_ERR_NULL;
  for (int j = 0; j < 4; ++j)
    if (bc->period[j] < 1 || bc->inner[j] < 1) return VCNF_ERR_SHAPE;
  return VCNF_OK;
}

template <typename T>
inline LimitsT<T> make_limits(const T* left, const T* right, const T* bottom, const T* top,
                              const vcnf_rqs_limit_bcast* bc, int64_t n) {
  LimitsT<T> l;
  l.lim[0] = left; l.lim[1] = right; l.lim[2] = bottom; l.lim[3] = top;
  l.narrow = n <= 0xffffffffLL;
  for (int j = 0; j < 4; ++j) {
    l.period[j] = bc->period[j];
    l.inner[j] = bc->inner[j];
    l.narrow = l.narrow && bc->period[j] <= 0x80000000LL && bc->inner[j] <= 0x80000000LL;
    l.same_prev[j] = j > 0 && bc->period[j] == bc->period[j - 1] && bc->inner[j] == bc->inner[j - 1];
  }
  for (int j = 0; j < 4; ++j) {
    l.dp[j] = make_fastdiv(l.narrow ? (unsigned)bc->period[j] : 1u);
    l.di[j] = make_fastdiv(l.narrow ? (unsigned)bc->inner[j] : 1u);
  }
  return l;
}

}  // namespace vcnf
