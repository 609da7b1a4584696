// Adjoint of the rational-quadratic map inside one bin, templated on the scalar type: the fp32 VJP kernels
// (rqs_backward.hip) and the fp64 one (rqs_f64.hip) share this arithmetic.  ``B`` is the selected bin: any struct
// with members xl, w, yl, h, d0, d1 of type T.  Nothing here sets a floating-point pragma: each including file keeps
// its own contraction setting (rqs_backward.hip inherits rqs_math.hpp's ``fp contract(off)``).
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace vcnf
