// Device-side rational-quadratic spline arithmetic in double precision: what the fp64 kernels of rqs_f64.hip (forward
// map and VJP) and both instances of made_sample.hip share - knots, bin search, derivative-logit padding - and, for the
// forward map and made_sample.hip, the selection of an element's bin (rqs_locate64), the root (rqs_root64) and one
// bin's map (rqs_bin_eval64), each defined once, so that every kernel selects the same bin and the two evaluate the
// same expressions.  The VJP kernel composes the first group itself and keeps its root in line: built on rqs_locate64
// and rqs_root64 its strided instances ran 5 - 9 % slower (profiles/rqs64_unit.md).  The reference's operation order as
// written in normflow/utils/splines.py:88-193: softmax -> floor -> cumsum -> affine map -> exact end knots -> sizes by
// differencing; compare-and-count bin search with the last knot bumped by 1e-6; the stable root form
// 2c / (-b - sqrt(disc)).  Library exp / log / sqrt.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/vcnf_hip.h"
#include "rqs_host.hpp"          // Rqs64Const

namespace vcnf {

// KT > 0: compile-time bin count (the templated instances keep every array in registers); KT == 0: runtime K (the
// generic instances of rqs_f64.hip, whose runtime-indexed arrays go to scratch).

// knots of one side: cum[0..K] from K logits lg[k * ks] (splines.py:109-119 / :123-133); ``prob`` (optional) receives
// the softmax probabilities, ``frac`` (optional) the cumulative fractions of the knots (0 and 1 at the ends)
template <int KT>
__device__ __forceinline__ void partition64(const double* lg, long long ks, int Kr, double scale, double lo, double hi,
                                            double floor_, double* cum, double* prob = nullptr,
                                            double* frac = nullptr) {
  const int K = KT > 0 ? KT : Kr;
  double m = -INFINITY;
  for (int k = 0; k < K; ++k) m = fmax(m, lg[k * ks] * scale);
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += exp(lg[k * ks] * scale - m);
  double run = 0.0;
  cum[0] = lo;
  for (int k = 0; k < K; ++k) {
    if (prob) prob[k] = exp(lg[k * ks] * scale - m) / s;
    const double p = floor_ + (1.0 - floor_ * K) * (exp(lg[k * ks] * scale - m) / s);
    run += p;
    cum[k + 1] = (hi - lo) * run + lo;
    if (frac) frac[k + 1] = run;
  }
  cum[K] = hi;
  if (frac) {
    frac[0] = 0.0;
    frac[K] = 1.0;
  }
}

// bin: number of knots <= value, last knot bumped by eps (splines.py:12-17), clamped to [0, K-1]
template <int KT>
__device__ __forceinline__ int bin64(const double* kn, int Kr, double x) {
  const int K = KT > 0 ? KT : Kr;
  int bin = -1;
  for (int k = 0; k <= K; ++k) bin += (x >= (k == K ? kn[k] + 1e-6 : kn[k])) ? 1 : 0;
  return bin < 0 ? 0 : (bin > K - 1 ? K - 1 : bin);
}

// derivative logit of knot k (padding per tails mode, splines.py:36-49): its column in the ud row, or -1 for the
// constant boundary logit of linear tails
__device__ __forceinline__ int dlogit_col64(int k, int K, int tails) {
  if (tails == VCNF_TAILS_LINEAR) return (k == 0 || k == K) ? -1 : k - 1;
  if (tails == VCNF_TAILS_CIRCULAR) return k == K ? 0 : k;
  return k;
}

__device__ __forceinline__ double softplus64(double v) { return v > 20.0 ? v : log1p(exp(v)); }   // F.softplus (threshold 20)

// the knots bounding bin ``bin`` on both sides.  KT > 0: picked by comparison, so that the knot arrays stay in
// registers; KT == 0: indexed.
template <int KT>
__device__ __forceinline__ void pick_bin64(const double* xk, const double* yk, int bin, int K, double& xl, double& xr,
                                           double& yl, double& yr) {
  if (KT > 0) {
    xl = xk[0]; xr = xk[1]; yl = yk[0]; yr = yk[1];
    for (int k = 1; k < K; ++k)
      if (bin == k) { xl = xk[k]; xr = xk[k + 1]; yl = yk[k]; yr = yk[k + 1]; }
  } else {
    xl = xk[bin]; xr = xk[bin + 1]; yl = yk[bin]; yr = yk[bin + 1];
  }
}

// The selected bin: its left knots, its sizes and the derivatives at its two knots (the B of rqs_vjp.hpp).
struct RqsBin64 {
  double xl, w, yl, h, d0, d1;
};

// Knots, then bin, then padded derivative logits, then the bin's six numbers, for one element inside the interval
// [left, right] x [bottom, top] (passed beside ``c``: the LIM kernels have them per element).  Logit k of the three rows
// at uw[k * ks], uh[k * ks], ud[k * ks]; ``inverse``: x is searched among the y knots.  The knot arrays xk, yk [K + 1]
// are the caller's locals, so that the KT > 0 instances keep them in registers.
template <int KT>
__device__ __forceinline__ void rqs_locate64(double x, bool inverse, const double* uw, const double* uh, const double* ud,
                                             long long ks, const Rqs64Const& c, double left, double right, double bottom,
                                             double top, double* xk, double* yk, RqsBin64& b) {
  const int K = KT > 0 ? KT : c.K;
  partition64<KT>(uw, ks, K, c.wh_scale, left, right, c.min_w, xk);
  partition64<KT>(uh, ks, K, c.wh_scale, bottom, top, c.min_h, yk);
  const int bin = bin64<KT>(inverse ? yk : xk, K, x);
  const int j0 = dlogit_col64(bin, K, c.tails), j1 = dlogit_col64(bin + 1, K, c.tails);
  b.d0 = c.min_d + softplus64(j0 < 0 ? c.edge : ud[j0 * ks]);        // :121
  b.d1 = c.min_d + softplus64(j1 < 0 ? c.edge : ud[j1 * ks]);
  double xr, yr;
  pick_bin64<KT>(xk, yk, bin, K, b.xl, xr, b.yl, yr);
  b.w = xr - b.xl;
  b.h = yr - b.yl;
}

// The root of the sampling direction in bin coordinates (splines.py:153-166), 2c / (-b - sqrt(disc)); ``bad`` is set on
// a negative discriminant (:164, the reference asserts).  ``s`` is the caller's.
__device__ __forceinline__ double rqs_root64(double dy, double h, double s, double d0, double d1, bool& bad) {
  const double e = d0 + d1 - 2.0 * s;
  const double qa = dy * e + h * (s - d0);                         // :153-161
  const double qb = h * d0 - dy * e;
  const double qc = -s * dy;
  const double disc = qb * qb - 4.0 * qa * qc;                     // :163
  bad = bad || !(disc >= 0.0);
  return (2.0 * qc) / (-qb - sqrt(disc));                          // :166
}

// One bin's map: y and log |dy/dx| of the density direction, or (INV) the root and minus that log-derivative at it.
template <bool INV>
__device__ __forceinline__ void rqs_bin_eval64(double x, const RqsBin64& b, double& y, double& lad, bool& bad) {
  const double s = b.h / b.w;                                      // :144
  const double t = INV ? rqs_root64(x - b.yl, b.h, s, b.d0, b.d1, bad) : (x - b.xl) / b.w;   // :179
  if (INV) y = t * b.w + b.xl;
  const double tt = t * (1.0 - t);
  const double num = b.h * (s * t * t + b.d0 * tt);
  // d0 + d1 - 2 s is formed here, after t, in both directions: the compiler contracts it with its neighbours into
  // fused multiply-adds, and stated ahead of t it is shared by a kernel's two directions and contracted otherwise
  const double den = s + (b.d0 + b.d1 - 2.0 * s) * tt;
  if (!INV) y = b.yl + num / den;                                  // :186
  const double dnum = s * s * (b.d1 * t * t + 2.0 * s * tt + b.d0 * (1.0 - t) * (1.0 - t));
  const double l = log(dnum) - 2.0 * log(den);                     // :191
  lad = INV ? -l : l;                                              // :175-177
}

// The sampling direction of one element inside its interval (the caller has taken the identity outside the tails,
// splines.py:30-49) with K = KT > 0 bins, every array in registers.
template <int KT>
__device__ __forceinline__ void rqs_inverse64(double x, const double* uw, const double* uh, const double* ud, long long ks,
                                              const Rqs64Const& c, double& out, double& lad, bool& bad) {
  static_assert(KT > 0, "compile-time bin count only: a runtime count would index the knot arrays in scratch");
  double xk[KT + 1], yk[KT + 1];
  RqsBin64 b;
  rqs_locate64<KT>(x, true, uw, uh, ud, ks, c, c.left, c.right, c.bottom, c.top, xk, yk, b);
  rqs_bin_eval64<true>(x, b, out, lad, bad);
}

}  // namespace vcnf
