// Device-side rational-quadratic spline arithmetic in double precision: what the fp64 kernels of rqs_f64.hip (forward
// map and VJP) and the fp64 instances of made_sample.hip share - knots, bin search, derivative-logit padding - each
// defined once, so that every kernel selects the same bin for every element.  The reference's operation order as
// written in normflow/utils/splines.py:88-193: softmax -> floor -> cumsum -> affine map -> exact end knots -> sizes by
// differencing; compare-and-count bin search with the last knot bumped by 1e-6; the stable root form
// 2c / (-b - sqrt(disc)).  Library exp / log / sqrt.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/vcnf_hip.h"

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

// The spline constants of one evaluation: the interval, the floors, the logit scale and the boundary logit of linear
// tails log(exp(1 - min_d) - 1).
struct Rqs64Const {
  int K, tails;
  double left, right, bottom, top, min_w, min_h, min_d, wh_scale, edge;
};

// The sampling direction of one element inside its interval (the caller has taken the identity outside the tails,
// splines.py:30-49) with K = KT > 0 bins, every array in registers: logit k of the three rows at uw[k * ks], uh[k * ks],
// ud[k * ks].  The knots, the bin and the padding are the functions above; the root is written as in
// rqs_elementwise_f64_kernel (rqs_f64.hip), expression for expression.  ``bad`` is set on a negative discriminant
// (splines.py:164, the reference asserts).
template <int KT>
__device__ __forceinline__ void rqs_inverse64(double x, const double* uw, const double* uh, const double* ud, long long ks,
                                              const Rqs64Const& c, double& out, double& lad, bool& bad) {
  static_assert(KT > 0, "compile-time bin count only: a runtime count would index the knot arrays in scratch");
  double xk[KT + 1], yk[KT + 1];
  partition64<KT>(uw, ks, KT, c.wh_scale, c.left, c.right, c.min_w, xk);
  partition64<KT>(uh, ks, KT, c.wh_scale, c.bottom, c.top, c.min_h, yk);
  const int bin = bin64<KT>(yk, KT, x);
  auto dlogit = [&](int k) -> double {
    const int j = dlogit_col64(k, KT, c.tails);
    return j < 0 ? c.edge : ud[j * ks];
  };
  const double d0 = c.min_d + softplus64(dlogit(bin));           // :121
  const double d1 = c.min_d + softplus64(dlogit(bin + 1));
  double x_lo, x_hi, y_lo, y_hi;
  pick_bin64<KT>(xk, yk, bin, KT, x_lo, x_hi, y_lo, y_hi);
  const double w = x_hi - x_lo;
  const double h = y_hi - y_lo;
  const double s = h / w;                                          // :144
  const double dy = x - y_lo;
  const double e = d0 + d1 - 2.0 * s;
  const double qa = dy * e + h * (s - d0);                         // :153-161
  const double qb = h * d0 - dy * e;
  const double qc = -s * dy;
  const double disc = qb * qb - 4.0 * qa * qc;                     // :163
  bad = bad || !(disc >= 0.0);                                     // :164
  const double r = (2.0 * qc) / (-qb - sqrt(disc));                // :166
  out = r * w + x_lo;
  const double rr = r * (1.0 - r);
  const double den = s + e * rr;
  const double dnum = s * s * (d1 * r * r + 2.0 * s * rr + d0 * (1.0 - r) * (1.0 - r));
  lad = -(log(dnum) - 2.0 * log(den));                             // :175-177
}

}  // namespace vcnf
