// Device functions of the three 2-D targets of normflow 1.2 (distributions/target.py), stated once for the units that
// evaluate them: target_density.hip (log p and its score in one launch) and stochastic.hip (the HMC runs and
// Metropolis-Hastings walks, which evaluate them at every leapfrog point).  With r = sqrt(z0^2 + z1^2) and a = |z0|:
//   TwoMoons          logp = -((r - 2) / 0.2)^2 / 2 - ((a - 2) / 0.3)^2 / 2 + log1p(exp(-4 a / 0.09))
//   circular mixture  d_i = |z - c_i|^2 / (2 s^2),  logp = -log(2 pi s^2 n) + logsumexp_i(-d_i),  c = table [n, 2]
//   ring mixture      d_i = (r - t_i)^2 / (2 s^2),  logp = logsumexp_i(-d_i),                     t = table [n]
// Every lane walks all n components, so the table is read at a wave-uniform index.  The logsumexp takes two passes over
// the components: the smallest d first, then the sum of exp(d_min - d_i) with the score's weighted sums beside it.
// Whether the score is computed is a template flag.  Contraction to fused multiply-adds is off in the including units
// (and below): logp is the same sequence of roundings with the score and without, in either unit.
#pragma once

#include "stream_common.hpp"

#pragma clang fp contract(off)

namespace vcnf_target {

using namespace vcnf_stream;

// z / r, 0 at r == 0 (the gradient torch gives norm there)
template <typename T>
__device__ __forceinline__ T unit(T z, T r) {
  return r > T(0) ? z / r : T(0);
}

template <typename T, bool SCORE>
__device__ __forceinline__ T two_moons(T z0, T z1, T& s0, T& s1) {
  const T r = sqrt_(z0 * z0 + z1 * z1), a = abs_(z0);
  const T tr = (r - T(2)) / T(0.2), ta = (a - T(2)) / T(0.3);
  const T e = exp_(T(-4) * a / T(0.09));
  if (SCORE) {
    // the bracket is 0 at a == 0: the density is smooth across z0 == 0, and sign(0) = 0 costs nothing
    const T k = -(r - T(2)) / T(0.04);
    const T sg = z0 > T(0) ? T(1) : z0 < T(0) ? T(-1) : T(0);
    s0 = k * unit(z0, r) + sg * ((T(2) - a) / T(0.09) - T(4.0 / 0.09) * (e / (T(1) + e)));
    s1 = k * unit(z1, r);
  }
  return T(-0.5) * tr * tr - T(0.5) * ta * ta + log1p_(e);
}

// F: VCNF_TARGET_CIRCULAR_GMM or VCNF_TARGET_RING_MIXTURE; i below is the same in every lane of a wave
template <typename T, int F, bool SCORE>
__device__ __forceinline__ T mixture(const T* __restrict__ table, int n, T scale, T z0, T z1, T& s0, T& s1) {
  const T var = scale * scale, h = T(1) / (T(2) * var);
  const T r = sqrt_(z0 * z0 + z1 * z1);
  auto dist = [&](int i) -> T {
    if (F == VCNF_TARGET_CIRCULAR_GMM) {
      const T x = z0 - table[2 * i], y = z1 - table[2 * i + 1];
      return (x * x + y * y) * h;
    }
    const T d = r - table[i];
    return d * d * h;
  };
  T least = dist(0);
  for (int i = 1; i < n; ++i) {
    const T d = dist(i);
    least = d < least ? d : least;
  }
  T sum = T(0), w0 = T(0), w1 = T(0);
  for (int i = 0; i < n; ++i) {
    const T w = exp_(least - dist(i));
    sum += w;
    if (SCORE) {
      if (F == VCNF_TARGET_CIRCULAR_GMM) {
        w0 += w * (table[2 * i] - z0);
        w1 += w * (table[2 * i + 1] - z1);
      } else {
        w0 += w * (table[i] - r);
      }
    }
  }
  if (SCORE) {
    const T k = T(1) / (var * sum);
    if (F == VCNF_TARGET_CIRCULAR_GMM) {
      s0 = w0 * k;
      s1 = w1 * k;
    } else {
      s0 = w0 * k * unit(z0, r);
      s1 = w0 * k * unit(z1, r);
    }
  }
  const T lse = log_(sum) - least;
  return F == VCNF_TARGET_CIRCULAR_GMM ? lse - log_(T(6.283185307179586476925) * var * T(n)) : lse;
}

static inline bool is_mixture(int f) { return f == VCNF_TARGET_CIRCULAR_GMM || f == VCNF_TARGET_RING_MIXTURE; }
static inline bool is_family(int f) { return f == VCNF_TARGET_TWO_MOONS || is_mixture(f); }

}  // namespace vcnf_target
