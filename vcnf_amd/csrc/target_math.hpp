// Device functions of the 2-D densities of normflow 1.2 - the three targets of distributions/target.py and the five
// energies of distributions/prior.py - stated once for the units that evaluate them: target_density.hip (log p and its
// score in one launch) and stochastic.hip (the HMC runs and Metropolis-Hastings walks, which evaluate them at every
// leapfrog point).  With r = sqrt(z0^2 + z1^2) and a = |z0|:
//   TwoMoons          logp = -((r - 2) / 0.2)^2 / 2 - ((a - 2) / 0.3)^2 / 2 + log1p(exp(-4 a / 0.09))
//   circular mixture  d_i = |z - c_i|^2 / (2 s^2),  logp = -log(2 pi s^2 n) + logsumexp_i(-d_i),  c = table [n, 2]
//   ring mixture      d_i = (r - t_i)^2 / (2 s^2),  logp = logsumexp_i(-d_i),                     t = table [n]
// and, with s = scale, q = (20 s)^4, om = 2 pi / period, w1 = sin(om z0), d = z1 - w1 and tail = (z0^4 + z1^4) / (2 q):
//   TwoModes          logp = -((r - loc) / 2s)^2 / 2 - ((a - |loc|) / 3s)^2 / 2 + log1p(exp(-2 a |loc| / (3s)^2)),
//                     table = {loc}
//   Sinusoidal        logp = -(d / s)^2 / 2 - tail,                                               table = {period}
//   Sinusoidal_gap    logp = logaddexp(-(d / s)^2 / 2, -((d + w) / s)^2 / 2) - tail,  w = A exp(-((z0 - mu) / sg)^2 / 2),
//   Sinusoidal_split  the same with w = A sigmoid((z0 - mu) / sg),                      table = {period, A, mu, sg}
//   Smiley            logp = -((r - 2) / 2s)^2 / 2 - ((|z1 + 0.8| - 1.2) / 2s)^2 / 2
// (the scores: include/vcnf_hip.h).  Every lane walks all n components of a mixture and reads an energy's constants at
// fixed indices, so the table is read at a wave-uniform index.  The logsumexp takes two passes over the components: the
// smallest d first, then the sum of exp(d_min - d_i) with the score's weighted sums beside it.  The two-branch log of the
// gap and the split subtracts its larger branch (max + log1p(exp(-|b - a|))) and its score weights are the sigmoid of
// b - a from the same exp: finite wherever the branches are.
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

// sign(v) with sign(0) = 0: torch's gradient of abs
template <typename T>
__device__ __forceinline__ T sign(T v) {
  return v > T(0) ? T(1) : v < T(0) ? T(-1) : T(0);
}

// table = {loc}
template <typename T, bool SCORE>
__device__ __forceinline__ T two_modes(const T* __restrict__ table, T scale, T z0, T z1, T& s0, T& s1) {
  const T loc = table[0], eps = abs_(loc), c1 = T(2) * scale, c2 = T(3) * scale, v2 = c2 * c2;
  const T r = sqrt_(z0 * z0 + z1 * z1), a = abs_(z0);
  const T tr = (r - loc) / c1, ta = (a - eps) / c2;
  const T e = exp_(T(-2) * a * eps / v2);
  if (SCORE) {
    // the bracket is 0 at a == 0 as in two_moons
    const T k = -(r - loc) / (c1 * c1);
    s0 = k * unit(z0, r) + sign(z0) * ((eps - a) / v2 - (T(2) * eps / v2) * (e / (T(1) + e)));
    s1 = k * unit(z1, r);
  }
  return T(-0.5) * tr * tr - T(0.5) * ta * ta + log1p_(e);
}

// F: VCNF_TARGET_SINUSOIDAL (table = {period}), VCNF_TARGET_SINUSOIDAL_GAP or VCNF_TARGET_SINUSOIDAL_SPLIT
// (table = {period, amp, mu, width})
template <typename T, int F, bool SCORE>
__device__ __forceinline__ T sinusoidal(const T* __restrict__ table, T scale, T z0, T z1, T& s0, T& s1) {
  const T om = T(6.283185307179586476925) / table[0], var = scale * scale;
  const T q1 = T(20) * scale, q2 = q1 * q1, q = q2 * q2;
  T w1, c1;
  sincos_(om * z0, w1, c1);
  const T d = z1 - w1, dw1 = om * c1;
  const T x0 = z0 * z0, x1 = z1 * z1;
  const T tail = T(0.5) * (x0 * x0 + x1 * x1) / q;
  if (F == VCNF_TARGET_SINUSOIDAL) {
    if (SCORE) {
      s0 = d * dw1 / var - T(2) * (x0 * z0) / q;
      s1 = -d / var - T(2) * (x1 * z1) / q;
    }
    const T u = d / scale;
    return T(-0.5) * u * u - tail;
  }
  const T amp = table[1], x = (z0 - table[2]) / table[3];
  T w, dw;                                             // the second ridge's offset and d w / d z0
  if (F == VCNF_TARGET_SINUSOIDAL_GAP) {
    w = amp * exp_(T(-0.5) * x * x);
    dw = -w * x / table[3];
  } else {
    const T sg = sigmoid_(x);
    w = amp * sg;
    dw = w * (T(1) - sg) / table[3];
  }
  const T dd = d + w, ua = d / scale, ub = dd / scale;
  const T a = T(-0.5) * ua * ua, b = T(-0.5) * ub * ub, t = b - a;
  const T e = exp_(-abs_(t));
  if (SCORE) {
    const T pb = t >= T(0) ? T(1) / (T(1) + e) : e / (T(1) + e), pa = T(1) - pb;
    s0 = (pa * d * dw1 + pb * dd * (dw1 - dw)) / var - T(2) * (x0 * z0) / q;
    s1 = -(pa * d + pb * dd) / var - T(2) * (x1 * z1) / q;
  }
  return (t > T(0) ? b : a) + log1p_(e) - tail;
}

template <typename T, bool SCORE>
__device__ __forceinline__ T smiley(T scale, T z0, T z1, T& s0, T& s1) {
  const T c = T(2) * scale, y = z1 + T(0.8);
  const T r = sqrt_(z0 * z0 + z1 * z1), t = abs_(y);
  const T tr = (r - T(2)) / c, tt = (t - T(1.2)) / c;
  if (SCORE) {
    const T k = -(r - T(2)) / (c * c);
    s0 = k * unit(z0, r);
    s1 = k * unit(z1, r) - sign(y) * (t - T(1.2)) / (c * c);
  }
  return T(-0.5) * tr * tr - T(0.5) * tt * tt;
}

// log p of family F at (z0, z1) and, with SCORE, its score; without SCORE s0, s1 are left alone
template <typename T, int F, bool SCORE>
__device__ __forceinline__ T density(const T* __restrict__ table, int n, T scale, T z0, T z1, T& s0, T& s1) {
  if constexpr (F == VCNF_TARGET_TWO_MOONS) {
    return two_moons<T, SCORE>(z0, z1, s0, s1);
  } else if constexpr (F == VCNF_TARGET_CIRCULAR_GMM || F == VCNF_TARGET_RING_MIXTURE) {
    return mixture<T, F, SCORE>(table, n, scale, z0, z1, s0, s1);
  } else if constexpr (F == VCNF_TARGET_TWO_MODES) {
    return two_modes<T, SCORE>(table, scale, z0, z1, s0, s1);
  } else if constexpr (F == VCNF_TARGET_SMILEY) {
    return smiley<T, SCORE>(scale, z0, z1, s0, s1);
  } else {
    return sinusoidal<T, F, SCORE>(table, scale, z0, z1, s0, s1);
  }
}

// the families, stated once: what both units dispatch on, and what is_family knows
constexpr IntList<VCNF_TARGET_TWO_MOONS, VCNF_TARGET_CIRCULAR_GMM, VCNF_TARGET_RING_MIXTURE, VCNF_TARGET_TWO_MODES,
                  VCNF_TARGET_SINUSOIDAL, VCNF_TARGET_SINUSOIDAL_GAP, VCNF_TARGET_SINUSOIDAL_SPLIT, VCNF_TARGET_SMILEY>
    kFamilies{};
static inline bool is_family(int f) { return in_list(kFamilies, f); }

// the least n_comp of a family - a mixture's components, an energy's constants in `table` - below which a call is a
// shape error; 0: table and n_comp are ignored; -1: no such family
static inline int table_min(int f) {
  switch (f) {
    case VCNF_TARGET_TWO_MOONS:
    case VCNF_TARGET_SMILEY: return 0;
    case VCNF_TARGET_CIRCULAR_GMM:
    case VCNF_TARGET_RING_MIXTURE:
    case VCNF_TARGET_TWO_MODES:
    case VCNF_TARGET_SINUSOIDAL: return 1;
    case VCNF_TARGET_SINUSOIDAL_GAP:
    case VCNF_TARGET_SINUSOIDAL_SPLIT: return 4;
    default: return -1;
  }
}
static inline bool has_table(int f) { return table_min(f) > 0; }

}  // namespace vcnf_target
