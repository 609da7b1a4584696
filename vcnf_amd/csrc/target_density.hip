// Target densities of the reverse-KL drivers for MI355X (gfx950, wave64): the three 2-D targets of normflow 1.2
// (distributions/target.py) - TwoMoons, the circular Gaussian mixture and the ring mixture - with their score
// d logp / d z from the same launch.  With r = sqrt(z0^2 + z1^2) and a = |z0|:
//   TwoMoons          logp = -((r - 2) / 0.2)^2 / 2 - ((a - 2) / 0.3)^2 / 2 + log1p(exp(-4 a / 0.09))
//   circular mixture  d_i = |z - c_i|^2 / (2 s^2),  logp = -log(2 pi s^2 n) + logsumexp_i(-d_i),  c = table [n, 2]
//   ring mixture      d_i = (r - t_i)^2 / (2 s^2),  logp = logsumexp_i(-d_i),                     t = table [n]
// The caller computes the table (no sin / cos in a kernel).
//
// The kernel is a stream over [B, 2]: one sample per lane, its row one 8-byte (fp32) or 16-byte (fp64) access when the
// buffers are aligned to it and two element accesses otherwise, a grid-stride loop under a capped grid.  Every lane
// walks all n components, so the table is read at a wave-uniform index (the compiler reads it through the scalar
// cache; nothing is staged in LDS, and n has no upper limit).  The logsumexp takes two passes over the components:
// the smallest d first, then the sum of exp(d_min - d_i) with the score's weighted sums beside it - nothing of size
// [B, n] exists.  Whether the score is written is a template flag, so the scoreless instance carries none of its
// arithmetic.  Contraction to fused multiply-adds is off in this unit: logp is the same sequence of roundings in the
// instance with the score and in the one without, whatever the compiler shares between logp and the score.
// No atomics, no LDS, no scratch: the same call twice gives the same bits.
#include "stream_common.hpp"

#pragma clang fp contract(off)

namespace vcnf_target {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;

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

// ROW: rows of z and score move as one pack of two elements
template <typename T, int F, bool SCORE, bool ROW>
__global__ __launch_bounds__(kBlock) void target_log_prob_kernel(const T* __restrict__ z, const T* __restrict__ table,
                                                                 T* __restrict__ logp, T* __restrict__ score,
                                                                 long long B, int n, T scale) {
  using RowT = Pack<T, 2>;
  for (long long b = (long long)blockIdx.x * kBlock + threadIdx.x; b < B; b += (long long)gridDim.x * kBlock) {
    RowT x;
    if (ROW) {
      x = reinterpret_cast<const RowT*>(z)[b];
    } else {
      x.v[0] = z[2 * b];
      x.v[1] = z[2 * b + 1];
    }
    RowT s;
    s.v[0] = s.v[1] = T(0);
    T lp = F == VCNF_TARGET_TWO_MOONS ? two_moons<T, SCORE>(x.v[0], x.v[1], s.v[0], s.v[1])
                                      : mixture<T, F, SCORE>(table, n, scale, x.v[0], x.v[1], s.v[0], s.v[1]);
    // a non-finite z has no density: NaN, where the formulas alone give -inf for some infinite rows
    if (!(abs_(x.v[0]) < T(INFINITY) && abs_(x.v[1]) < T(INFINITY))) lp = s.v[0] = s.v[1] = T(NAN);
    logp[b] = lp;
    if (SCORE) {
      if (ROW) {
        reinterpret_cast<RowT*>(score)[b] = s;
      } else {
        score[2 * b] = s.v[0];
        score[2 * b + 1] = s.v[1];
      }
    }
  }
}

// ------------------------------------------------------------------ host side
static inline bool is_mixture(int f) { return f == VCNF_TARGET_CIRCULAR_GMM || f == VCNF_TARGET_RING_MIXTURE; }

template <typename T, int F>
static int launch(const T* z, const T* table, T* logp, T* score, int64_t batch, int32_t n, T scale, hipStream_t st) {
  const bool row = all_aligned({z, score}, 2 * sizeof(T));
  const dim3 grid = grid_for(batch, 1, kBlock, kMaxBlocks);
#define VCNF_TARGET_LAUNCH(SCORE, ROW)                                                                               \
  hipLaunchKernelGGL((target_log_prob_kernel<T, F, SCORE, ROW>), grid, dim3(kBlock), 0, st, z, table, logp, score, \
                     (long long)batch, (int)n, scale)
  if (score) {
    if (row)
      VCNF_TARGET_LAUNCH(true, true);
    else
      VCNF_TARGET_LAUNCH(true, false);
  } else {
    if (row)
      VCNF_TARGET_LAUNCH(false, true);
    else
      VCNF_TARGET_LAUNCH(false, false);
  }
#undef VCNF_TARGET_LAUNCH
  return launched();
}

template <typename T>
static int log_prob(const T* z, const T* table, T* logp, T* score, int64_t batch, int32_t n, int family, T scale,
                    void* stream) {
  if (batch < 0) return VCNF_ERR_SHAPE;
  if (family != VCNF_TARGET_TWO_MOONS && !is_mixture(family)) return VCNF_ERR_UNSUPPORTED;
  if (is_mixture(family) && n < 1) return VCNF_ERR_SHAPE;
  if (batch == 0) return VCNF_OK;
  if (!z || !logp || (is_mixture(family) && !table)) return VCNF_ERR_NULL;
  if (!all_aligned({z, table, logp, score}, sizeof(T))) return VCNF_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  switch (family) {
    case VCNF_TARGET_TWO_MOONS: return launch<T, VCNF_TARGET_TWO_MOONS>(z, nullptr, logp, score, batch, 0, T(0), st);
    case VCNF_TARGET_CIRCULAR_GMM: return launch<T, VCNF_TARGET_CIRCULAR_GMM>(z, table, logp, score, batch, n, scale, st);
    default: return launch<T, VCNF_TARGET_RING_MIXTURE>(z, table, logp, score, batch, n, scale, st);
  }
}

}  // namespace vcnf_target

#define VCNF_TARGET_ENTRY_POINTS(T, SFX)                                                                             \
  extern "C" int vcnf_target_log_prob_##SFX(const T* z, const T* table, T* logp, T* score, int64_t batch,            \
                                            int32_t n_comp, int family, T scale, void* stream) {                     \
    return vcnf_target::log_prob<T>(z, table, logp, score, batch, n_comp, family, scale, stream);                    \
  }

VCNF_TARGET_ENTRY_POINTS(float, f32)
VCNF_TARGET_ENTRY_POINTS(double, f64)
