// Target densities of the reverse-KL drivers for MI355X (gfx950, wave64): the three 2-D targets of normflow 1.2
// (distributions/target.py) - TwoMoons, the circular Gaussian mixture and the ring mixture - with their score
// d logp / d z from the same launch.  With r = sqrt(z0^2 + z1^2) and a = |z0|:
//   TwoMoons          logp = -((r - 2) / 0.2)^2 / 2 - ((a - 2) / 0.3)^2 / 2 + log1p(exp(-4 a / 0.09))
//   circular mixture  d_i = |z - c_i|^2 / (2 s^2),  logp = -log(2 pi s^2 n) + logsumexp_i(-d_i),  c = table [n, 2]
//   ring mixture      d_i = (r - t_i)^2 / (2 s^2),  logp = logsumexp_i(-d_i),                     t = table [n]
// The caller computes a mixture's table (no sin / cos in a mixture's kernel).  The same kernel evaluates the five energy
// densities of distributions/prior.py - TwoModes, Sinusoidal, Sinusoidal_gap, Sinusoidal_split, Smiley - whose table
// holds their constants ({loc}, {period}, {period, amp, mu, width}, none) and whose formulas stand in target_math.hpp;
// the Sinusoidal trio calls sincos once per point.  The device functions are target_math.hpp's, shared with
// stochastic.hip.
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

#include "target_math.hpp"

namespace vcnf_target {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;

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
    T lp = density<T, F, SCORE>(table, n, scale, x.v[0], x.v[1], s.v[0], s.v[1]);
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
template <typename T>
static int log_prob(const T* z, const T* table, T* logp, T* score, int64_t batch, int32_t n, int family, T scale,
                    void* stream) {
  if (batch < 0) return VCNF_ERR_SHAPE;
  if (!is_family(family)) return VCNF_ERR_UNSUPPORTED;
  if (has_table(family) && n < table_min(family)) return VCNF_ERR_SHAPE;
  if (batch == 0) return VCNF_OK;
  if (!z || !logp || (has_table(family) && !table)) return VCNF_ERR_NULL;
  if (!all_aligned({z, table, logp, score}, sizeof(T))) return VCNF_ERR_ALIGN;
  if (!has_table(family)) table = nullptr, n = 0;      // ignored by the family: never read
  const dim3 grid = grid_for(batch, 1, kBlock, kMaxBlocks);
  return launch_listed(kFamilies, family, [&](auto F) {
    return with_flags([&](auto SCORE, auto ROW) {
      hipLaunchKernelGGL((target_log_prob_kernel<T, F(), SCORE(), ROW()>), grid, dim3(kBlock), 0, (hipStream_t)stream, z,
                         table, logp, score, (long long)batch, (int)n, scale);
      return launched();
    }, score != nullptr, all_aligned({z, score}, 2 * sizeof(T)));
  });
}

}  // namespace vcnf_target

#define VCNF_TARGET_ENTRY_POINTS(T, SFX)                                                                             \
  extern "C" int vcnf_target_log_prob_##SFX(const T* z, const T* table, T* logp, T* score, int64_t batch,            \
                                            int32_t n_comp, int family, T scale, void* stream) {                     \
    return vcnf_target::log_prob<T>(z, table, logp, score, batch, n_comp, family, scale, stream);                    \
  }

VCNF_TARGET_ENTRY_POINTS(float, f32)
VCNF_TARGET_ENTRY_POINTS(double, f64)
