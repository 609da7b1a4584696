// The stochastic layers of normflow 1.2 (flows/stochastic.py) against the 2-D kernel targets for MI355X (gfx950,
// wave64), fp32 and fp64 from one template: a run of HamiltonianMonteCarlo layers in ONE launch, its VJP, and the
// random walk of a MetropolisHastings layer with a diagonal Gaussian proposal.  Written in torch one HMC layer of L
// leapfrog steps is 2 L autograd.grad calls through target.log_prob, four more log_prob calls and some twenty
// elementwise ops on a few kilobytes; here the sample's row, its momentum, log p and the score stay in the lane's
// registers from the first layer to the last, and a leapfrog point is one fused (log p, score) evaluation of
// target_math.hpp: steps + 1 per layer for the first layer of a run and steps for each later one, since the second
// score of step i is the first of step i + 1 and log p of a layer's output is log p of the next layer's input.
//
// HMC layer k of a run, per sample (step, mass, sqrt_mass are rows [2] of the [K, 2] operands, noise [K, B, 2] and
// unif [K, B] the draws; nothing random is drawn here):
//   p = noise sqrt_mass,  z_new = z,  p_new = p
//   steps times:  p_half = p_new - (step / 2) (-score(z_new)),  z_new = z_new + step (p_half / mass),
//                 p_new = p_half - (step / 2) (-score(z_new))
//   prob = exp(logp(z_new) - logp(z) - sum(p_new^2 / mass) / 2 + sum(p^2 / mass) / 2)
//   accept = unif < prob (a NaN prob rejects),  z_out = accept ? z_new : z (a rejected row keeps its bits),
//   log_det += logp(z) - logp(z_out)
// A non-finite row has NaN log p and score (the targets' rule), so it is rejected and its log_det is NaN.
//
// VJP.  The reference detaches the score and the decision has no derivative, so given the scores the leapfrog is affine
// in z and the cotangents have a closed form that needs no stored trajectory: with a the decision, gz and gl the
// cotangents of z_out and log_det, G = a (gz - gl score(z_new)) is the cotangent of z_new and
//   g_z = (1 - a) gz + G + a gl score(z)
//   g_step      = G sum_i [p_half_i / mass + (step / mass) ((steps - i) s_i + (steps - 1 - i) s_{i+1}) / 2]
//   g_mass      = -G step sum_i p_half_i / mass^2
//   g_sqrt_mass = steps G (step / mass) noise
// where s_i is the score before step i.  One launch walks the layers last to first: per layer it reads the layer's
// entrance row (trace) and decision, recomputes the trajectory once in the forward direction with the sums above beside
// it, and hands g_z on as the next layer's gz.  The layer's six parameter terms are summed over the lanes of a wave
// (butterfly), over the waves through LDS in ascending order, and added to the workgroup's own block [K, 3, 2] of the
// workspace; a second launch (reduce_partials) adds the blocks in a fixed order.
//
// Annealed run (Hamiltonian annealed importance sampling): layer k's density is the LinearInterpolation of the target
// and a 2-D diagonal Gaussian prior, beta [K] the layers' weights and loc, log_scale [2] the prior's parameters:
//   sig = exp(log_scale),  u = (x - loc) / sig,  l0 = -log(2 pi) - (ls_0 + ls_1) - (u_0^2 + u_1^2) / 2,  s0 = -u / sig
//   logp_k = beta_k logp + (1 - beta_k) l0,   score_k = beta_k score + (1 - beta_k) s0
// The same kernels with another policy (Plain, Annealed below): the leapfrog, the decision, log_det and the VJP's sums
// are stated once and read logp_k, score_k where the plain run reads the target's.  What a lane carries from layer to
// layer is the target's (logp, score) alone - the prior's part is a handful of flops, recomputed at the layer's entrance
// - so a run of K layers still costs K steps + 1 target evaluations per sample; the carried logp at z_out is an output
// (logp_target), the last term of the sampler's weights.  beta and the prior's parameters are constants of the VJP.
//
// MH walk, per step (eps [S, B, 2] and w [S, B] the draws, prop_scale [2] the proposal's standard deviations):
//   z_ = eps prop_scale + z,  accept = w <= min(exp(logp(z_) - logp(z)), 1) (NaN rejects),  z = accept ? z_ : z
// with logp(z) carried from step to step: steps + 1 evaluations.
//
// All kernels are streams over [B, 2] like target_density.hip: one sample per lane, a row one 8-byte (fp32) or 16-byte
// (fp64) access when the row buffers are aligned to it and two element accesses otherwise, a grid-stride loop under a
// capped grid.  Every loop is bounded by a host argument (n_layers, steps, n_comp) that the entry point validates;
// none depends on data.  No atomics, no scratch; LDS only for the VJP's sums over the waves.  The same call twice gives
// the same bits.  Contraction to fused multiply-adds is off, as in target_density.hip: log p at a point has the bits
// that unit gives.
#include "stream_common.hpp"

#pragma clang fp contract(off)

#include "target_math.hpp"

namespace vcnf_stoch {

using namespace vcnf_stream;
using vcnf_target::is_family;
using vcnf_target::has_table;
using vcnf_target::table_min;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxBlocks = 2048;
constexpr int kMaxBwdGroups = 1024;
// the two above are what the caller sizes the VJP's workspace by: the header states them (tests/grid_caps.py reads the
// numerals here, so they stay numerals and the compiler holds them to the header's names)
static_assert(kBlock == VCNF_HMC_BLOCK && kMaxBwdGroups == VCNF_HMC_MAX_BWD_GROUPS, "include/vcnf_hip.h states these");
constexpr long long kMaxPoints = VCNF_STOCH_MAX_POINTS;   // n_layers (steps + 1) of one call
constexpr int kTerms = 6;                     // g_step, g_mass, g_sqrt_mass of a layer: [3, 2]

typedef unsigned char byte_t;

template <typename T>
struct Target {
  const T* table;
  int n;
  T scale;
};

// log p and, with SCORE, the score at (z0, z1) with the targets' rule for a non-finite row; without SCORE none of the
// score's arithmetic is instantiated and s0, s1 are left alone (log p has the same bits either way)
template <typename T, int F, bool SCORE>
__device__ __forceinline__ T point(const Target<T>& t, T z0, T z1, T& s0, T& s1) {
  if (SCORE) s0 = s1 = T(0);
  T lp = vcnf_target::density<T, F, SCORE>(t.table, t.n, t.scale, z0, z1, s0, s1);
  if (!(abs_(z0) < T(INFINITY) && abs_(z1) < T(INFINITY))) {
    lp = T(NAN);
    if (SCORE) s0 = s1 = T(NAN);
  }
  return lp;
}

template <typename T, bool ROW>
__device__ __forceinline__ Pack<T, 2> load_row(const T* __restrict__ p, long long row) {
  Pack<T, 2> x;
  if (ROW) {
    x = reinterpret_cast<const Pack<T, 2>*>(p)[row];
  } else {
    x.v[0] = p[2 * row];
    x.v[1] = p[2 * row + 1];
  }
  return x;
}

template <typename T, bool ROW>
__device__ __forceinline__ void store_row(T* __restrict__ p, long long row, const Pack<T, 2>& x) {
  if (ROW) {
    reinterpret_cast<Pack<T, 2>*>(p)[row] = x;
  } else {
    p[2 * row] = x.v[0];
    p[2 * row + 1] = x.v[1];
  }
}

// ------------------------------------------------------------------ the density of a layer
// The policy of an HMC kernel says what layer k's (log p, score) are at a point where the target's are known.  Its Mix
// is made once per lane, set to a layer with layer(k), and turns the target's values at (x0, x1) into the layer's in
// place; logp_target(b, lt) receives the target's log p at a sample's last row.
template <typename T>
struct Plain {                              // the target's own: nothing is instantiated
  struct Mix {
    __device__ explicit Mix(const Plain&) {}
    __device__ void layer(const Plain&, int) {}
    __device__ void operator()(T, T, T&, T&, T&) const {}
  };
  __device__ void logp_target(long long, T) const {}
};

template <typename T>
struct Annealed {                           // the LinearInterpolation of the target and a diagonal Gaussian prior
  const T *beta, *loc, *log_scale;          // [K], [2], [2]
  T* lt_out;                                // [B] or NULL (the VJP has none)
  struct Mix {
    T loc0, loc1, ls, sig0, sig1, beta, rest;
    __device__ explicit Mix(const Annealed& p)
        : loc0(p.loc[0]), loc1(p.loc[1]), ls(p.log_scale[0] + p.log_scale[1]), sig0(exp_(p.log_scale[0])),
          sig1(exp_(p.log_scale[1])), beta(T(1)), rest(T(0)) {}
    __device__ void layer(const Annealed& p, int k) {
      beta = p.beta[k];
      rest = T(1) - beta;
    }
    __device__ void operator()(T x0, T x1, T& lp, T& s0, T& s1) const {
      const T u0 = (x0 - loc0) / sig0, u1 = (x1 - loc1) / sig1;
      const T l0 = T(-1.8378770664093454836) - ls - T(0.5) * (u0 * u0 + u1 * u1);       // -log(2 pi)
      lp = beta * lp + rest * l0;           // a non-finite row's NaN log p and score stay NaN
      s0 = beta * s0 + rest * (-u0 / sig0);
      s1 = beta * s1 + rest * (-u1 / sig1);
    }
  };
  __device__ void logp_target(long long b, T lt) const {
    if (lt_out) lt_out[b] = lt;
  }
};

// ------------------------------------------------------------------ HMC run, forward
template <typename T, typename P>
struct HmcArgs {
  Target<T> t;
  P policy;
  const T *z, *noise, *unif, *step, *mass, *sqm;
  T *out, *logdet, *trace;
  byte_t* accept;
  long long B;
  int K, steps;
};

// lt, c0, c1: the target's log p and score at the sample's row, carried from layer to layer; lp, s0, s1 the layer's
// own there (the same registers under Plain)
template <typename T, int F, bool ROW, typename P>
__global__ __launch_bounds__(kBlock) void hmc_fwd_kernel(const HmcArgs<T, P> a) {
  typename P::Mix mix(a.policy);
  for (long long b = (long long)blockIdx.x * kBlock + threadIdx.x; b < a.B; b += (long long)gridDim.x * kBlock) {
    Pack<T, 2> z = load_row<T, ROW>(a.z, b);
    T c0, c1;
    T lt = point<T, F, true>(a.t, z.v[0], z.v[1], c0, c1);
    T ld = T(0);
    for (int k = 0; k < a.K; ++k) {
      const long long at = (long long)k * a.B + b;
      const T h0 = a.step[2 * k], h1 = a.step[2 * k + 1], m0 = a.mass[2 * k], m1 = a.mass[2 * k + 1];
      const Pack<T, 2> e = load_row<T, ROW>(a.noise, at);
      const T u = a.unif[at];
      if (a.trace) store_row<T, ROW>(a.trace, at, z);
      mix.layer(a.policy, k);
      T lp = lt, s0 = c0, s1 = c1;
      mix(z.v[0], z.v[1], lp, s0, s1);
      const T p0 = e.v[0] * a.sqm[2 * k], p1 = e.v[1] * a.sqm[2 * k + 1];
      T x0 = z.v[0], x1 = z.v[1], r0 = p0, r1 = p1, t0 = s0, t1 = s1, lpn = lp;
      T ltn = lt, d0 = c0, d1 = c1;                    // the target's at the trajectory's point
      for (int i = 0; i < a.steps; ++i) {
        const T q0 = r0 - (h0 / T(2)) * -t0, q1 = r1 - (h1 / T(2)) * -t1;
        x0 = x0 + h0 * (q0 / m0);
        x1 = x1 + h1 * (q1 / m1);
        ltn = point<T, F, true>(a.t, x0, x1, d0, d1);
        lpn = ltn, t0 = d0, t1 = d1;
        mix(x0, x1, lpn, t0, t1);
        r0 = q0 - (h0 / T(2)) * -t0;
        r1 = q1 - (h1 / T(2)) * -t1;
      }
      const T prob = exp_(lpn - lp - T(0.5) * (r0 * r0 / m0 + r1 * r1 / m1) + T(0.5) * (p0 * p0 / m0 + p1 * p1 / m1));
      const bool acc = u < prob;
      ld += lp - (acc ? lpn : lp);
      z.v[0] = acc ? x0 : z.v[0];
      z.v[1] = acc ? x1 : z.v[1];
      c0 = acc ? d0 : c0;
      c1 = acc ? d1 : c1;
      lt = acc ? ltn : lt;
      if (a.accept) a.accept[at] = acc ? 1 : 0;
    }
    store_row<T, ROW>(a.out, b, z);
    a.logdet[b] = ld;
    a.policy.logp_target(b, lt);
  }
}

// ------------------------------------------------------------------ HMC run, VJP
template <typename T, typename P>
struct HmcBwdArgs {
  Target<T> t;
  P policy;
  const T *trace, *noise, *step, *mass, *sqm, *gout, *gld;
  const byte_t* accept;
  T *gin, *partials;
  long long B, tiles;
  int K, steps;
};

template <typename T, int F, bool ROW, typename P>
__global__ __launch_bounds__(kBlock) void hmc_bwd_kernel(const HmcBwdArgs<T, P> a) {
  __shared__ T red[2][kWaves][kTerms];
  typename P::Mix mix(a.policy);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  T* const block = a.partials + (long long)blockIdx.x * a.K * kTerms;
  int it = 0;                                          // layers visited: its parity picks the LDS buffer
  bool first = true;
  // every lane of the workgroup walks every tile (barriers inside); a lane past the batch adds zeros
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x, first = false) {
    const long long b = tile * kBlock + threadIdx.x;
    const bool live = b < a.B;
    Pack<T, 2> gz;
    gz.v[0] = gz.v[1] = T(0);
    if (live && a.gout) gz = load_row<T, ROW>(a.gout, b);
    const T gl = (live && a.gld) ? a.gld[b] : T(0);
    for (int k = a.K - 1; k >= 0; --k, ++it) {
      T v[kTerms];
#pragma unroll
      for (int j = 0; j < kTerms; ++j) v[j] = T(0);
      if (live) {
        const long long at = (long long)k * a.B + b;
        const T h0 = a.step[2 * k], h1 = a.step[2 * k + 1], m0 = a.mass[2 * k], m1 = a.mass[2 * k + 1];
        const T c0 = h0 / m0, c1 = h1 / m1;
        const Pack<T, 2> z = load_row<T, ROW>(a.trace, at);
        const Pack<T, 2> e = load_row<T, ROW>(a.noise, at);
        const bool acc = a.accept[at] != 0;
        mix.layer(a.policy, k);
        T t0, t1;
        T lpx = point<T, F, true>(a.t, z.v[0], z.v[1], t0, t1);      // log p: the policy's mix writes it, nothing reads it
        mix(z.v[0], z.v[1], lpx, t0, t1);
        const T sz0 = t0, sz1 = t1;                    // the layer's score at its entrance
        // the forward pass's trajectory again, with the sums of the closed form beside it
        T x0 = z.v[0], x1 = z.v[1], r0 = e.v[0] * a.sqm[2 * k], r1 = e.v[1] * a.sqm[2 * k + 1];
        T w0 = T(0), w1 = T(0);                        // sum_i p_half_i
        T f0 = T(0), f1 = T(0);                        // sum_i ((steps - i) s_i + (steps - 1 - i) s_{i+1}) / 2
        for (int i = 0; i < a.steps; ++i) {
          const T q0 = r0 - (h0 / T(2)) * -t0, q1 = r1 - (h1 / T(2)) * -t1;
          const T n_half = T(a.steps - i), n_next = T(a.steps - 1 - i);
          const T u0 = t0, u1 = t1;
          x0 = x0 + h0 * (q0 / m0);
          x1 = x1 + h1 * (q1 / m1);
          lpx = point<T, F, true>(a.t, x0, x1, t0, t1);
          mix(x0, x1, lpx, t0, t1);
          r0 = q0 - (h0 / T(2)) * -t0;
          r1 = q1 - (h1 / T(2)) * -t1;
          w0 += q0;
          w1 += q1;
          f0 += (n_half * u0 + n_next * t0) / T(2);
          f1 += (n_half * u1 + n_next * t1) / T(2);
        }
        // selects, not products with a: a rejected row - a non-finite one, or one whose leapfrog ran off to inf / NaN,
        // has NaN sums - adds exact zeros to the parameter sums and hands its gz on as it is
        const T G0 = acc ? gz.v[0] - gl * t0 : T(0), G1 = acc ? gz.v[1] - gl * t1 : T(0);
        if (acc) {
          v[0] = G0 * (w0 / m0 + c0 * f0);
          v[1] = G1 * (w1 / m1 + c1 * f1);
          v[2] = -(G0 * h0 * w0) / (m0 * m0);
          v[3] = -(G1 * h1 * w1) / (m1 * m1);
          v[4] = T(a.steps) * G0 * c0 * e.v[0];
          v[5] = T(a.steps) * G1 * c1 * e.v[1];
        }
        gz.v[0] = acc ? G0 + gl * sz0 : gz.v[0];
        gz.v[1] = acc ? G1 + gl * sz1 : gz.v[1];
      }
      // over the lanes of the wave, then over the waves
#pragma unroll
      for (int j = 0; j < kTerms; ++j) v[j] = lanes_sum(v[j], 1, 64);
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kTerms; ++j) red[it & 1][wave][j] = v[j];
      }
      __syncthreads();
      if (threadIdx.x < kTerms) {
        T s = red[it & 1][0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += red[it & 1][w][threadIdx.x];
        T* const dst = block + (long long)k * kTerms + threadIdx.x;
        *dst = first ? s : *dst + s;
      }
    }
    if (live) store_row<T, ROW>(a.gin, b, gz);
  }
}

// element e of the summed block [K, 3, 2] goes to g_step | g_mass | g_sqrt_mass, each [K, 2]
template <typename T>
struct ParamDest {
  T *step, *mass, *sqm;
  __device__ T* operator()(long long e) const {
    const long long k = e / kTerms;
    const int j = (int)(e - k * kTerms);
    return (j < 2 ? step : j < 4 ? mass : sqm) + 2 * k + (j & 1);
  }
};

// ------------------------------------------------------------------ MH walk
template <typename T>
struct MhArgs {
  Target<T> t;
  const T *z, *eps, *w, *prop;
  T* out;
  byte_t* accept;
  long long B;
  int steps;
};

template <typename T, int F, bool ROW>
__global__ __launch_bounds__(kBlock) void mh_walk_kernel(const MhArgs<T> a) {
  const T c0 = a.prop[0], c1 = a.prop[1];
  for (long long b = (long long)blockIdx.x * kBlock + threadIdx.x; b < a.B; b += (long long)gridDim.x * kBlock) {
    Pack<T, 2> z = load_row<T, ROW>(a.z, b);
    T s0 = T(0), s1 = T(0);                          // not computed: the walk needs log p alone
    T lp = point<T, F, false>(a.t, z.v[0], z.v[1], s0, s1);
    for (int i = 0; i < a.steps; ++i) {
      const long long at = (long long)i * a.B + b;
      const Pack<T, 2> e = load_row<T, ROW>(a.eps, at);
      const T x0 = e.v[0] * c0 + z.v[0], x1 = e.v[1] * c1 + z.v[1];
      const T lpn = point<T, F, false>(a.t, x0, x1, s0, s1);
      const T ratio = exp_(lpn - lp);
      const bool acc = a.w[at] <= (ratio > T(1) ? T(1) : ratio);       // a NaN ratio stays NaN and rejects
      z.v[0] = acc ? x0 : z.v[0];
      z.v[1] = acc ? x1 : z.v[1];
      lp = acc ? lpn : lp;
      if (a.accept) a.accept[at] = acc ? 1 : 0;
    }
    store_row<T, ROW>(a.out, b, z);
  }
}

// ------------------------------------------------------------------ host side
// what every entry point checks before it looks at a pointer
static int check_run(int64_t batch, int32_t n_layers, int32_t steps, int32_t n_comp, int family) {
  if (batch < 0 || n_layers < 1 || steps < 0) return VCNF_ERR_SHAPE;
  if (!is_family(family)) return VCNF_ERR_UNSUPPORTED;
  if (has_table(family) && n_comp < table_min(family)) return VCNF_ERR_SHAPE;
  if ((long long)n_layers * ((long long)steps + 1) > kMaxPoints) return VCNF_ERR_UNSUPPORTED;
  return VCNF_OK;
}

static long long sample_tiles(int64_t batch) { return (batch + kBlock - 1) / kBlock; }

// launch(F, ROW): the family and whether rows move as one pack, as constants
template <typename L>
static int with_family_row(int family, bool row, L&& launch) {
  return launch_listed(vcnf_target::kFamilies, family,
                       [&](auto F) { return with_flags([&](auto ROW) { return launch(F, ROW); }, row); });
}

template <typename T>
static Target<T> target_of(const T* table, int32_t n_comp, int family, T scale) {
  return has_table(family) ? Target<T>{table, (int)n_comp, scale} : Target<T>{nullptr, 0, scale};
}

// a policy's part of the entry points' checks: its required pointers, and all of its pointers' alignment
template <typename T>
static bool complete(const Plain<T>&) { return true; }
template <typename T>
static bool complete(const Annealed<T>& p) { return p.beta && p.loc && p.log_scale; }
template <typename T>
static bool policy_aligned(const Plain<T>&) { return true; }
template <typename T>
static bool policy_aligned(const Annealed<T>& p) { return all_aligned({p.beta, p.loc, p.log_scale, p.lt_out}, sizeof(T)); }

template <typename T, typename P>
static int hmc_stack(const P& policy, const T* z, const T* noise, const T* unif, const T* step, const T* mass, const T* sqm,
                     const T* table, T* out, T* logdet, T* trace, byte_t* accept, int64_t batch, int32_t n_layers,
                     int32_t steps, int32_t n_comp, int family, T scale, void* stream) {
  if (const int st = check_run(batch, n_layers, steps, n_comp, family)) return st;
  if (batch == 0) return VCNF_OK;
  if (!z || !noise || !unif || !step || !mass || !sqm || !out || !logdet || (has_table(family) && !table) || !complete(policy))
    return VCNF_ERR_NULL;
  if (!all_aligned({z, noise, unif, step, mass, sqm, table, out, logdet, trace}, sizeof(T)) || !policy_aligned(policy))
    return VCNF_ERR_ALIGN;
  const HmcArgs<T, P> a{target_of(table, n_comp, family, scale), policy, z, noise, unif, step, mass, sqm, out, logdet, trace,
                        accept, batch, n_layers, steps};
  const bool row = all_aligned({z, noise, out, trace}, 2 * sizeof(T));
  return with_family_row(family, row, [&](auto F, auto ROW) {
    hipLaunchKernelGGL((hmc_fwd_kernel<T, F(), ROW()>), grid_for(batch, 1, kBlock, kMaxBlocks), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return launched();
  });
}

template <typename T, typename P>
static int hmc_stack_bwd(const P& policy, const T* trace, const byte_t* accept, const T* noise, const T* step, const T* mass,
                         const T* sqm, const T* table, const T* gout, const T* gld, T* gin, T* g_step, T* g_mass, T* g_sqm,
                         T* workspace, int64_t batch, int32_t n_layers, int32_t steps, int32_t groups, int32_t n_comp,
                         int family, T scale, void* stream) {
  if (const int st = check_run(batch, n_layers, steps, n_comp, family)) return st;
  if (batch == 0) return VCNF_OK;
  // one block of the workspace per workgroup, and every workgroup has a tile to write its block for
  if (groups < 1 || groups > kMaxBwdGroups || groups > sample_tiles(batch)) return VCNF_ERR_SHAPE;
  if (!trace || !accept || !noise || !step || !mass || !sqm || !gin || !g_step || !g_mass || !g_sqm || !workspace ||
      (has_table(family) && !table) || !complete(policy))
    return VCNF_ERR_NULL;
  if (!all_aligned({trace, noise, step, mass, sqm, table, gout, gld, gin, g_step, g_mass, g_sqm, workspace}, sizeof(T)) ||
      !policy_aligned(policy))
    return VCNF_ERR_ALIGN;
  const HmcBwdArgs<T, P> a{target_of(table, n_comp, family, scale), policy, trace, noise, step, mass, sqm, gout, gld, accept, gin,
                        workspace, batch, sample_tiles(batch), n_layers, steps};
  const bool row = all_aligned({trace, noise, gout, gin}, 2 * sizeof(T));
  const int rc = with_family_row(family, row, [&](auto F, auto ROW) {
    hipLaunchKernelGGL((hmc_bwd_kernel<T, F(), ROW()>), dim3((unsigned)groups), dim3(kBlock), 0, (hipStream_t)stream, a);
    return launched();
  });
  if (rc) return rc;
  return launch_reduce_partials(workspace, (long long)groups, (long long)n_layers * kTerms, ParamDest<T>{g_step, g_mass, g_sqm},
                                stream);
}

template <typename T>
static int mh_walk(const T* z, const T* eps, const T* w, const T* prop, const T* table, T* out, byte_t* accept,
                   int64_t batch, int32_t steps, int32_t n_comp, int family, T scale, void* stream) {
  if (const int st = check_run(batch, 1, steps, n_comp, family)) return st;
  if (batch == 0) return VCNF_OK;
  if (!z || !prop || !out || (steps > 0 && (!eps || !w)) || (has_table(family) && !table)) return VCNF_ERR_NULL;
  if (!all_aligned({z, eps, w, prop, table, out}, sizeof(T))) return VCNF_ERR_ALIGN;
  const MhArgs<T> a{target_of(table, n_comp, family, scale), z, eps, w, prop, out, accept, batch, steps};
  const bool row = all_aligned({z, eps, out}, 2 * sizeof(T));
  return with_family_row(family, row, [&](auto F, auto ROW) {
    hipLaunchKernelGGL((mh_walk_kernel<T, F(), ROW()>), grid_for(batch, 1, kBlock, kMaxBlocks), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return launched();
  });
}

}  // namespace vcnf_stoch

#define VCNF_STOCH_ENTRY_POINTS(T, SFX)                                                                                \
  extern "C" int vcnf_hmc_stack_##SFX(const T* z, const T* noise, const T* unif, const T* step, const T* mass,         \
                                      const T* sqrt_mass, const T* table, T* z_out, T* log_det, T* trace,              \
                                      uint8_t* accept, int64_t batch, int32_t n_layers, int32_t steps, int32_t n_comp, \
                                      int family, T scale, void* stream) {                                             \
    return vcnf_stoch::hmc_stack(vcnf_stoch::Plain<T>{}, z, noise, unif, step, mass, sqrt_mass, table, z_out, log_det, \
                                 trace, accept, batch, n_layers, steps, n_comp, family, scale, stream);                \
  }                                                                                                                    \
  extern "C" int vcnf_hmc_annealed_stack_##SFX(                                                                        \
      const T* z, const T* noise, const T* unif, const T* step, const T* mass, const T* sqrt_mass, const T* beta,      \
      const T* prior_loc, const T* prior_log_scale, const T* table, T* z_out, T* log_det, T* logp_target, T* trace,    \
      uint8_t* accept, int64_t batch, int32_t n_layers, int32_t steps, int32_t n_comp, int family, T scale,            \
      void* stream) {                                                                                                  \
    return vcnf_stoch::hmc_stack(vcnf_stoch::Annealed<T>{beta, prior_loc, prior_log_scale, logp_target}, z, noise,     \
                                 unif, step, mass, sqrt_mass, table, z_out, log_det, trace, accept, batch, n_layers,   \
                                 steps, n_comp, family, scale, stream);                                                \
  }                                                                                                                    \
  extern "C" int vcnf_hmc_stack_bwd_##SFX(const T* trace, const uint8_t* accept, const T* noise, const T* step,        \
                                          const T* mass, const T* sqrt_mass, const T* table, const T* g_out,           \
                                          const T* g_logdet, T* g_in, T* g_step, T* g_mass, T* g_sqrt_mass,            \
                                          T* workspace, int64_t batch, int32_t n_layers, int32_t steps,                \
                                          int32_t groups, int32_t n_comp, int family, T scale, void* stream) {         \
    return vcnf_stoch::hmc_stack_bwd(vcnf_stoch::Plain<T>{}, trace, accept, noise, step, mass, sqrt_mass, table,       \
                                     g_out, g_logdet, g_in, g_step, g_mass, g_sqrt_mass, workspace, batch, n_layers,   \
                                     steps, groups, n_comp, family, scale, stream);                                    \
  }                                                                                                                    \
  extern "C" int vcnf_hmc_annealed_stack_bwd_##SFX(                                                                    \
      const T* trace, const uint8_t* accept, const T* noise, const T* step, const T* mass, const T* sqrt_mass,         \
      const T* beta, const T* prior_loc, const T* prior_log_scale, const T* table, const T* g_out, const T* g_logdet,  \
      T* g_in, T* g_step, T* g_mass, T* g_sqrt_mass, T* workspace, int64_t batch, int32_t n_layers, int32_t steps,     \
      int32_t groups, int32_t n_comp, int family, T scale, void* stream) {                                             \
    return vcnf_stoch::hmc_stack_bwd(vcnf_stoch::Annealed<T>{beta, prior_loc, prior_log_scale, nullptr}, trace,        \
                                     accept, noise, step, mass, sqrt_mass, table, g_out, g_logdet, g_in, g_step,       \
                                     g_mass, g_sqrt_mass, workspace, batch, n_layers, steps, groups, n_comp, family,   \
                                     scale, stream);                                                                   \
  }                                                                                                                    \
  extern "C" int vcnf_mh_walk_##SFX(const T* z, const T* eps, const T* w, const T* prop_scale, const T* table,         \
                                    T* z_out, uint8_t* accept, int64_t batch, int32_t steps, int32_t n_comp,           \
                                    int family, T scale, void* stream) {                                               \
    return vcnf_stoch::mh_walk<T>(z, eps, w, prop_scale, table, z_out, accept, batch, steps, n_comp, family, scale,    \
                                  stream);                                                                             \
  }

VCNF_STOCH_ENTRY_POINTS(float, f32)
VCNF_STOCH_ENTRY_POINTS(double, f64)

