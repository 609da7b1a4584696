// Rational-quadratic spline in double precision: the elementwise spline of vcnf_rqs_elementwise_f32 (and, with strided
// logit rows, of vcnf_rqs_elementwise_strided_f32 / vcnf_rqs_packed_bwd_f32 for image couplings) for models
// converted with .double() (the reference's drivers do: /root/reference run.py:114, runadultvdeq.py:183; its Flow
// contract is dtype-agnostic).  One thread per element, the reference's operation order as written in
// normflow/utils/splines.py:20-85 (tails) and :88-193 (spline): softmax -> floor -> cumsum -> affine map -> exact end
// knots -> sizes by differencing; compare-and-count bin search with the last knot bumped by 1e-6; the stable root form
// 2c / (-b - sqrt(disc)).  Library exp / log / sqrt in fp64: this path is for parity with fp64 models, not for speed
// (fp64 vector rate is 1/2 .. 1/4 of fp32 and nothing here is tuned); the hot path is fp32.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <array>

#include "../../include/vcnf_hip.h"
#include "host_common.hpp"
#include "rqs_host.hpp"
#include "rqs_math64.hpp"
#include "rqs_vjp.hpp"

namespace vcnf {

constexpr int kMaxBins64 = 64;

struct Rqs64Args {
  const double *x, *uw, *uh, *ud;
  long long ld_w, ld_h, ld_d;
  double *y, *lad;
  long long n;
  int inverse;
  Rqs64Const c;
  int32_t* bad;
  long long inner, ks, period;     // strided addressing only (see rows64)
  LimitsT<double> lim;             // LIM kernels only: per-element interval limits (left, right, bottom, top)
};

// Offsets of element i's logit rows.  Dense (vcnf_rqs_elementwise_f64): row i at i * ld, logit k at + k.  Strided
// (vcnf_rqs_elementwise_strided_f64, as vcnf_rqs_elementwise_strided_f32): r = period > 0 ? i % period : i,
// outer = r / inner, s = r % inner; row at outer * ld + s, logit k at + k * ks (ld_* are the per-row strides).
struct Rows64 {
  long long w, h, d, ks;
};

template <bool STRIDED>
__device__ __forceinline__ Rows64 rows64(const Rqs64Args& a, long long i) {
  if (!STRIDED) return Rows64{i * a.ld_w, i * a.ld_h, i * a.ld_d, 1};
  const long long r = a.period > 0 ? i % a.period : i;
  const long long outer = a.inner == 1 ? r : r / a.inner, s = r - outer * a.inner;
  return Rows64{outer * a.ld_w + s, outer * a.ld_h + s, outer * a.ld_d + s, a.ks};
}

static dim3 grid64(int64_t n) { return dim3(elem_blocks(n, 256, 256 * 32)); }

// The selection of an element's bin and the bin's map in either direction are rqs_math64.hpp's (rqs_locate64,
// rqs_bin_eval64), shared with made_sample.hip.
// KT > 0: compile-time bin count, every array in registers (K = 8, 10, 16); KT == 0: any K up to 64 (runtime-indexed
// arrays in scratch).  Both instances evaluate the same expressions in the same order.  LIM (dense rows, no tails): the
// interval of element i comes from a.lim (tensor limits, splines.py:99-102).
template <int KT, bool STRIDED, bool LIM = false>
__global__ __launch_bounds__(256) void rqs_elementwise_f64_kernel(const Rqs64Args a) {
  constexpr int KA = KT > 0 ? KT : kMaxBins64;
  const Rqs64Const& c = a.c;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long long)gridDim.x * blockDim.x) {
    const double x = a.x[i];
    double out = x, lad = 0.0;                                            // splines.py:30-49: identity outside
    if (c.tails == VCNF_TAILS_NONE || (x >= c.left && x <= c.right)) {
      double lv[4] = {c.left, c.right, c.bottom, c.top};
      if (LIM) a.lim.load(i, lv);
      const Rows64 rw = rows64<STRIDED>(a, i);
      double xk[KA + 1], yk[KA + 1];
      RqsBin64 b;
      rqs_locate64<KT>(x, a.inverse, a.uw + rw.w, a.uh + rw.h, a.ud + rw.d, rw.ks, c, lv[0], lv[1], lv[2], lv[3], xk, yk,
                       b);
      bool bad = false;
      if (a.inverse) rqs_bin_eval64<true>(x, b, out, lad, bad);
      else rqs_bin_eval64<false>(x, b, out, lad, bad);
      if (bad && a.bad) atomicAdd(a.bad, 1);                              // :164 (the reference asserts)
    }
    a.y[i] = out;
    a.lad[i] = lad;
  }
}

template <bool STRIDED, bool LIM = false>
static int launch_fwd64(const Rqs64Args& a, void* stream) {
  with_bins(kBins64, a.c.K, [&](auto kt) {
    hipLaunchKernelGGL((rqs_elementwise_f64_kernel<decltype(kt)::value, STRIDED, LIM>), grid64(a.n), dim3(256), 0,
                       (hipStream_t)stream, a);
  });
  return launched();
}


// ------------------------------------------------------------------ VJP (training path of .double() models)
// The adjoint of rqs_elementwise_f64_kernel, as rqs_backward.hip does it in fp32: the element is re-evaluated with
// the forward kernel's own knot / bin / padding functions, then walked backwards - bin map (rqs_vjp.hpp) -> knots ->
// cumulative widths (end knots are constants) -> the floor's (1 - min K) factor -> softmax -> wh_scale; the two knot
// derivatives through softplus.  The sampling direction differentiates the closed-form root implicitly in bin
// coordinates; in fp64 that root is exact enough that the fp32 kernel's Newton refinement is not needed.
struct Rqs64BwdArgs {
  Rqs64Args f;                     // forward operands (y, lad, bad unused)
  const double *gy, *glad;
  double *gx, *guw, *guh, *gud;    // dense: gradient rows of K, K, nd; strided: the layout of the logits (rows64)
  int nd;
  long long lad_div;               // strided: g_logabsdet read at i / lad_div (dense: at i)
  double* glim[4];                 // LIM: per-element gradients of the limits (NULL: not wanted)
};

// KT > 0: the K probabilities and K+1 knots of each side live in registers (loops of constant trip count, fully
// unrolled by the compiler: compile-time indices;
// the bin's values are picked by comparison, never by a runtime index).  KT == 0 (any other K up to 64): the same
// code with runtime-indexed arrays, which go to scratch.
// LIM (dense rows, no tails): per-element limits as in the forward kernel, plus their per-element gradients.
template <int KT, bool INV, bool STRIDED, bool LIM = false>
__global__ __launch_bounds__(256) void rqs_elementwise_bwd_f64_kernel(const Rqs64BwdArgs g) {
  const Rqs64Args& a = g.f;
  const Rqs64Const& c = a.c;
  constexpr int KA = KT > 0 ? KT : kMaxBins64;
  const int K = KT > 0 ? KT : c.K;
  const int nd = g.nd;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long long)gridDim.x * blockDim.x) {
    const double x = a.x[i];
    const double gy = g.gy[i], gl = g.glad[STRIDED && g.lad_div != 1 ? i / g.lad_div : i];
    const Rows64 rw = rows64<STRIDED>(a, i);
    const long long ks = rw.ks;
    double* guw = g.guw + (STRIDED ? rw.w : i * K);
    double* guh = g.guh + (STRIDED ? rw.h : i * K);
    double* gud = g.gud + (STRIDED ? rw.d : i * nd);
    if (c.tails != VCNF_TAILS_NONE && !(x >= c.left && x <= c.right)) {   // identity outside: dy/dx = 1
      g.gx[i] = gy;
      for (int k = 0; k < K; ++k) { guw[k * ks] = 0.0; guh[k * ks] = 0.0; }
      for (int k = 0; k < nd; ++k) gud[k * ks] = 0.0;
      continue;
    }
    double lv[4] = {c.left, c.right, c.bottom, c.top};
    if (LIM) a.lim.load(i, lv);
    const double left = lv[0], right = lv[1], bottom = lv[2], top = lv[3];
    double xk[KA + 1], yk[KA + 1], pw[KA], ph[KA];
    constexpr int KF = LIM ? KA + 1 : 1;
    double fx[KF], fy[KF];                           // LIM: cumulative fractions of the knots
    partition64<KT>(a.uw + rw.w, ks, K, c.wh_scale, left, right, c.min_w, xk, pw, LIM ? fx : nullptr);
    partition64<KT>(a.uh + rw.h, ks, K, c.wh_scale, bottom, top, c.min_h, yk, ph, LIM ? fy : nullptr);
    const int bin = bin64<KT>(INV ? yk : xk, K, x);
    RqsBin64 b;
    double xr, yr;
    pick_bin64<KT>(xk, yk, bin, K, b.xl, xr, b.yl, yr);
    b.w = xr - b.xl;
    b.h = yr - b.yl;
    const double* ud = a.ud + rw.d;
    const int j0 = dlogit_col64(bin, K, c.tails), j1 = dlogit_col64(bin + 1, K, c.tails);
    const double l0 = j0 < 0 ? c.edge : ud[j0 * ks], l1 = j1 < 0 ? c.edge : ud[j1 * ks];
    b.d0 = c.min_d + softplus64(l0);
    b.d1 = c.min_d + softplus64(l1);
    BinGradT<double> bg;
    if (!INV) {
      bg = bin_forward_vjp<double>(x, b, gy, gl);
    } else {
      // the forward kernel's root (rqs_root64, splines.py:153-166) at this kernel's s = h * (1 / w), whose rounding
      // its gradients follow; kept in line: see profiles/rqs64_unit.md section 1
      const double rw = 1.0 / b.w;
      const double s = b.h * rw;
      const double dy = x - b.yl;
      const double e = b.d0 + b.d1 - 2.0 * s;
      const double qa = dy * e + b.h * (s - b.d0);
      const double qb = b.h * b.d0 - dy * e;
      const double qc = -s * dy;
      const double r = (2.0 * qc) / (-qb - sqrt(qb * qb - 4.0 * qa * qc));
      bg = bin_inverse_vjp_at_root<double>(r, rw, s, b, gy, gl);
    }
    g.gx[i] = bg.gx;
    // knots -> cumulative widths -> softmax -> logits.  X_bin carries (gxl - gw), X_bin+1 carries gw; the end knots
    // are constants.  dX_k / dW_j = span (1 - min K) for j < k.
    const double gXl = bin >= 1 ? bg.gxl - bg.gw : 0.0, gXr = bin + 1 <= K - 1 ? bg.gw : 0.0;
    const double gYl = bin >= 1 ? bg.gyl - bg.gh : 0.0, gYr = bin + 1 <= K - 1 ? bg.gh : 0.0;
    const double cx = (right - left) * (1.0 - c.min_w * K), cy = (top - bottom) * (1.0 - c.min_h * K);
    double dotw = 0.0, doth = 0.0;
    for (int k = 0; k < K; ++k) {
      dotw += pw[k] * (cx * ((k < bin ? gXl : 0.0) + (k < bin + 1 ? gXr : 0.0)));
      doth += ph[k] * (cy * ((k < bin ? gYl : 0.0) + (k < bin + 1 ? gYr : 0.0)));
    }
    for (int k = 0; k < K; ++k) {
      const double gWk = cx * ((k < bin ? gXl : 0.0) + (k < bin + 1 ? gXr : 0.0));
      const double gHk = cy * ((k < bin ? gYl : 0.0) + (k < bin + 1 ? gYr : 0.0));
      guw[k * ks] = c.wh_scale * pw[k] * (gWk - dotw);
      guh[k * ks] = c.wh_scale * ph[k] * (gHk - doth);
    }
    // derivative logits: d softplus / dv = sigmoid(v) (1 above the threshold 20); circular with one bin: both knots
    // share logit 0 and the two contributions add
    double gd0 = j0 < 0 ? 0.0 : bg.gd0 * (l0 > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-l0)));
    double gd1 = j1 < 0 ? 0.0 : bg.gd1 * (l1 > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-l1)));
    if (j0 == j1) { gd0 += gd1; gd1 = 0.0; }
    for (int k = 0; k < nd; ++k) gud[k * ks] = k == j0 ? gd0 : (k == j1 ? gd1 : 0.0);
    if (LIM) {
      double fx0, fx1, fy0, fy1, gv[4];
      pick_bin64<KT>(fx, fy, bin, K, fx0, fx1, fy0, fy1);
      limit_vjp<double>(bg.gxl - bg.gw, bg.gw, fx0, fx1, gv[0], gv[1]);
      limit_vjp<double>(bg.gyl - bg.gh, bg.gh, fy0, fy1, gv[2], gv[3]);
      for (int j = 0; j < 4; ++j)
        if (g.glim[j]) g.glim[j][i] = gv[j];
    }
  }
}

template <bool STRIDED, bool LIM = false>
static int launch_bwd64(const Rqs64BwdArgs& g, void* stream) {
  with_bins(kBins64, g.f.c.K, [&](auto kt) {
    with_flags([&](auto INVERSE) {
      hipLaunchKernelGGL((rqs_elementwise_bwd_f64_kernel<kt(), INVERSE(), STRIDED, LIM>), grid64(g.f.n), dim3(256), 0,
                         (hipStream_t)stream, g);
    }, g.f.inverse != 0);
  });
  return launched();
}

}  // namespace vcnf

using namespace vcnf;

// The logit rows of an entry point: dense rows (row i at i * ld) unless it sets inner / ks / period (rows64).
struct Logits64 {
  const double *uw, *uh, *ud;
  int64_t ld_w, ld_h, ld_d;
  int64_t inner = 1, ks = 1, period = 0;
};

// The arguments of the forward kernel.  ``lim``: the per-element limits of the LIM kernels.  The VJP leaves the outputs
// of the forward map out.
static Rqs64Args fwd_args64(const vcnf_rqs_cfg_f64* cfg, int inverse, const double* x, const Logits64& lg, int64_t n,
                            const LimitsT<double>* lim = nullptr, double* y = nullptr, double* lad = nullptr,
                            int32_t* bad = nullptr) {
  Rqs64Args a{};
  a.x = x; a.uw = lg.uw; a.uh = lg.uh; a.ud = lg.ud; a.ld_w = lg.ld_w; a.ld_h = lg.ld_h; a.ld_d = lg.ld_d;
  a.inner = lg.inner; a.ks = lg.ks; a.period = lg.period;
  a.y = y; a.lad = lad; a.bad = bad; a.n = n;
  a.c = rqs_fill_const64(*cfg);
  a.inverse = inverse ? 1 : 0;
  if (lim) a.lim = *lim;
  return a;
}

// The arguments of the VJP kernel: the forward operands, the upstream gradients g_y and g_logabsdet (read at
// i / lad_div), the gradient rows (in the layout of the logits where those are strided) and, for the LIM kernels, the
// limits' gradients.
static Rqs64BwdArgs bwd_args64(const vcnf_rqs_cfg_f64* cfg, int inverse, const double* x, const Logits64& lg, int64_t n,
                               const LimitsT<double>* lim, const double* g_y, const double* g_logabsdet, int64_t lad_div,
                               double* g_x, double* g_uw, double* g_uh, double* g_ud,
                               std::array<double*, 4> g_lim = {}) {
  Rqs64BwdArgs g{};
  g.f = fwd_args64(cfg, inverse, x, lg, n, lim);
  g.gy = g_y; g.glad = g_logabsdet; g.lad_div = lad_div;
  g.gx = g_x; g.guw = g_uw; g.guh = g_uh; g.gud = g_ud;
  g.nd = rqs_n_deriv(cfg->tails, cfg->num_bins);
  for (int j = 0; j < 4; ++j) g.glim[j] = g_lim[j];
  return g;
}

// Not rqs_check_cfg: this check tests n together with the bin count, ahead of the tails, and lets linear tails pass
// with one bin; callers see both in the status they get.
static int check_fwd64(const vcnf_rqs_cfg_f64* cfg, int64_t n) {
  if (!cfg) return VCNF_ERR_NULL;
  if (n < 0 || cfg->num_bins < 1 || cfg->num_bins > kMaxBins64) return VCNF_ERR_SHAPE;
  if (cfg->tails < VCNF_TAILS_NONE || cfg->tails > VCNF_TAILS_CIRCULAR) return VCNF_ERR_UNSUPPORTED;
  const int K = cfg->num_bins;
  if (cfg->min_bin_width * K > 1.0 || cfg->min_bin_height * K > 1.0) return VCNF_ERR_VALUE;
  return VCNF_OK;
}

// validation as bwd_common / vcnf_rqs_elementwise_bwd_f32 (rqs_backward.hip)
static int check_bwd64(const vcnf_rqs_cfg_f64* cfg, int64_t n) {
  const int rc = rqs_check_cfg(cfg, kMaxBins64);
  if (rc != VCNF_OK) return rc;
  return n < 0 ? VCNF_ERR_SHAPE : VCNF_OK;
}

extern "C" int vcnf_rqs_elementwise_f64(const double* x, const double* uw, const double* uh, const double* ud,
                                        int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                        double* y, double* logabsdet, int64_t n,
                                        const vcnf_rqs_cfg_f64* cfg, int inverse, int32_t* bad_disc, void* stream) {
  const int rc = check_fwd64(cfg, n);
  if (rc != VCNF_OK) return rc;
  if (n == 0) return VCNF_OK;
  if (!x || !uw || !uh || !ud || !y || !logabsdet) return VCNF_ERR_NULL;
  const Logits64 lg{uw, uh, ud, ld_w, ld_h, ld_d};
  return launch_fwd64<false>(fwd_args64(cfg, inverse, x, lg, n, nullptr, y, logabsdet, bad_disc), stream);
}

extern "C" int vcnf_rqs_elementwise_strided_f64(const double* x, const double* uw, const double* uh, const double* ud,
                                                int64_t row_w, int64_t row_h, int64_t row_d, int64_t inner,
                                                int64_t k_stride, int64_t period,
                                                double* y, double* logabsdet, int64_t n,
                                                const vcnf_rqs_cfg_f64* cfg, int inverse, int32_t* bad_disc,
                                                void* stream) {
  const int rc = check_fwd64(cfg, n);
  if (rc != VCNF_OK) return rc;
  if (row_w < 0 || row_h < 0 || row_d < 0 || inner < 1 || k_stride < 1 || period < 0) return VCNF_ERR_SHAPE;
  if (n == 0) return VCNF_OK;
  if (!x || !uw || !uh || !ud || !y || !logabsdet) return VCNF_ERR_NULL;
  const Logits64 lg{uw, uh, ud, row_w, row_h, row_d, inner, k_stride, period};
  return launch_fwd64<true>(fwd_args64(cfg, inverse, x, lg, n, nullptr, y, logabsdet, bad_disc), stream);
}

extern "C" int vcnf_rqs_elementwise_bwd_f64(const double* x, const double* uw, const double* uh, const double* ud,
                                            int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                            const double* g_y, const double* g_logabsdet,
                                            double* g_x, double* g_uw, double* g_uh, double* g_ud, int64_t n,
                                            const vcnf_rqs_cfg_f64* cfg, int inverse, void* stream) {
  const int rc = check_bwd64(cfg, n);
  if (rc != VCNF_OK) return rc;
  if (ld_w < 0 || ld_h < 0 || ld_d < 0) return VCNF_ERR_SHAPE;
  if (n == 0) return VCNF_OK;
  if (!x || !uw || !uh || !ud || !g_y || !g_logabsdet || !g_x || !g_uw || !g_uh || !g_ud) return VCNF_ERR_NULL;
  const Logits64 lg{uw, uh, ud, ld_w, ld_h, ld_d};
  return launch_bwd64<false>(
      bwd_args64(cfg, inverse, x, lg, n, nullptr, g_y, g_logabsdet, 1, g_x, g_uw, g_uh, g_ud), stream);
}

extern "C" int vcnf_rqs_elementwise_limits_f64(const double* x, const double* uw, const double* uh, const double* ud,
                                               int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                               const double* left, const double* right, const double* bottom,
                                               const double* top, const vcnf_rqs_limit_bcast* bcast,
                                               double* y, double* logabsdet, int64_t n,
                                               const vcnf_rqs_cfg_f64* cfg, int inverse, int32_t* bad_disc,
                                               void* stream) {
  const int rc = limits_validate(cfg, n, ld_w, ld_h, ld_d, bcast);
  if (rc != VCNF_OK) return rc;
  if (n == 0) return VCNF_OK;
  if (!x || !uw || !uh || !ud || !left || !right || !bottom || !top || !y || !logabsdet) return VCNF_ERR_NULL;
  const Logits64 lg{uw, uh, ud, ld_w, ld_h, ld_d};
  const LimitsT<double> lim = make_limits(left, right, bottom, top, bcast, n);
  return launch_fwd64<false, true>(fwd_args64(cfg, inverse, x, lg, n, &lim, y, logabsdet, bad_disc), stream);
}

extern "C" int vcnf_rqs_elementwise_limits_bwd_f64(const double* x, const double* uw, const double* uh,
                                                   const double* ud, int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                                   const double* left, const double* right, const double* bottom,
                                                   const double* top, const vcnf_rqs_limit_bcast* bcast,
                                                   const double* g_y, const double* g_logabsdet,
                                                   double* g_x, double* g_uw, double* g_uh, double* g_ud,
                                                   double* g_left, double* g_right, double* g_bottom, double* g_top,
                                                   int64_t n, const vcnf_rqs_cfg_f64* cfg, int inverse, void* stream) {
  const int rc = limits_validate(cfg, n, ld_w, ld_h, ld_d, bcast);
  if (rc != VCNF_OK) return rc;
  if (n == 0) return VCNF_OK;
  if (!x || !uw || !uh || !ud || !left || !right || !bottom || !top || !g_y || !g_logabsdet || !g_x || !g_uw ||
      !g_uh || !g_ud)
    return VCNF_ERR_NULL;
  const Logits64 lg{uw, uh, ud, ld_w, ld_h, ld_d};
  const LimitsT<double> lim = make_limits(left, right, bottom, top, bcast, n);
  return launch_bwd64<false, true>(bwd_args64(cfg, inverse, x, lg, n, &lim, g_y, g_logabsdet, 1, g_x, g_uw, g_uh, g_ud,
                                              {g_left, g_right, g_bottom, g_top}),
                                   stream);
}

extern "C" int vcnf_rqs_packed_bwd_f64(const double* x, const double* params, int64_t inner, int64_t lad_div,
                                       const double* g_y, const double* g_logabsdet,
                                       double* g_x, double* g_params, int64_t n,
                                       const vcnf_rqs_cfg_f64* cfg, int inverse, void* stream) {
  const int rc = check_bwd64(cfg, n);
  if (rc != VCNF_OK) return rc;
  if (inner < 1 || lad_div < 1) return VCNF_ERR_SHAPE;
  if (n == 0) return VCNF_OK;
  if (!x || !params || !g_y || !g_logabsdet || !g_x || !g_params) return VCNF_ERR_NULL;
  // params / g_params [rows, P, inner]: logit k of element i = row * P * inner + s + k * inner
  const int64_t K = cfg->num_bins, row = (2 * K + rqs_n_deriv(cfg->tails, cfg->num_bins)) * inner;
  const Logits64 lg{params, params + K * inner, params + 2 * K * inner, row, row, row, inner, inner};
  return launch_bwd64<true>(bwd_args64(cfg, inverse, x, lg, n, nullptr, g_y, g_logabsdet, lad_div, g_x, g_params,
                                       g_params + K * inner, g_params + 2 * K * inner),
                            stream);
}
