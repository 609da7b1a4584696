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
  int K, tails, inverse;
  double left, right, bottom, top, min_w, min_h, min_d, wh_scale, edge;
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

// Knot construction, bin search and derivative-logit padding (rqs_math64.hpp) are shared by the forward kernel and the
// VJP kernel below, so that both select the same bin for every element.  KT > 0: compile-time bin count (the templated
// instances of both kernels keep every array in registers); KT == 0: runtime K (their generic instances).

// KT > 0: compile-time bin count, every array in registers (K = 8, 10, 16); KT == 0: any K up to 64 (runtime-indexed
// arrays in scratch).  Both instances evaluate the same expressions in the same order.  LIM (dense rows, no tails): the
// interval of element i comes from a.lim (tensor limits, splines.py:99-102).
template <int KT, bool STRIDED, bool LIM = false>
__global__ __launch_bounds__(256) void rqs_elementwise_f64_kernel(const Rqs64Args a) {
  constexpr int KA = KT > 0 ? KT : kMaxBins64;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long long)gridDim.x * blockDim.x) {
    const double x = a.x[i];
    if (a.tails != VCNF_TAILS_NONE && !(x >= a.left && x <= a.right)) {   // splines.py:30-49: identity outside
      a.y[i] = x;
      a.lad[i] = 0.0;
      continue;
    }
    double lv[4] = {a.left, a.right, a.bottom, a.top};
    if (LIM) a.lim.load(i, lv);
    const double left = lv[0], right = lv[1], bottom = lv[2], top = lv[3];
    const int K = KT > 0 ? KT : a.K;
    const Rows64 rw = rows64<STRIDED>(a, i);
    double xk[KA + 1], yk[KA + 1];
    partition64<KT>(a.uw + rw.w, rw.ks, K, a.wh_scale, left, right, a.min_w, xk);
    partition64<KT>(a.uh + rw.h, rw.ks, K, a.wh_scale, bottom, top, a.min_h, yk);
    const int bin = a.inverse ? bin64<KT>(yk, K, x) : bin64<KT>(xk, K, x);
    const double* ud = a.ud + rw.d;
    auto dlogit = [&](int k) -> double {
      const int j = dlogit_col64(k, K, a.tails);
      return j < 0 ? a.edge : ud[j * rw.ks];
    };
    const double d0 = a.min_d + softplus64(dlogit(bin));           // :121
    const double d1 = a.min_d + softplus64(dlogit(bin + 1));
    double x_lo, x_hi, y_lo, y_hi;
    pick_bin64<KT>(xk, yk, bin, K, x_lo, x_hi, y_lo, y_hi);
    const double w = x_hi - x_lo;
    const double h = y_hi - y_lo;
    const double s = h / w;                                          // :144
    double out, lad;
    if (a.inverse) {
      const double dy = x - y_lo;
      const double e = d0 + d1 - 2.0 * s;
      const double qa = dy * e + h * (s - d0);                       // :153-161
      const double qb = h * d0 - dy * e;
      const double qc = -s * dy;
      const double disc = qb * qb - 4.0 * qa * qc;                   // :163
      if (!(disc >= 0.0) && a.bad) atomicAdd(a.bad, 1);              // :164 (the reference asserts)
      const double r = (2.0 * qc) / (-qb - sqrt(disc));              // :166
      out = r * w + x_lo;
      const double rr = r * (1.0 - r);
      const double den = s + e * rr;
      const double dnum = s * s * (d1 * r * r + 2.0 * s * rr + d0 * (1.0 - r) * (1.0 - r));
      lad = -(log(dnum) - 2.0 * log(den));                           // :175-177
    } else {
      const double t = (x - x_lo) / w;                               // :179
      const double tt = t * (1.0 - t);
      const double num = h * (s * t * t + d0 * tt);
      const double den = s + (d0 + d1 - 2.0 * s) * tt;
      out = y_lo + num / den;                                        // :186
      const double dnum = s * s * (d1 * t * t + 2.0 * s * tt + d0 * (1.0 - t) * (1.0 - t));
      lad = log(dnum) - 2.0 * log(den);                              // :191
    }
    a.y[i] = out;
    a.lad[i] = lad;
  }
}

template <bool STRIDED, bool LIM = false>
static void launch_fwd64(const Rqs64Args& a, dim3 grid, hipStream_t st) {
  with_bins(kBins64, a.K, [&](auto kt) {
    hipLaunchKernelGGL((rqs_elementwise_f64_kernel<decltype(kt)::value, STRIDED, LIM>), grid, dim3(256), 0, st, a);
  });
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

struct RqsBin64 {
  double xl, w, yl, h, d0, d1;
};

// KT > 0: the K probabilities and K+1 knots of each side live in registers (loops of constant trip count, fully
// unrolled by the compiler: compile-time indices;
// the bin's values are picked by comparison, never by a runtime index).  KT == 0 (any other K up to 64): the same
// code with runtime-indexed arrays, which go to scratch.
// LIM (dense rows, no tails): per-element limits as in the forward kernel, plus their per-element gradients.
template <int KT, bool INV, bool STRIDED, bool LIM = false>
__global__ __launch_bounds__(256) void rqs_elementwise_bwd_f64_kernel(const Rqs64BwdArgs g) {
  const Rqs64Args& a = g.f;
  constexpr int KA = KT > 0 ? KT : kMaxBins64;
  const int K = KT > 0 ? KT : a.K;
  const int nd = g.nd;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long long)gridDim.x * blockDim.x) {
    const double x = a.x[i];
    const double gy = g.gy[i], gl = g.glad[STRIDED && g.lad_div != 1 ? i / g.lad_div : i];
    const Rows64 rw = rows64<STRIDED>(a, i);
    const long long ks = rw.ks;
    double* guw = g.guw + (STRIDED ? rw.w : i * K);
    double* guh = g.guh + (STRIDED ? rw.h : i * K);
    double* gud = g.gud + (STRIDED ? rw.d : i * nd);
    if (a.tails != VCNF_TAILS_NONE && !(x >= a.left && x <= a.right)) {   // identity outside: dy/dx = 1
      g.gx[i] = gy;
      for (int k = 0; k < K; ++k) { guw[k * ks] = 0.0; guh[k * ks] = 0.0; }
      for (int k = 0; k < nd; ++k) gud[k * ks] = 0.0;
      continue;
    }
    double lv[4] = {a.left, a.right, a.bottom, a.top};
    if (LIM) a.lim.load(i, lv);
    const double left = lv[0], right = lv[1], bottom = lv[2], top = lv[3];
    double xk[KA + 1], yk[KA + 1], pw[KA], ph[KA];
    constexpr int KF = LIM ? KA + 1 : 1;
    double fx[KF], fy[KF];                           // LIM: cumulative fractions of the knots
    partition64<KT>(a.uw + rw.w, ks, K, a.wh_scale, left, right, a.min_w, xk, pw, LIM ? fx : nullptr);
    partition64<KT>(a.uh + rw.h, ks, K, a.wh_scale, bottom, top, a.min_h, yk, ph, LIM ? fy : nullptr);
    const int bin = bin64<KT>(INV ? yk : xk, K, x);
    RqsBin64 b;
    double xr, yr;
    pick_bin64<KT>(xk, yk, bin, K, b.xl, xr, b.yl, yr);
    b.w = xr - b.xl;
    b.h = yr - b.yl;
    const double* ud = a.ud + rw.d;
    const int j0 = dlogit_col64(bin, K, a.tails), j1 = dlogit_col64(bin + 1, K, a.tails);
    const double l0 = j0 < 0 ? a.edge : ud[j0 * ks], l1 = j1 < 0 ? a.edge : ud[j1 * ks];
    b.d0 = a.min_d + softplus64(l0);
    b.d1 = a.min_d + softplus64(l1);
    BinGradT<double> bg;
    if (!INV) {
      bg = bin_forward_vjp<double>(x, b, gy, gl);
    } else {
      // the forward kernel's root (splines.py:153-166), in bin coordinates
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
    const double cx = (right - left) * (1.0 - a.min_w * K), cy = (top - bottom) * (1.0 - a.min_h * K);
    double dotw = 0.0, doth = 0.0;
    for (int k = 0; k < K; ++k) {
      dotw += pw[k] * (cx * ((k < bin ? gXl : 0.0) + (k < bin + 1 ? gXr : 0.0)));
      doth += ph[k] * (cy * ((k < bin ? gYl : 0.0) + (k < bin + 1 ? gYr : 0.0)));
    }
    for (int k = 0; k < K; ++k) {
      const double gWk = cx * ((k < bin ? gXl : 0.0) + (k < bin + 1 ? gXr : 0.0));
      const double gHk = cy * ((k < bin ? gYl : 0.0) + (k < bin + 1 ? gYr : 0.0));
      guw[k * ks] = a.wh_scale * pw[k] * (gWk - dotw);
      guh[k * ks] = a.wh_scale * ph[k] * (gHk - doth);
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
static void launch_bwd64(const Rqs64BwdArgs& g, dim3 grid, hipStream_t st) {
  with_bins(kBins64, g.f.K, [&](auto kt) {
    with_flags([&](auto INVERSE) {
      hipLaunchKernelGGL((rqs_elementwise_bwd_f64_kernel<kt(), INVERSE(), STRIDED, LIM>), grid, dim3(256), 0, st, g);
    }, g.f.inverse != 0);
  });
}

}  // namespace vcnf

using namespace vcnf;

// constants of the spline, the same for every entry point (kept in double, so not rqs_fill_const); dense rows
// unless the caller sets inner / ks / period, no outputs of the forward map unless it sets y / lad / bad
static void fill64(Rqs64Args& a, const vcnf_rqs_cfg_f64* cfg, int inverse) {
  a.K = cfg->num_bins; a.tails = cfg->tails; a.inverse = inverse ? 1 : 0;
  a.left = cfg->left; a.right = cfg->right; a.bottom = cfg->bottom; a.top = cfg->top;
  a.min_w = cfg->min_bin_width; a.min_h = cfg->min_bin_height; a.min_d = cfg->min_derivative;
  a.wh_scale = cfg->wh_scale;
  a.edge = log(exp(1.0 - cfg->min_derivative) - 1.0);
  a.inner = 1; a.ks = 1; a.period = 0;
  a.y = nullptr; a.lad = nullptr; a.bad = nullptr;
}

// the input and its logit rows
static void operands64(Rqs64Args& a, const double* x, const double* uw, const double* uh, const double* ud,
                       int64_t ld_w, int64_t ld_h, int64_t ld_d, int64_t n) {
  a.x = x; a.uw = uw; a.uh = uh; a.ud = ud; a.ld_w = ld_w; a.ld_h = ld_h; a.ld_d = ld_d; a.n = n;
}

// the gradient operands of a VJP
static void grads64(Rqs64BwdArgs& g, const vcnf_rqs_cfg_f64* cfg, const double* g_y, const double* g_logabsdet,
                    double* g_x, double* g_uw, double* g_uh, double* g_ud, int64_t lad_div) {
  g.gy = g_y; g.glad = g_logabsdet; g.gx = g_x; g.guw = g_uw; g.guh = g_uh; g.gud = g_ud;
  g.nd = rqs_n_deriv(cfg->tails, cfg->num_bins); g.lad_div = lad_div;
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

static dim3 grid64(int64_t n) { return dim3(elem_blocks(n, 256, 256 * 32)); }

extern "C" int vcnf_rqs_elementwise_f64(const double* x, const double* uw, const double* uh, const double* ud,
                                        int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                        double* y, double* logabsdet, int64_t n,
                                        const vcnf_rqs_cfg_f64* cfg, int inverse, int32_t* bad_disc, void* stream) {
  const int rc = check_fwd64(cfg, n);
  if (rc != VCNF_OK) return rc;
  if (n == 0) return VCNF_OK;
  if (!x || !uw || !uh || !ud || !y || !logabsdet) return VCNF_ERR_NULL;
  Rqs64Args a;
  fill64(a, cfg, inverse);
  operands64(a, x, uw, uh, ud, ld_w, ld_h, ld_d, n);
  a.y = y; a.lad = logabsdet; a.bad = bad_disc;
  launch_fwd64<false>(a, grid64(n), (hipStream_t)stream);
  return launched();
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
  Rqs64Args a;
  fill64(a, cfg, inverse);
  operands64(a, x, uw, uh, ud, row_w, row_h, row_d, n);
  a.inner = inner; a.ks = k_stride; a.period = period;
  a.y = y; a.lad = logabsdet; a.bad = bad_disc;
  launch_fwd64<true>(a, grid64(n), (hipStream_t)stream);
  return launched();
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
  Rqs64BwdArgs g;
  Rqs64Args& a = g.f;
  fill64(a, cfg, inverse);
  operands64(a, x, uw, uh, ud, ld_w, ld_h, ld_d, n);
  grads64(g, cfg, g_y, g_logabsdet, g_x, g_uw, g_uh, g_ud, 1);
  launch_bwd64<false>(g, grid64(n), (hipStream_t)stream);
  return launched();
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
  Rqs64Args a;
  fill64(a, cfg, inverse);
  operands64(a, x, uw, uh, ud, ld_w, ld_h, ld_d, n);
  a.y = y; a.lad = logabsdet; a.bad = bad_disc;
  a.lim = make_limits(left, right, bottom, top, bcast, n);
  launch_fwd64<false, true>(a, grid64(n), (hipStream_t)stream);
  return launched();
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
  Rqs64BwdArgs g;
  Rqs64Args& a = g.f;
  fill64(a, cfg, inverse);
  operands64(a, x, uw, uh, ud, ld_w, ld_h, ld_d, n);
  a.lim = make_limits(left, right, bottom, top, bcast, n);
  grads64(g, cfg, g_y, g_logabsdet, g_x, g_uw, g_uh, g_ud, 1);
  g.glim[0] = g_left; g.glim[1] = g_right; g.glim[2] = g_bottom; g.glim[3] = g_top;
  launch_bwd64<false, true>(g, grid64(n), (hipStream_t)stream);
  return launched();
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
  Rqs64BwdArgs g;
  Rqs64Args& a = g.f;
  const long long K = cfg->num_bins, P = 2 * K + rqs_n_deriv(cfg->tails, cfg->num_bins);
  // params / g_params [rows, P, inner]: logit k of element i = row * P * inner + s + k * inner
  const long long row = P * inner;
  fill64(a, cfg, inverse);
  operands64(a, x, params, params + K * inner, params + 2 * K * inner, row, row, row, n);
  a.inner = inner; a.ks = inner;
  grads64(g, cfg, g_y, g_logabsdet, g_x, g_params, g_params + K * inner, g_params + 2 * K * inner, lad_div);
  launch_bwd64<true>(g, grid64(n), (hipStream_t)stream);
  return launched();
}
