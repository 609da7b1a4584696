// The sampling direction of the autoregressive flows - MaskedAffineAutoregressive.inverse (the MAF) and
// MaskedPiecewiseRationalQuadraticAutoregressive.inverse (the autoregressive neural spline layers) - in one launch
// (normflow/flows/affine/autoregressive.py:29-36 over nets/made.py:215-300).  The reference runs D = features full MADE
// passes, each fixing one more variable.  In a MADE with the reference's sequential hidden degrees a hidden unit of
// degree m, in any layer, depends only on inputs of degree <= m and on hidden units of degree <= m: once the variable of
// degree m is known every unit of degree m in every layer is final.  So the D passes cost one masked MADE pass, ordered
// by degree, with one inversion between stages.
//
// Operands (vcnf_amd/made_sample.py packs them; T = float or double):
//   tables int32 [2 D]: order[i], the column of x that holds the variable of degree i + 1, and count[i], the number of
//     hidden units of degree <= i.  Hidden units are stored in ascending degree (the same order in every layer), so the
//     units of degree <= i are the first count[i] of every layer.
//   wpack, the masked weights W * mask in that order, one after the other:
//     Wi [H, D] (columns in the order of `order`), bi [H];  per residual block  W0 [H, H], b0 [H], W1 [H, H], b1 [H];
//     Wf [D P, H] (the P rows of the variable of degree i + 1 at rows i P ..), bf [D P].
//   ctx_add [B, H] (or NULL): context_layer(context) of the MADE;  ctx_gate [nb, B, H] (or NULL): the blocks'
//     context_layer(context) before the sigmoid; both with their units in the stored order.
// Per sample, for i = 0 .. D - 1 (the stage rule):
//   1. for the units u in [count[i - 1], count[i]) (count[-1] = 0), layer by layer:
//        h_0[u]     = bi[u] + sum_{j < i} Wi[u, j] y[j] + ctx_add[u]
//        t_k[u]     = b0_k[u] + sum_{v < count[i]} W0_k[u, v] relu(h_k[v])
//        h_{k+1}[u] = h_k[u] + (b1_k[u] + sum_{v < count[i]} W1_k[u, v] relu(t_k[v])) gate_k[u],
//        gate_k[u]  = sigmoid(ctx_gate[k, b, u]), 1 without context
//   2. q[p] = bf[i P + p] + sum_{v < count[i]} Wf[i P + p, v] h_nb[v]  for p < P
//   3. affine (P = 2, cfg NULL): scale = sigmoid(q[0] + 2) + 1e-3, y[i] = (x[order[i]] - q[1]) / scale, ld -= log scale
//      spline: (y[i], lad) = the inverse spline of cfg (rqs_math64.hpp, in both precisions) at x[order[i]] with the logits q
//      laid out [K widths | K heights | derivatives]; ld += lad
//   4. out[order[i]] = y[i]
// and logdet[b] = ld_sign ld, stored or accumulated.  Stage 0 of features = 1 has count[0] = H (every degree is 0) and
// no input term; a degree that owns no unit has an empty range in step 1.
//
// Mapping: a sample needs (1 + 2 nb) H + D values and P doubles that live from its first variable to its last,
// too many for registers, so they sit in LDS and a group of G lanes (8 .. 64, a power of two) shares a sample.  A dot
// product is split over the lanes of the group (lane g takes the terms k = g, g + G, ...), four rows at a time so that
// one LDS read feeds four multiply-adds, and summed with the ascending butterfly: a fixed order, the same bits in every
// call and at every batch size.  Lanes of a group read consecutive LDS words and the samples of a wave start G banks
// apart.  Weight rows are read over their prefix only: the masked-out part is never multiplied.  G is the smallest group
// with which a workgroup's LDS stays under 48 KiB, so at least three workgroups (12 waves) fit a CU.  The grid is capped
// and a workgroup loops over tiles of 256 / G samples.  No scratch, no atomics besides the bad_disc flag.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vcnf_hip.h"
#include "rqs_host.hpp"
#include "rqs_math64.hpp"
#include "stream_common.hpp"

// every multiply-add below is written out (fma): the same bits whatever the compiler would contract
#pragma clang fp contract(off)

namespace vcnf_made {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr int kRows = 4;                     // rows of a weight matrix per pass over the activations
constexpr int kDeep = 4;                     // terms per lane whose loads are issued together
constexpr int kMinLanes = 8, kMaxLanes = 64;
constexpr long long kMaxGrid = 1024;         // workgroups; beyond it a workgroup takes several tiles
constexpr size_t kLdsTarget = 48 * 1024;     // three workgroups per CU
constexpr int kMaxFeatures = 1024, kMaxHidden = 4096, kMaxNetBlocks = 16, kMaxBins = 64;

// Storage is T (x, y, weights, the activations in LDS); arithmetic is double in both instances.  The fp32 instance
// accumulates its dot products in double, keeps a stage's logits in double and inverts with the fp64 spline: the
// inverse spline is ill-conditioned beside a floor-level derivative (rqs_math.hpp on the discriminant), and in fp32 its
// own rounding, not the conditioner's, sets the error of y and of the log-det.  Each activation, y and the log-det are
// rounded to T once.
using A = double;

// the spline configuration of an entry point
template <typename T>
struct SplineOf;
template <>
struct SplineOf<float> {
  using Cfg = vcnf_rqs_cfg;
};
template <>
struct SplineOf<double> {
  using Cfg = vcnf_rqs_cfg_f64;
};

template <typename T>
struct Args {
  const T* x;
  T *y, *logdet;
  const T *ctx_add, *ctx_gate, *w;
  const int32_t* tab;
  long long B;
  int D, H, nb, P, G, stride, nwg, ld_mode;
  T ld_sign;
  int32_t* bad;
  vcnf::Rqs64Const c;
};

// step 3 for the spline, on the logits q of one variable: [K widths | K heights | derivative logits]
template <int KT>
__device__ __forceinline__ void invert_spline(double x, const double* q, const vcnf::Rqs64Const& c, double& y,
                                              double& lad, bool& bad) {
  if (c.tails != VCNF_TAILS_NONE && !(x >= c.left && x <= c.right)) {   // splines.py:30-49: identity outside
    y = x;
    lad = 0.0;
    return;
  }
  vcnf::rqs_inverse64<KT>(x, q, q + KT, q + 2 * KT, 1, c, y, lad, bad);
}

// epi(r, w[r, :n] . f(v[:n])) for the rows r0 <= r < r1 of w (row stride ldw), f = relu or the identity: lane g of the
// group takes the terms g, g + G, ..., the butterfly leaves the sum in every lane, lane r % kRows hands it to epi.
template <typename T, bool RELU, class Epi>
__device__ __forceinline__ void dot_rows(const T* __restrict__ w, int ldw, int r0, int r1, const T* v, int n, int g, int G,
                                         Epi&& epi) {
  for (int r = r0; r < r1; r += kRows) {
    const T* row[kRows];
    A acc[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      const int rr = r + u < r1 ? r + u : r1 - 1;     // a row past the end repeats the last one and is dropped below
      row[u] = w + (long long)rr * ldw;
      acc[u] = A(0);
    }
    // kDeep terms per lane and pass: their kRows * kDeep weight loads are in flight together (a tile is a chain of
    // dependent stages, so a pass that waits for one load at a time runs at the latency of the L2); the terms enter the
    // sums in ascending order either way
    int k = g;
    for (; k + (kDeep - 1) * G < n; k += kDeep * G) {
      T xv[kDeep], wv[kRows][kDeep];
#pragma unroll
      for (int j = 0; j < kDeep; ++j) {
#pragma unroll
        for (int u = 0; u < kRows; ++u) wv[u][j] = row[u][k + j * G];
        xv[j] = v[k + j * G];
        if (RELU) xv[j] = xv[j] < T(0) ? T(0) : xv[j];
      }
#pragma unroll
      for (int j = 0; j < kDeep; ++j) {
#pragma unroll
        for (int u = 0; u < kRows; ++u) acc[u] = fma((A)wv[u][j], (A)xv[j], acc[u]);
      }
    }
    for (; k < n; k += G) {
      T xv = v[k];
      if (RELU) xv = xv < T(0) ? T(0) : xv;
#pragma unroll
      for (int u = 0; u < kRows; ++u) acc[u] = fma((A)row[u][k], (A)xv, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < kRows; ++u) acc[u] = lanes_sum(acc[u], 1, G);
#pragma unroll
    for (int u = 0; u < kRows; ++u)
      if (g == u && r + u < r1) epi(r + u, acc[u]);
  }
}

// KIND < 0: the affine map of the MAF; KIND > 0: the spline with KIND bins (compile time only: rqs_math64.hpp).
template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void made_sample_kernel(const Args<T> a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int D = a.D, H = a.H, nb = a.nb, P = a.P, G = a.G;
  const int g = threadIdx.x & (G - 1);
  const int per_block = kBlock / G;
  // per sample: the P logits of a stage (double; the stride keeps them 8-byte aligned), y in degree order, the activations
  A* const q = reinterpret_cast<A*>(reinterpret_cast<T*>(lds_raw) + (size_t)(threadIdx.x / G) * a.stride);
  T* const ys = reinterpret_cast<T*>(q + P);
  T* const act = ys + D;                                 // h_k at act + 2 k H, t_k at act + (2 k + 1) H
  const T* const wi = a.w;
  const T* const bi = wi + (long long)H * D;
  const T* const wblk = bi + H;
  const long long blk = 2LL * H * H + 2LL * H;
  const T* const wf = wblk + nb * blk;
  const T* const bf = wf + (long long)D * P * H;
  const long long ntiles = (a.B + per_block - 1) / per_block;
  bool bad = false;
  for (long long tile = blockIdx.x; tile < ntiles; tile += a.nwg) {
    const long long b = tile * per_block + threadIdx.x / G;
    const bool live = b < a.B;
    const long long bb = live ? b : a.B - 1;           // lanes past the batch follow the last sample and store nothing
    A ld = A(0);
    bool bad_here = false;
    int prev = 0;
    for (int i = 0; i < D; ++i) {
      int cnt = a.tab[D + i], var = a.tab[i];
      cnt = cnt < prev ? prev : (cnt > H ? H : cnt);   // a table that is not one cannot send an index out of bounds
      var = var < 0 ? 0 : (var >= D ? D - 1 : var);
      if (cnt > prev) {
        dot_rows<T, false>(wi, D, prev, cnt, ys, i, g, G, [&](int u, A s) {
          s += (A)bi[u];
          if (a.ctx_add) s += (A)a.ctx_add[bb * H + u];
          act[u] = (T)s;
        });
        __syncthreads();
        for (int k = 0; k < nb; ++k) {
          const T* const w0 = wblk + k * blk;
          const T* const b0 = w0 + (long long)H * H;
          const T* const w1 = b0 + H;
          const T* const b1 = w1 + (long long)H * H;
          T* const h = act + 2 * k * H;
          dot_rows<T, true>(w0, H, prev, cnt, h, cnt, g, G, [&](int u, A s) { h[H + u] = (T)(s + (A)b0[u]); });
          __syncthreads();
          dot_rows<T, true>(w1, H, prev, cnt, h + H, cnt, g, G, [&](int u, A s) {
            s += (A)b1[u];
            if (a.ctx_gate) s *= sigmoid_((A)a.ctx_gate[((long long)k * a.B + bb) * H + u]);
            h[2 * H + u] = (T)((A)h[u] + s);
          });
          __syncthreads();
        }
      }
      dot_rows<T, false>(wf + (long long)i * P * H, H, 0, P, act + 2 * nb * H, cnt, g, G,
                         [&](int p, A s) { q[p] = s + (A)bf[i * P + p]; });
      __syncthreads();
      const A xv = (A)a.x[bb * D + var];
      A yv, lad;
      if constexpr (KIND < 0) {
        const A scale = sigmoid_(q[0] + A(2)) + A(1e-3);
        yv = (xv - q[1]) / scale;
        lad = -log_(scale);
      } else {
        invert_spline<KIND>(xv, q, a.c, yv, lad, bad_here);
      }
      ld += lad;
      if (g == 0) {
        ys[i] = (T)yv;
        if (live) a.y[b * D + var] = (T)yv;
      }
      prev = cnt;
      __syncthreads();
    }
    if (g == 0 && live) put_ld(a.logdet, b, (T)((A)a.ld_sign * ld), a.ld_mode);
    bad = bad || (bad_here && live);
  }
  if (bad && g == 0 && a.bad) atomicAdd(a.bad, 1);
}

// lanes per sample, the sample's LDS stride in elements and the workgroup's LDS in bytes; false where no group fits
static bool plan(int64_t D, int64_t H, int64_t nb, int64_t P, size_t elem, int& G, int& stride, size_t& lds) {
  if (D < 1 || D > kMaxFeatures || H < 1 || H > kMaxHidden || nb < 0 || nb > kMaxNetBlocks || P < 2 ||
      P > 3 * kMaxBins + 1 || (elem != 4 && elem != 8))
    return false;
  const int64_t need = P * (int64_t)(sizeof(A) / elem) + D + (1 + 2 * nb) * H;     // in elements; the logits are doubles
  for (G = kMinLanes;; G <<= 1) {
    // the samples of a 32-lane half start G banks apart (fp64: 2 G of 64); an even stride keeps the logits aligned
    stride = (int)(G < 32 ? need + ((G - need % 32) + 32) % 32 : need + need % 2);
    lds = (size_t)(kBlock / G) * stride * elem;
    if (lds <= kLdsTarget) return true;
    if (G == kMaxLanes) return lds <= vcnf::kDynamicLdsDefault;
  }
}

// bins of a parameter row: P = 3 K - 1 (linear tails), 3 K (circular) or 3 K + 1 (none)
static int bins_of(int P) { return (P + 1) / 3; }

template <typename T, int KIND>
static int launch(const Args<T>& a, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL((made_sample_kernel<T, KIND>), dim3((unsigned)a.nwg), dim3(kBlock), lds, st, a);
  return launched();
}

// the constants of either configuration, in double (a float configuration's values as they are)
template <class Cfg>
static void fill(const Cfg& cfg, vcnf::Rqs64Const& c) {
  c = vcnf::rqs_fill_const64(vcnf_rqs_cfg_f64{cfg.num_bins, cfg.tails, cfg.left, cfg.right, cfg.bottom, cfg.top,
                                              cfg.min_bin_width, cfg.min_bin_height, cfg.min_derivative, cfg.wh_scale});
}

template <typename T>
static int dispatch(const Args<T>& a, size_t lds, hipStream_t st) {
  return launch_listed(vcnf::kBins64, a.c.K, [&](auto kt) { return launch<T, kt()>(a, lds, st); });
}

template <typename T>
static int made_sample(const T* x, T* y, T* logdet, const T* ctx_add, const T* ctx_gate, const T* wpack,
                       int64_t wpack_elems, const int32_t* tables, int64_t batch, int32_t features, int32_t hidden,
                       int32_t num_blocks, int32_t params, const typename SplineOf<T>::Cfg* cfg, int ld_mode, T ld_sign,
                       int32_t* bad_disc, void* stream) {
  Args<T> a{};
  size_t lds;
  if (batch < 0 || !plan(features, hidden, num_blocks, params, sizeof(T), a.G, a.stride, lds)) return VCNF_ERR_SHAPE;
  if (wpack_elems != vcnf_made_sample_pack_elems(features, hidden, num_blocks, params)) return VCNF_ERR_SHAPE;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (cfg) {
    const int rc = vcnf::rqs_check_cfg(cfg, kMaxBins);
    if (rc != VCNF_OK) return rc;
    if (params != 2 * cfg->num_bins + vcnf::rqs_n_deriv(cfg->tails, cfg->num_bins)) return VCNF_ERR_SHAPE;
    if (!in_list(vcnf::kBins64, cfg->num_bins)) return VCNF_ERR_UNSUPPORTED;
  } else if (params != 2) {
    return VCNF_ERR_SHAPE;
  }
  if (batch == 0) return VCNF_OK;
  if (!x || !y || !logdet || !wpack || !tables) return VCNF_ERR_NULL;
  if ((ctx_gate && !ctx_add) || (ctx_add && num_blocks > 0 && !ctx_gate)) return VCNF_ERR_NULL;
  if (!all_aligned({x, y, logdet, ctx_add, ctx_gate, wpack}, sizeof(T)) || !all_aligned({tables, bad_disc}, 4))
    return VCNF_ERR_ALIGN;
  a.x = x; a.y = y; a.logdet = logdet; a.ctx_add = ctx_add; a.ctx_gate = ctx_gate; a.w = wpack; a.tab = tables;
  a.B = batch; a.D = features; a.H = hidden; a.nb = num_blocks; a.P = params;
  a.ld_mode = ld_mode; a.ld_sign = ld_sign; a.bad = bad_disc;
  const long long per_block = kBlock / a.G, ntiles = (batch + per_block - 1) / per_block;
  a.nwg = (int)(ntiles < kMaxGrid ? ntiles : kMaxGrid);
  if (!cfg) return launch<T, -1>(a, lds, (hipStream_t)stream);
  fill(*cfg, a.c);
  return dispatch(a, lds, (hipStream_t)stream);
}

}  // namespace vcnf_made

extern "C" int64_t vcnf_made_sample_pack_elems(int32_t features, int32_t hidden, int32_t num_blocks,
                                               int32_t params_per_feature) {
  const int64_t D = features, H = hidden, nb = num_blocks, P = params_per_feature;
  if (D < 1 || H < 1 || nb < 0 || P < 1) return 0;
  return H * D + H + nb * (2 * H * H + 2 * H) + D * P * H + D * P;
}

extern "C" int vcnf_made_sample_supported(int32_t features, int32_t hidden, int32_t num_blocks,
                                          int32_t params_per_feature, int32_t elem_size) {
  int G, stride;
  size_t lds;
  if (!vcnf_made::plan(features, hidden, num_blocks, params_per_feature, (size_t)elem_size, G, stride, lds)) return 0;
  if (params_per_feature == 2) return 1;
  const int K = vcnf_made::bins_of(params_per_feature);
  if (K > vcnf_made::kMaxBins) return 0;
  return vcnf::in_list(vcnf::kBins64, K) ? 1 : 0;
}

extern "C" int32_t vcnf_made_sample_lanes(int32_t features, int32_t hidden, int32_t num_blocks,
                                          int32_t params_per_feature, int32_t elem_size) {
  int G, stride;
  size_t lds;
  return vcnf_made::plan(features, hidden, num_blocks, params_per_feature, (size_t)elem_size, G, stride, lds) ? G : 0;
}

extern "C" int vcnf_made_sample_f32(const float* x, float* y, float* logdet, const float* ctx_add, const float* ctx_gate,
                                    const float* wpack, int64_t wpack_elems, const int32_t* tables, int64_t batch,
                                    int32_t features, int32_t hidden, int32_t num_blocks, int32_t params_per_feature,
                                    const vcnf_rqs_cfg* cfg, int ld_mode, float ld_sign, int32_t* bad_disc,
                                    void* stream) {
  return vcnf_made::made_sample<float>(x, y, logdet, ctx_add, ctx_gate, wpack, wpack_elems, tables, batch, features,
                                       hidden, num_blocks, params_per_feature, cfg, ld_mode, ld_sign, bad_disc, stream);
}

extern "C" int vcnf_made_sample_f64(const double* x, double* y, double* logdet, const double* ctx_add,
                                    const double* ctx_gate, const double* wpack, int64_t wpack_elems,
                                    const int32_t* tables, int64_t batch, int32_t features, int32_t hidden,
                                    int32_t num_blocks, int32_t params_per_feature, const vcnf_rqs_cfg_f64* cfg,
                                    int ld_mode, double ld_sign, int32_t* bad_disc, void* stream) {
  return vcnf_made::made_sample<double>(x, y, logdet, ctx_add, ctx_gate, wpack, wpack_elems, tables, batch, features,
                                        hidden, num_blocks, params_per_feature, cfg, ld_mode, ld_sign, bad_disc, stream);
}
