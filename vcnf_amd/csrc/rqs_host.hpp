// Host side of the spline units (rqs_kernels.hip, rqs_backward.hip, rqs_f64.hip, the host ends of fused_layer.hip and
// fused_final.hip), each piece stated once: the spline constants a kernel receives, the validation of a spline
// configuration, the dispatch from a run-time bin count to a kernel instance and the capped grid size.  Plain C++17
// without a HIP include, so that a host program can compile and test it on its own (tests/c_host/rqs_host_check.cpp).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/vcnf_hip.h"
#include "host_common.hpp"          // IntList and its dispatcher (the plain C++ part)

namespace vcnf {

// Sits inside the kernels' argument structs: field order and types are part of every kernel's argument layout.
struct RqsConst {
  int K;
  int tails;              // 0 none (K+1 derivative logits), 1 linear (K-1, identity outside),
                          // 2 circular (K: the last knot shares the first knot's logit, identity outside)
  float lo_x, hi_x, span_x;
  float lo_y, hi_y, span_y;
  float min_w, min_h, min_d;
  float free_w, free_h;   // 1 - min*K, rounded from double like the reference's Python scalar
  float wh_scale;
  float edge_logit;       // log(exp(1 - min_d) - 1), splines.py:38
};

// derivative logits per spline
inline int rqs_n_deriv(int tails, int K) {
  return tails == VCNF_TAILS_LINEAR ? K - 1 : tails == VCNF_TAILS_CIRCULAR ? K : K + 1;
}

// The constants of a (valid) configuration.  The forward kernels, their VJPs, the fused layers and the kernel that
// re-evaluates their flagged tiles must agree on these to the bit: spans and free fractions are computed in double
// and rounded once, every product and difference on its own.
inline void rqs_fill_const(const vcnf_rqs_cfg& cfg, RqsConst& c) {
#ifdef __clang__
#pragma clang fp contract(off)      // as the units' own copies were, below rqs_math.hpp's file-wide pragma
#endif
  const int K = cfg.num_bins;
  c.K = K; c.tails = cfg.tails;
  c.lo_x = cfg.left; c.hi_x = cfg.right; c.span_x = (float)((double)cfg.right - (double)cfg.left);
  c.lo_y = cfg.bottom; c.hi_y = cfg.top; c.span_y = (float)((double)cfg.top - (double)cfg.bottom);
  c.min_w = cfg.min_bin_width; c.min_h = cfg.min_bin_height; c.min_d = cfg.min_derivative;
  c.free_w = (float)(1.0 - (double)cfg.min_bin_width * K);
  c.free_h = (float)(1.0 - (double)cfg.min_bin_height * K);
  c.wh_scale = cfg.wh_scale;
  c.edge_logit = (float)log(exp(1.0 - (double)cfg.min_derivative) - 1.0);
}

// The constants of the fp64 spline unit (rqs_f64.hip and both instances of made_sample.hip, whose arithmetic is double):
// the configuration as it is, and the boundary logit of linear tails.  Sits inside those kernels' argument structs.
struct Rqs64Const {
  int K, tails;
  double left, right, bottom, top, min_w, min_h, min_d, wh_scale;
  double edge;            // log(exp(1 - min_d) - 1), splines.py:38
};

inline Rqs64Const rqs_fill_const64(const vcnf_rqs_cfg_f64& cfg) {
  return Rqs64Const{cfg.num_bins, cfg.tails, cfg.left, cfg.right, cfg.bottom, cfg.top, cfg.min_bin_width,
                    cfg.min_bin_height, cfg.min_derivative, cfg.wh_scale, log(exp(1.0 - cfg.min_derivative) - 1.0)};
}

// Validation of a configuration (vcnf_rqs_cfg or vcnf_rqs_cfg_f64), in this order: cfg, bin count, tails, two bins
// for linear tails, bin minima (splines.py:104-107).  The callers test their sizes after it.
template <class Cfg>
inline int rqs_check_cfg(const Cfg* cfg, int max_bins) {
  if (!cfg) return VCNF_ERR_NULL;
  const int K = cfg->num_bins;
  if (K < 1 || K > max_bins) return VCNF_ERR_SHAPE;
  if (cfg->tails != VCNF_TAILS_NONE && cfg->tails != VCNF_TAILS_LINEAR && cfg->tails != VCNF_TAILS_CIRCULAR)
    return VCNF_ERR_UNSUPPORTED;
  if (cfg->tails == VCNF_TAILS_LINEAR && K < 2) return VCNF_ERR_SHAPE;
  if ((double)cfg->min_bin_width * K > 1.0 || (double)cfg->min_bin_height * K > 1.0) return VCNF_ERR_VALUE;
  return VCNF_OK;
}

// Bin counts with kernel instances of their own; the lists differ on purpose.  The spline names of host_common.hpp's
// integer-list dispatcher.
template <int... Ks>
using BinList = IntList<Ks...>;
constexpr BinList<4, 8, 10, 16> kBins{};               // every other count: the generic instance (run-time K)
constexpr BinList<8, 10, 16> kBins64{};                // fp64 kernels, generic instance likewise
constexpr BinList<4, 8, 10, 16, 32> kBinsIdHalf{};     // identity half: no generic instance

template <int... Ks>
inline bool in_bins(BinList<Ks...> list, int K) {
  return in_list(list, K);
}

// f(std::integral_constant<int, K>{}) if K is one of Ks (true), else nothing (false)
template <int... Ks, class F>
inline bool with_bins_only(BinList<Ks...> list, int K, F&& f) {
  return with_listed_only(list, K, std::forward<F>(f));
}

// the same, and f(std::integral_constant<int, 0>{}) - the generic instance - for every other K
template <int... Ks, class F>
inline void with_bins(BinList<Ks...> list, int K, F&& f) {
  if (!with_bins_only(list, K, f)) f(std::integral_constant<int, 0>{});
}

// workgroups of ``block`` threads for n elements, at most ``cap`` (the kernels stride over the rest)
inline unsigned elem_blocks(long long n, int block, long long cap) {
  const long long blocks = (n + block - 1) / block;
  return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace vcnf
