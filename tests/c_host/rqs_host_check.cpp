// Host-only check of csrc/rqs_host.hpp (g++ -std=c++17, no HIP): the bin-count dispatcher over its three lists,
// host_common.hpp's with_flags, the spline constants of one configuration against the expressions the units carried
// before the header existed, the fp64 constants (rqs_fill_const64) field by field, and the number of derivative logits.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rqs_host.hpp"

using namespace vcnf;

static int failures = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      printf("FAILED line %d: %s\n", __LINE__, #cond);          \
      ++failures;                                               \
    }                                                           \
  } while (0)

template <int... Ks>
static void check_list(BinList<Ks...> list, const char* name) {
  const int members[] = {Ks...};
  for (int K = 1; K <= 1024; K = K < 70 ? K + 1 : 1024) {
    bool in_list = false;
    for (int m : members) in_list = in_list || m == K;
    int got = -1, calls = 0;
    with_bins(list, K, [&](auto kt) { got = decltype(kt)::value; ++calls; });
    if (got != (in_list ? K : 0) || calls != 1) {
      printf("FAILED with_bins(%s, %d): handed over %d in %d calls\n", name, K, got, calls);
      ++failures;
    }
    got = -1, calls = 0;
    const bool found = with_bins_only(list, K, [&](auto kt) { got = decltype(kt)::value; ++calls; });
    if (found != in_list || got != (in_list ? K : -1) || calls != (in_list ? 1 : 0)) {
      printf("FAILED with_bins_only(%s, %d): %d, handed over %d in %d calls\n", name, K, (int)found, got, calls);
      ++failures;
    }
    if (K == 1024) break;
  }
}

// with_flags over N flags: each of the 2^N combinations reaches f once, with the constants of its booleans in their
// order, and f's status comes back
static int flag_bits() { return 0; }
template <class B, class... Bs>
static int flag_bits(B b, Bs... rest) {
  static_assert(std::is_same<B, std::true_type>::value || std::is_same<B, std::false_type>::value, "a bool_constant");
  return (B::value ? 1 << sizeof...(Bs) : 0) | flag_bits(rest...);
}

template <class... Bools>
static void check_flags_at(int want, Bools... flags) {
  int got = -1, calls = 0;
  const int status = with_flags([&](auto... c) { got = flag_bits(c...); ++calls; return 100 + got; }, flags...);
  if (got != want || calls != 1 || status != 100 + want) {
    printf("FAILED with_flags, %d flags, combination %d: constants %d in %d calls, status %d\n", (int)sizeof...(Bools),
           want, got, calls, status);
    ++failures;
  }
}

static void check_flags() {
  check_flags_at(0);
  for (int a = 0; a < 2; ++a) {
    check_flags_at(a, a != 0);
    for (int b = 0; b < 2; ++b) {
      check_flags_at(a << 1 | b, a != 0, b != 0);
      for (int c = 0; c < 2; ++c) check_flags_at(a << 2 | b << 1 | c, a != 0, b != 0, c != 0);
    }
  }
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }
static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

// rqs_fill_const64: every field is the configuration's own, the boundary logit its one expression
static void check_const64(int tails, double bound, double min_w, double min_h, double min_d, double scale) {
  vcnf_rqs_cfg_f64 cfg;
  cfg.num_bins = 10; cfg.tails = tails;
  cfg.left = -bound; cfg.right = bound; cfg.bottom = -0.5 * bound; cfg.top = 2.0 * bound;
  cfg.min_bin_width = min_w; cfg.min_bin_height = min_h; cfg.min_derivative = min_d; cfg.wh_scale = scale;
  const Rqs64Const c = rqs_fill_const64(cfg);
  CHECK(c.K == cfg.num_bins);
  CHECK(c.tails == cfg.tails);
  CHECK(same_bits(c.left, cfg.left));
  CHECK(same_bits(c.right, cfg.right));
  CHECK(same_bits(c.bottom, cfg.bottom));
  CHECK(same_bits(c.top, cfg.top));
  CHECK(same_bits(c.min_w, cfg.min_bin_width));
  CHECK(same_bits(c.min_h, cfg.min_bin_height));
  CHECK(same_bits(c.min_d, cfg.min_derivative));
  CHECK(same_bits(c.wh_scale, cfg.wh_scale));
  CHECK(same_bits(c.edge, log(exp(1.0 - cfg.min_derivative) - 1.0)));
}

int main() {
  check_list(kBins, "kBins");
  check_list(kBins64, "kBins64");
  check_list(kBinsIdHalf, "kBinsIdHalf");
  check_flags();

  // 8 bins, linear tails, bound 3, the default floors
  vcnf_rqs_cfg cfg_v;
  cfg_v.num_bins = 8; cfg_v.tails = VCNF_TAILS_LINEAR;
  cfg_v.left = -3.f; cfg_v.right = 3.f; cfg_v.bottom = -3.f; cfg_v.top = 3.f;
  cfg_v.min_bin_width = 1e-3f; cfg_v.min_bin_height = 1e-3f; cfg_v.min_derivative = 1e-3f; cfg_v.wh_scale = 1.f;
  const vcnf_rqs_cfg* cfg = &cfg_v;
  RqsConst c;
  memset(&c, 0xff, sizeof c);
  rqs_fill_const(*cfg, c);
  const int K = cfg->num_bins;
  CHECK(c.K == K);
  CHECK(c.tails == cfg->tails);
  CHECK(same_bits(c.lo_x, cfg->left));
  CHECK(same_bits(c.hi_x, cfg->right));
  CHECK(same_bits(c.span_x, (float)((double)cfg->right - (double)cfg->left)));
  CHECK(same_bits(c.lo_y, cfg->bottom));
  CHECK(same_bits(c.hi_y, cfg->top));
  CHECK(same_bits(c.span_y, (float)((double)cfg->top - (double)cfg->bottom)));
  CHECK(same_bits(c.min_w, cfg->min_bin_width));
  CHECK(same_bits(c.min_h, cfg->min_bin_height));
  CHECK(same_bits(c.min_d, cfg->min_derivative));
  CHECK(same_bits(c.free_w, (float)(1.0 - (double)cfg->min_bin_width * K)));
  CHECK(same_bits(c.free_h, (float)(1.0 - (double)cfg->min_bin_height * K)));
  CHECK(same_bits(c.wh_scale, cfg->wh_scale));
  CHECK(same_bits(c.edge_logit, (float)log(exp(1.0 - (double)cfg->min_derivative) - 1.0)));
  CHECK(sizeof(RqsConst) == 15 * 4);               // 2 ints + 13 floats: part of every kernel's argument layout
  CHECK(rqs_check_cfg(cfg, 64) == VCNF_OK);

  // the fp64 constants: the three tails modes at the default floors, and one other set of floors
  check_const64(VCNF_TAILS_NONE, 1.0, 1e-3, 1e-3, 1e-3, 1.0);
  check_const64(VCNF_TAILS_LINEAR, 3.0, 1e-3, 1e-3, 1e-3, 1.0);
  check_const64(VCNF_TAILS_CIRCULAR, 3.141592653589793, 1e-3, 1e-3, 1e-3, 1.0);
  check_const64(VCNF_TAILS_LINEAR, 5.0, 2e-2, 5e-3, 0.25, 0.125);
  CHECK(sizeof(Rqs64Const) == 2 * 4 + 9 * 8);      // part of the fp64 kernels' argument layout

  CHECK(rqs_n_deriv(VCNF_TAILS_LINEAR, 8) == 7);
  CHECK(rqs_n_deriv(VCNF_TAILS_CIRCULAR, 8) == 8);
  CHECK(rqs_n_deriv(VCNF_TAILS_NONE, 8) == 9);

  CHECK(elem_blocks(1, 256, 4096) == 1);
  CHECK(elem_blocks(257, 256, 4096) == 2);
  CHECK(elem_blocks(1LL << 40, 256, 4096) == 4096);

  if (failures) return 1;
  printf("rqs_host_check ok\n");
  return 0;
}
