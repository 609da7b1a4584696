// Host-only check of csrc/fused_lds.hpp (g++ -std=c++17, no HIP): for every instance of the three fused RQS layer
// kernels (DI = DT in {16, 32}, C in {0, 16}, NBLK in {1, 2, 3}; H = 128, K = 8) the layout's BYTES equals the byte count
// the launchers computed on their own before the header existed - spelled out here literally - and the regions are in
// increasing order without overlap.
#include <stddef.h>
#include <stdio.h>

#include "fused_lds.hpp"

using namespace vcnf;

static int failures = 0, instances = 0;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      printf("FAILED line %d (DI %d, C %d, NBLK %d): %s\n", __LINE__, DI, C, NBLK, #cond);  \
      ++failures;                                                                           \
    }                                                                                       \
  } while (0)

// regions as (offset, floats) pairs in layout order: increasing, each ends at or below the start of the next, the last
// ends within ``bytes``
static bool ordered(const int (*reg)[2], int n, size_t bytes) {
  for (int i = 0; i < n; ++i) {
    if (reg[i][1] < 0) return false;
    if (i + 1 < n && (reg[i + 1][0] < reg[i][0] || reg[i][0] + reg[i][1] > reg[i + 1][0])) return false;
  }
  return (size_t)(reg[n - 1][0] + reg[n - 1][1]) * 4 <= bytes;
}

template <int DI, int C, int NBLK>
static void check_instance() {
  constexpr int DT = DI, D = DI + DT, H = 128, K = 8;
  ++instances;
  {
    using S = LdsV6<DI, DT, C, H, NBLK, K>;
    const size_t NBT = 1 + NBLK * (C ? 3 : 2);
    const size_t parent = ((size_t)128 * (D + 4) + ((DI * 27 + 3) & ~3) + 256 + D + 8 + (DT / 4) * 96 + NBT * 128) * 4 +
                          (C ? 8192 : 0) + 98304 + 64;
    CHECK(S::BYTES == parent);
    CHECK(S::FRAG == 0);
    CHECK((size_t)S::END * 4 + S::SLACK_BYTES == S::BYTES);
    const int reg[][2] = {{S::FRAG, S::FRAG_N}, {S::XT, S::XT_N},     {S::CTXF, S::CTXF_N},   {S::TAB, S::TAB_N},
                          {S::LDT, S::LDT_N},   {S::TFI, S::TFI_N},   {S::IDI, S::IDI_N},     {S::BIAS, S::BIAS_N},
                          {S::LDOLD, S::LDOLD_N}, {S::TFLAG, S::TFLAG_N}};
    CHECK(ordered(reg, 10, S::BYTES));
  }
  {
    using S = LdsV6s<DI, DT, C, H, NBLK, K>;
    const size_t TSET = ((DI * 27 + 3) & ~3) + DT + DI + 4 + (DT / 4) * 96;
    const size_t parent = (size_t)4 * 8 * 64 * 16 + (C ? 2048 : 0) + ((size_t)32 * (D + 4) + 32 + 256 + 4 + 2 * TSET) * 4 + 64;
    CHECK(S::BYTES == parent);
    CHECK((size_t)S::END * 4 + S::SLACK_BYTES == S::BYTES);
    const int reg[][2] = {{S::ACT, S::ACT_N}, {S::XT, S::XT_N},       {S::CTXF, S::CTXF_N},  {S::LDT, S::LDT_N},
                          {S::LDX, S::LDX_N}, {S::TFLAG, S::TFLAG_N}, {S::TSETS, S::TSETS_N}};
    CHECK(ordered(reg, 7, S::BYTES));
  }
  {
    using S = LdsF32<DI, DT, C, H, NBLK, K, 2>;
    const size_t parent = ((size_t)128 * (D + 4) + (size_t)128 * ((C ? C : 4) + 4) + ((DI * 27 + 3) & ~3) + D) * 4 + 64;
    CHECK(S::BYTES == parent);
    CHECK((size_t)S::END * 4 + S::SLACK_BYTES == S::BYTES);
    const int reg[][2] = {{S::XT, S::XT_N}, {S::CT, S::CT_N}, {S::TAB, S::TAB_N}, {S::TFI, S::TFI_N}, {S::IDI, S::IDI_N}};
    CHECK(ordered(reg, 5, S::BYTES));
  }
}

template <int DI, int C>
static void check_blocks() {
  check_instance<DI, C, 1>();
  check_instance<DI, C, 2>();
  check_instance<DI, C, 3>();
}

int main() {
  check_blocks<16, 0>();
  check_blocks<16, 16>();
  check_blocks<32, 0>();
  check_blocks<32, 16>();
  // the ordering check itself: an overlap and an overrun are seen
  const int overlap[][2] = {{0, 8}, {4, 4}}, overrun[][2] = {{0, 8}, {8, 9}};
  if (ordered(overlap, 2, 64) || ordered(overrun, 2, 64)) {
    printf("FAILED: ordered() accepts an overlap or an overrun\n");
    ++failures;
  }
  if (failures || instances != 12) return 1;
  printf("fused_lds_check ok (%d instances x 3 layouts)\n", instances);
  return 0;
}
