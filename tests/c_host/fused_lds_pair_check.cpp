// Host-only check of LdsV6Pair in csrc/fused_lds.hpp (g++ -std=c++17, no HIP), the layout of the two-layer form of the
// 128-sample-tile fused RQS layer kernel: for every shape of the family (DI = DT in {16, 32}, C in {0, 16}, NBLK in
// {1, 2, 3}; H = 128, K = 8) the regions are in increasing order without overlap, the second table set lies SET floats
// behind the first and holds the same five regions, the byte count is LdsV6's plus one table set - spelled out here
// literally - and FITS says exactly whether that is within the 163 840 bytes of a workgroup.  Prints one line per shape
// ("pair DI C NBLK bytes fits") for tests/test_fused_lds_pair.py to hold against the library's query.
#include <stddef.h>
#include <stdio.h>

#include "fused_lds.hpp"

using namespace vcnf;

static int failures = 0, instances = 0, fitting = 0;
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
  using S = LdsV6Pair<DI, DT, C, H, NBLK, K>;
  using One = LdsV6<DI, DT, C, H, NBLK, K>;
  const size_t NBT = 1 + NBLK * (C ? 3 : 2);
  // one table set: knot tables, identity-half log|det|, transform and identity index vectors, two bias planes
  const size_t set_bytes = ((size_t)((DI * 27 + 3) & ~3) + 128 + DT + (DI + 4) + 2 * ((DT / 4) * 48 + NBT * 64)) * 4;
  CHECK((size_t)S::SET * 4 == set_bytes);
  CHECK(S::BYTES == One::BYTES + set_bytes);
  CHECK((size_t)S::END * 4 + S::SLACK_BYTES == S::BYTES);
  CHECK(S::FRAG == 0 && S::SET % 4 == 0);
  const int o = S::SET;
  const int reg[][2] = {{S::FRAG, S::FRAG_N},   {S::XT, S::XT_N},         {S::CTXF, S::CTXF_N},
                        {S::TAB, S::TAB_N},     {S::LDT, S::LDT_N},       {S::TFI, S::TFI_N},
                        {S::IDI, S::IDI_N},     {S::BIAS, S::BIAS_N},     {S::TAB + o, S::TAB_N},
                        {S::LDT + o, S::LDT_N}, {S::TFI + o, S::TFI_N},   {S::IDI + o, S::IDI_N},
                        {S::BIAS + o, S::BIAS_N}, {S::LDOLD, S::LDOLD_N}, {S::TFLAG, S::TFLAG_N}};
  CHECK(ordered(reg, 15, S::BYTES));
  CHECK(S::SET1 == S::TAB + o && S::BIAS + S::BIAS_N == S::SET1);     // set 0 ends where set 1 begins
  CHECK(S::FITS == (S::BYTES <= (size_t)163840));
  // everything up to the first table set is LdsV6's: the kernel body addresses both layouts alike
  CHECK(S::XT == One::XT && S::CTXF == One::CTXF && S::TAB == One::TAB && S::BIAS == One::BIAS && S::BPL == One::BPL);
  if (DI == 32 && C == 16 && NBLK == 2) {                             // config C3
    CHECK(One::BYTES == 152800 && set_bytes == 10896 && S::BYTES == 163696 && S::FITS);
  }
  if (DI == 32 && C == 16 && NBLK == 3) CHECK(!S::FITS);
  fitting += S::FITS ? 1 : 0;
  printf("pair %d %d %d %zu %d\n", DI, C, NBLK, (size_t)S::BYTES, S::FITS ? 1 : 0);
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
  if (failures || instances != 12 || fitting != 11) return 1;
  printf("fused_lds_pair_check ok (%d instances, %d with the pair form)\n", instances, fitting);
  return 0;
}
