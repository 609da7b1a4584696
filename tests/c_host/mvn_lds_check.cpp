// csrc/mvn_lds.hpp on its own (plain C++17, no HIP): for every D, both working types and both layouts, the regions are
// in order and 16-byte (fp64: 32-byte) aligned, the packed triangle's rows tile it exactly, the tile rows keep 16 lanes
// of a 16-byte read on distinct banks, and the byte count fits a CU.
#include <stdio.h>

#include <initializer_list>

#include "mvn_lds.hpp"

using namespace vcnf_mvn;

template <typename T>
static int check(int D, bool two) {
  const Layout l = layout<T>(D, two);
  int bad = 0;
  bad += !(l.TRI == 0 && l.TRI + tri_elems(D) == l.LOC && l.LOC + padded(D) == l.A && l.A < l.B && l.B <= l.Q &&
           l.Q + kBlock == l.S && l.S + 3 * tile_rows<T>() == l.END);
  bad += (l.B - l.A) != tile_rows<T>() * row_stride(D);
  bad += (l.Q - l.B) != (two ? tile_rows<T>() * row_stride(D) : 0);
  for (int off : {l.LOC, l.A, l.B, l.Q, l.S}) bad += off % 4 != 0;
  bad += bytes<T>(D, two) != (size_t)l.END * sizeof(T) || bytes<T>(D, two) > kLdsPerCu;
  // rows of the packed triangle: consecutive, 4 (i / 4 + 1) long, ending at tri_elems
  int at = 0;
  for (int i = 0; i < padded(D); ++i) {
    bad += tri_row(i) != at;
    at += 4 * (i / 4 + 1);
  }
  bad += at != tri_elems(D);
  bad += row_stride(D) < padded(D) || row_stride(D) % 4 != 0 || (row_stride(D) / 4) % 2 != 1;
  bad += tri_blocks(D) > kMaxBlocksOwned * kBlock || kBlock % tile_rows<T>() != 0;
  if (bad) printf("D = %d, %zu-byte type, two tiles %d: %d checks failed\n", D, sizeof(T), (int)two, bad);
  return bad;
}

int main() {
  int bad = 0;
  for (int D = 1; D <= kMaxD; ++D)
    for (int two = 0; two < 2; ++two) bad += check<float>(D, two) + check<double>(D, two);
  if (bad) return 1;
  printf("mvn_lds_check ok (%d sizes x 2 types x 2 layouts)\n", kMaxD);
  return 0;
}
