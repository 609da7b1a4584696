// Shapes and the dynamic-LDS layout of the full-covariance base kernels (mvn_base.hip), each stated once: the kernels
// take their pointers from the offsets, the launchers take bytes().  Offsets and sizes are in elements of the working
// type T.  Plain C++17 without a HIP include, so that a host program can compile and check it on its own
// (tests/c_host/mvn_lds_check.cpp).
//
// The triangular operand lives in LDS as 4 x 4 blocks of its lower triangle, zero where a block crosses the diagonal or
// the edge: with Dp = D rounded up to 4 and nb = Dp / 4, block row I holds the rows 4I .. 4I + 3, each 4 (I + 1)
// elements long, so every run of four entries a thread multiplies with is one aligned 16-byte (fp64: 32-byte) read.
// 8 nb (nb + 1) elements: 8448 at D = 128 against 16384 for the square.
#pragma once

#include <stddef.h>

#include "../../include/vcnf_hip.h"

namespace vcnf_mvn {

constexpr int kMaxD = VCNF_MVN_MAX_DIM;       // features: VCNF_ERR_SHAPE beyond
constexpr int kBlock = 256;                   // threads per workgroup
constexpr int kMaxBlocksOwned = 3;            // 4 x 4 blocks of the outer-product sum a thread keeps in registers

// samples per tile: a thread (sample s, part p) of the kBlock / tile_rows parts takes the block rows p, p + parts, ...
template <typename T>
constexpr int tile_rows() { return sizeof(T) == 4 ? 64 : 32; }

constexpr int padded(int D) { return (D + 3) & ~3; }
constexpr int block_rows(int D) { return padded(D) / 4; }
constexpr int tri_blocks(int D) { return block_rows(D) * (block_rows(D) + 1) / 2; }
constexpr int tri_elems(int D) { return 8 * block_rows(D) * (block_rows(D) + 1); }
// offset of row i of the packed triangle; the row has 4 (i / 4 + 1) elements
constexpr int tri_row(int i) { return 8 * (i / 4) * (i / 4 + 1) + (i % 4) * 4 * (i / 4 + 1); }
// elements between the rows of a sample tile: Dp or Dp + 4, whichever is an odd number of 16-byte fp32 packs, so that
// the 16 lanes of one ds_read_b128 group, each on its own row, cover the 64 banks once
constexpr int row_stride(int D) { return (padded(D) / 4) % 2 ? padded(D) : padded(D) + 4; }

// TRI the packed triangle | LOC [Dp] | A [tile][stride] the streamed operand | B [tile][stride] the second tile of the
// sampling kernel and the VJPs | Q [kBlock] the parts' partial sums | S [3][tile] per-sample scalars
struct Layout {
  int TRI, LOC, A, B, Q, S, END;
};

template <typename T>
constexpr Layout layout(int D, bool two_tiles) {
  Layout l{};
  const int tile = tile_rows<T>() * row_stride(D);
  l.TRI = 0;
  l.LOC = l.TRI + tri_elems(D);
  l.A = l.LOC + padded(D);
  l.B = l.A + tile;
  l.Q = l.B + (two_tiles ? tile : 0);
  l.S = l.Q + kBlock;
  l.END = l.S + 3 * tile_rows<T>();
  return l;
}

template <typename T>
constexpr size_t bytes(int D, bool two_tiles) { return (size_t)layout<T>(D, two_tiles).END * sizeof(T); }

constexpr size_t kLdsPerCu = 160 * 1024, kLdsNoAttribute = 64 * 1024;

static_assert(tri_blocks(kMaxD) <= kMaxBlocksOwned * kBlock, "every 4 x 4 block of the outer-product sum has an owner");
static_assert(padded(kMaxD) <= kBlock, "one thread per column of d_loc");
static_assert(bytes<float>(kMaxD, true) <= kLdsPerCu && bytes<double>(kMaxD, true) <= kLdsPerCu, "the largest launch fits a CU");
static_assert(bytes<float>(kMaxD, true) == 103680 && bytes<double>(kMaxD, true) == 139008 && bytes<float>(kMaxD, false) == 69888 &&
                  bytes<double>(kMaxD, false) == 105216, "the byte counts profiles/mvn_base.md quotes");

}  // namespace vcnf_mvn
