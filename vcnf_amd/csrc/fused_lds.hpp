// Dynamic-LDS layouts of the three fused RQS layer kernels and of the 128-sample kernel's two-layer form, each stated
// once: the kernel takes its pointers from the offsets, its launcher takes BYTES.  Offsets and sizes are in floats (4
// bytes), BYTES in bytes; a region named X has X (offset) and X_N (floats).  Plain C++17 without a HIP include, so that a
// host program can compile and test it on its own (tests/c_host/fused_lds_check.cpp, fused_lds_pair_check.cpp).
// Template parameters as the kernels': DI identity features, DT
// transformed features, C context features, H hidden units, NBLK residual blocks, K bins.
#pragma once

#include <stddef.h>

namespace vcnf {

// fused_rqs_layer_v6_kernel (fused_layer_v6.hip): 128-sample tiles
template <int DI, int DT, int C, int H, int NBLK, int K>
struct LdsV6 {
  static constexpr int TILE = 128, D = DI + DT, NG = DT / 4;
  static constexpr int NBT = 1 + NBLK * (C > 0 ? 3 : 2);          // trunk bias vectors: b0, then ba | bb (| bc) per block
  static constexpr int BPL = NG * 48 + NBT * (H / 2);             // bias floats per lane-half plane
  // fragment region first (LDS offset 0: every fragment address is a per-lane base + 16-bit immediate): the trunk's
  // activation fragments, then the last layer's weight window of two feature groups (3 row blocks x H / 16 k-steps x
  // hi | lo x 64 lanes x 16 bytes each)
  static constexpr int FRAG = 0, FRAG_N = 2 * 3 * (H / 16) * 2 * 64 * 4;
  static constexpr int XT = FRAG + FRAG_N, XT_N = TILE * (D + 4);               // [128][D + 4]  x in, y out
  static constexpr int CTXF = XT + XT_N, CTXF_N = C > 0 ? 4 * 2 * 64 * 4 : 0;   // context fragments
  static constexpr int TAB = CTXF + CTXF_N, TAB_N = (DI * 3 * (K + 1) + 3) & ~3;   // knot tables of the identity half
  static constexpr int LDT = TAB + TAB_N, LDT_N = TILE;                         // identity-half log|det|
  static constexpr int TFI = LDT + LDT_N, TFI_N = DT;
  static constexpr int IDI = TFI + TFI_N, IDI_N = DI + 4;
  static constexpr int BIAS = IDI + IDI_N, BIAS_N = 2 * BPL;
  static constexpr int LDOLD = BIAS + BIAS_N, LDOLD_N = TILE;                   // accumulate mode: log|det| to add onto
  static constexpr int TFLAG = LDOLD + LDOLD_N, TFLAG_N = 1;
  static constexpr int END = TFLAG + TFLAG_N;
  static constexpr size_t SLACK_BYTES = 3 * 4 + 64;                             // unused tail the launch has always asked for
  static constexpr size_t BYTES = (size_t)END * 4 + SLACK_BYTES;
  static_assert(FRAG == 0 && FRAG + FRAG_N <= XT && XT + XT_N <= CTXF && CTXF + CTXF_N <= TAB && TAB + TAB_N <= LDT &&
                    LDT + LDT_N <= TFI && TFI + TFI_N <= IDI && IDI + IDI_N <= BIAS && BIAS + BIAS_N <= LDOLD &&
                    LDOLD + LDOLD_N <= TFLAG && (size_t)(TFLAG + TFLAG_N) * 4 <= BYTES,
                "regions in order, none overlaps the next, the last ends within BYTES");
  static_assert(XT % 4 == 0 && CTXF % 4 == 0 && TAB % 4 == 0, "16-byte aligned rows and fragments");
};

// fused_rqs_layer_v6_pair_kernel (fused_layer_v6_pair.hip): LdsV6 with the per-layer tables (knot tables, identity-half
// log|det|, index vectors, bias planes) twice, SET floats apart: layer l of the pair adds l * SET to every table
// address.  Where BYTES exceeds kLdsMaxBytes the pair kernel does not exist (FITS).
constexpr size_t kLdsMaxBytes = 160 * 1024;
template <int DI, int DT, int C, int H, int NBLK, int K>
struct LdsV6Pair {
  using One = LdsV6<DI, DT, C, H, NBLK, K>;
  static constexpr int TILE = One::TILE, D = One::D, NG = One::NG, NBT = One::NBT, BPL = One::BPL;
  static constexpr int FRAG = One::FRAG, FRAG_N = One::FRAG_N, XT = One::XT, XT_N = One::XT_N;
  static constexpr int CTXF = One::CTXF, CTXF_N = One::CTXF_N;
  static constexpr int TAB = One::TAB, TAB_N = One::TAB_N, LDT = One::LDT, LDT_N = One::LDT_N;      // set 0, as LdsV6
  static constexpr int TFI = One::TFI, TFI_N = One::TFI_N, IDI = One::IDI, IDI_N = One::IDI_N;
  static constexpr int BIAS = One::BIAS, BIAS_N = One::BIAS_N;
  static constexpr int SET = BIAS + BIAS_N - TAB;                               // tab | ldt | tfi | idi | bias planes
  static constexpr int SET1 = TAB + SET;                                        // set 1: the same five, SET further
  static constexpr int LDOLD = SET1 + SET, LDOLD_N = TILE;
  static constexpr int TFLAG = LDOLD + LDOLD_N, TFLAG_N = 1;
  static constexpr int END = TFLAG + TFLAG_N;
  static constexpr size_t SLACK_BYTES = One::SLACK_BYTES;
  static constexpr size_t BYTES = (size_t)END * 4 + SLACK_BYTES;
  static constexpr bool FITS = BYTES <= kLdsMaxBytes;
  static_assert(SET == TAB_N + LDT_N + TFI_N + IDI_N + BIAS_N && TAB + TAB_N <= LDT && LDT + LDT_N <= TFI &&
                    TFI + TFI_N <= IDI && IDI + IDI_N <= BIAS && CTXF + CTXF_N <= TAB && TAB + SET <= SET1 &&
                    SET1 + SET <= LDOLD && LDOLD + LDOLD_N <= TFLAG && (size_t)(TFLAG + TFLAG_N) * 4 <= BYTES,
                "regions in order, a set is its five regions and nothing else, none overlaps the next, the last ends within BYTES");
  static_assert(SET % 4 == 0 && SET1 % 4 == 0, "16-byte aligned tables in both sets");
};

// fused_rqs_layer_v6s_kernel (fused_layer_v6s.hip): 32-sample tiles, two sets of per-layer tables
template <int DI, int DT, int C, int H, int NBLK, int K>
struct LdsV6s {
  static constexpr int TILE = 32, D = DI + DT, NG = DT / 4;
  static constexpr int TABF = (DI * 3 * (K + 1) + 3) & ~3;
  static constexpr int TSET = TABF + DT + DI + 4 + NG * 96;       // one set: tab | tfi | idi [DI + 4] | last-layer bias
  static constexpr int ACT = 0, ACT_N = 4 * (H / 16) * 64 * 4;                  // [buffer][hi | lo][k-step][lane] x 16 bytes
  static constexpr int XT = ACT + ACT_N, XT_N = TILE * (D + 4);                 // [32][D + 4]  x in, y out
  static constexpr int CTXF = XT + XT_N, CTXF_N = C > 0 ? 2 * 64 * 4 : 0;       // context fragment
  static constexpr int LDT = CTXF + CTXF_N, LDT_N = TILE;                       // identity-half log|det|
  static constexpr int LDX = LDT + LDT_N, LDX_N = 8 * TILE;                     // per-wave shares of the transformed half
  static constexpr int TFLAG = LDX + LDX_N, TFLAG_N = 4;
  static constexpr int TSETS = TFLAG + TFLAG_N, TSETS_N = 2 * TSET;
  static constexpr int END = TSETS + TSETS_N;
  static constexpr size_t SLACK_BYTES = 64;
  static constexpr size_t BYTES = (size_t)END * 4 + SLACK_BYTES;
  static_assert(ACT == 0 && ACT + ACT_N <= XT && XT + XT_N <= CTXF && CTXF + CTXF_N <= LDT && LDT + LDT_N <= LDX &&
                    LDX + LDX_N <= TFLAG && TFLAG + TFLAG_N <= TSETS && (size_t)(TSETS + TSETS_N) * 4 <= BYTES,
                "regions in order, none overlaps the next, the last ends within BYTES");
  static_assert(XT % 4 == 0 && CTXF % 4 == 0 && TSETS % 4 == 0 && TSET % 4 == 0, "16-byte aligned rows and tables");
};

// fused_rqs_layer_kernel (fused_layer.hip, exact fp32): tiles of 4 waves x kCB column blocks x 16 samples
template <int DI, int DT, int C, int H, int NBLK, int K, int kCB>
struct LdsF32 {
  static constexpr int TILE = 4 * kCB * 16, D = DI + DT;
  static constexpr int XT = 0, XT_N = TILE * (D + 4);                           // [TILE][D + 4]  x in, y out
  static constexpr int CT = XT + XT_N, CT_N = TILE * ((C > 0 ? C : 4) + 4);     // [TILE][C + 4] context rows
  static constexpr int TAB = CT + CT_N, TAB_N = (DI * 3 * (K + 1) + 3) & ~3;    // knot tables of the identity half
  static constexpr int TFI = TAB + TAB_N, TFI_N = DT;
  static constexpr int IDI = TFI + TFI_N, IDI_N = DI;
  static constexpr int END = IDI + IDI_N;
  static constexpr size_t SLACK_BYTES = 64;
  static constexpr size_t BYTES = (size_t)END * 4 + SLACK_BYTES;
  static_assert(XT + XT_N <= CT && CT + CT_N <= TAB && TAB + TAB_N <= TFI && TFI + TFI_N <= IDI &&
                    (size_t)(IDI + IDI_N) * 4 <= BYTES,
                "regions in order, none overlaps the next, the last ends within BYTES");
  static_assert(CT % 4 == 0 && TAB % 4 == 0, "16-byte aligned rows");
};

}  // namespace vcnf
