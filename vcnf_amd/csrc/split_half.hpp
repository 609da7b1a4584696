// The fp16 split-half ("fp16x3") vocabulary of v_mfma_f32_32x32x16_f16, stated once: an fp32 value v travels as
// hi = fp16(v), lo = fp16((v - hi) * 2^11); a product keeps hi*hi + (hi*lo + lo*hi) * 2^-11 in fp32 accumulators.
// Reference arithmetic this stands in for: fp32 nn.Linear, normflow/nets/resnet.py:92-106.
// Users: fused_layer_v6.hip, fused_layer_v6s.hip, fused_affine.hip, linear_f16x3.hip, linear_wgrad.hip, gemm_probe.hip
// (split8 / mfma32h); conv1x1.hip, conv3x3_1x1.hip (split_plain, mfma32h_x3, acc_row).  The leaf blocks of the two
// fused RQS layer kernels (fused_layer_v6.hip and its two-layer form, fused_layer_v6s.hip) live here too: mfma32h_x4,
// fold_x4, fold_x3, glu_update, set_quad, acc_logits, split4_raw, split1.  The folds and the GLU update take and return
// their vectors BY VALUE: with the accumulators passed by reference the same source came out on other registers in
// some kernels (profiles/fused_leaf_blocks.md).
#pragma once
#include <hip/hip_runtime.h>

#include "fused_common.hpp"

namespace vcnf {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ floatx16 mfma32h(half8 a, half8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// Row of accumulator register r (0..15) of lane ``lane`` in a 32 x 32 result whose first row is ``first``; the column
// is lane % 32 (measured: profiles/r02_mfma_32x32x16_layout.txt).  Four consecutive registers are four adjacent rows.
__host__ __device__ constexpr int acc_row(int r, int lane, int first = 0) {
  return first + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
}

// One k-step of a split-half product on three independent accumulator chains: hi x hi, hi x lo, lo x hi
// (result: m + (ca + cb) * kLoUnscale).
__device__ __forceinline__ void mfma32h_x3(half8 ah, half8 al, half8 bh, half8 bl, floatx16& m, floatx16& ca, floatx16& cb) {
  m = mfma32h(ah, bh, m);
  ca = mfma32h(ah, bl, ca);
  cb = mfma32h(al, bh, cb);
}

// The same k-step where lo x lo is kept (16- to 48-deep layers on raw inputs: the accumulator rounds once or thrice, so
// the operands' 22 bits are what is left of the error, tests/test_gpu_gemm_error.py): hi x hi, hi x lo + lo x hi on ONE
// chain, lo x lo (result: fold_x4).
__device__ __forceinline__ void mfma32h_x4(half8 ah, half8 al, half8 bh, half8 bl, floatx16& m, floatx16& c, floatx16& c2) {
  m = mfma32h(ah, bh, m);
  c = mfma32h(ah, bl, c);
  c = mfma32h(al, bh, c);
  c2 = mfma32h(al, bl, c2);
}

// m + (c + c2 * 2^-11) * 2^-11: what the chains of mfma32h_x4 add up to
__device__ __forceinline__ floatx16 fold_x4(floatx16 m, floatx16 c, floatx16 c2) {
#pragma unroll
  for (int r = 0; r < 16; ++r) m[r] = fmaf(fmaf(c2[r], kLoUnscale, c[r]), kLoUnscale, m[r]);
  return m;
}

// m + c * 2^-11: the three-product form, hi x lo and lo x hi both on chain c
__device__ __forceinline__ floatx16 fold_x3(floatx16 m, floatx16 c) {
#pragma unroll
  for (int r = 0; r < 16; ++r) m[r] = fmaf(c[r], kLoUnscale, m[r]);
  return m;
}

// GLU residual update h + t * sigmoid(gate) of the ResidualNet block (resnet.py:49-57); the packed gate weights carry
// log2 e: sigmoid(g) = 1 / (1 + 2^-g')
__device__ __forceinline__ floatx16 glu_update(floatx16 h, floatx16 t, floatx16 gate) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float sg = hw_rcp(1.f + hw_exp2(-gate[r]));
    h[r] = fmaf(t[r], sg, h[r]);
  }
  return h;
}

// Quad i (registers 4 i .. 4 i + 3) of an accumulator: bias vectors lie in accumulator order and arrive 16 bytes at a
// time.  The loop over the four quads stays with the caller, load and fill in turn.
__device__ __forceinline__ void set_quad(floatx16& dst, int i, floatx4 q) {
  dst[4 * i + 0] = q[0]; dst[4 * i + 1] = q[1]; dst[4 * i + 2] = q[2]; dst[4 * i + 3] = q[3];
}

// Last layer of the fused RQS kernels: pa holds a feature group's 96 logit rows as three accumulator blocks; the 23
// logits of the lane's feature f2 (0 or 1) are entries 24 f2 + 0 .. 22 (entry v = register v % 16 of block v / 16).
__device__ __forceinline__ void acc_logits(const floatx16 (&pa)[3], int f2, float (&lg)[23]) {
#pragma unroll
  for (int tl = 0; tl < 23; ++tl) lg[tl] = pa[(24 * f2 + tl) >> 4][(24 * f2 + tl) & 15];
}

// Two forms of the split live here.  They give the same bits (both differences are exact) with different instructions:
// split_plain subtracts and scales, split8 scales inside one fma and converts in pairs.  Which one a kernel uses is
// part of its device code - keep a kernel on the form it has.
//
// hi / lo halves of one value, plain form; the running maximum of |v| goes to ``satm`` (beyond 65504: clamped)
struct HiLo {
  _Float16 hi, lo;
};
__device__ __forceinline__ HiLo split_plain(float v, float& satm) {
  satm = fmaxf(satm, __builtin_fabsf(v));
  const float t = __builtin_amdgcn_fmed3f(v, -65504.f, 65504.f);
  const _Float16 h = (_Float16)t;
  return {h, (_Float16)((t - (float)h) * kLoScale)};
}

// hi / lo halves of four RAW inputs (a context row quarter), plain form.  A NaN counts as out of range too: fmaxf
// drops NaNs, the reference propagates them.  The running maximum is pinned like in split8.
__device__ __forceinline__ void split4_raw(const float (&v)[4], half4& hi, half4& lo, float& satm) {
#pragma unroll
  for (int i = 0; i < 4; ++i) satm = fmaxf(satm, v[i] == v[i] ? __builtin_fabsf(v[i]) : __builtin_inff());
  asm volatile("" : "+v"(satm));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float x = __builtin_amdgcn_fmed3f(v[i], -65504.f, 65504.f);
    const _Float16 hv = (_Float16)x;
    hi[i] = hv;
    lo[i] = (_Float16)((x - (float)hv) * kLoScale);
  }
}

// hi / lo halves of eight values, fma form; the running maximum of what was clamped goes to ``satm``
template <bool RELU>
__device__ __forceinline__ void split8(const float (&v)[8], half8& hi, half8& lo, float& satm) {
#pragma unroll
  for (int i = 0; i < 8; i += 2)
    satm = RELU ? fmaxf(fmaxf(satm, v[i]), v[i + 1]) : fmaxf(fmaxf(satm, __builtin_fabsf(v[i])), __builtin_fabsf(v[i + 1]));
  // pin the running maximum here: left alone the compiler sinks these updates to the end of the tile and keeps
  // (spills) every value that ever went through a split until then
  asm volatile("" : "+v"(satm));
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const float x0 = __builtin_amdgcn_fmed3f(v[i], RELU ? 0.f : -65504.f, 65504.f);
    const float x1 = __builtin_amdgcn_fmed3f(v[i + 1], RELU ? 0.f : -65504.f, 65504.f);
    const half2v h2 = __builtin_convertvector(float2v{x0, x1}, half2v);
    hi[i] = h2[0];
    hi[i + 1] = h2[1];
    lo[i] = (_Float16)__builtin_fmaf((float)h2[0], -kLoScale, x0 * kLoScale);
    lo[i + 1] = (_Float16)__builtin_fmaf((float)h2[1], -kLoScale, x1 * kLoScale);
  }
}

// hi / lo halves of one value, the arithmetic of split8 (the caller keeps the running maximum)
template <bool RELU>
__device__ __forceinline__ void split1(float v, _Float16& hi, _Float16& lo) {
  const float x = __builtin_amdgcn_fmed3f(v, RELU ? 0.f : -65504.f, 65504.f);
  hi = (_Float16)x;
  lo = (_Float16)__builtin_fmaf((float)hi, -kLoScale, x * kLoScale);
}

// Pre-scale of ONE operand of a split-half product (the cotangent of the training path's backward GEMMs: a mean loss
// over B samples puts it at 1/B, below fp16's smallest normal 2^-14 from B = 32 768 on, where hi and lo are subnormal
// and keep few bits), per vector of that operand that meets only its own outputs: a row of g in g W, a column of dy
// in dy^T x.  ``amax`` points at the device float holding that vector's largest |value|
// (vcnf_abs_max_rows_cols_f32); the vector is multiplied by 2^e as it is read, e = 14 - floor(log2 amax) - the largest
// |value| lands in [2^14, 2^15), 2^29 of full-precision range below it - and its outputs by 2^-e in the epilogue.
// Both are exact in fp32, so a launch on 2^-k times the operand gives 2^-k times the result bit for bit.  e is kept in [-113, 100] (2^e,
// 2^-e and 2^-e * 2^-11 stay normal fp32).  amax NULL, 0 or not finite: e = 0, the plain clamp-and-count behaviour.
struct PreScale {
  float scale, unscale;
};
__device__ __forceinline__ PreScale pre_scale(const float* amax) {
  PreScale p{1.f, 1.f};
  if (amax) {
    const float m = *amax;
    if (m > 0.f && m < __builtin_inff()) {
      int e = 14 + 127 - (int)((__builtin_bit_cast(unsigned, m) >> 23) & 255u);   // (a subnormal amax reads as 2^-127)
      e = e > 100 ? 100 : (e < -113 ? -113 : e);
      p.scale = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
      p.unscale = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
    }
  }
  return p;
}

}  // namespace vcnf
