// Weight and bias gradient of a dense layer of the conditioner for LARGE batches:
//     dW[o, i] = sum_b dy[b, o] x[b, i]        db[o] = sum_b dy[b, o]            x [B, IN], dy [B, OUT]
// (the reference gets both from autograd over nets/resnet.py:92-106, i.e. torch.nn.functional.linear's backward).
// These are GEMMs whose reduction runs over the batch and whose output is tiny (128 x 128 for a hidden layer of
// config C3): PyTorch-ROCm hands them to a library kernel that splits the OUTPUT into 32 x 32 tiles - 16 workgroups
// on a 256-CU device, 223 us per 131 072-sample layer, 36 % of the whole training step (profiles/
// r01_train_step_kernel_stats.csv) - and the bias gradient to a separate column-sum kernel.  Here the BATCH is split:
// workgroup = (block of 128 output rows, slice of the batch); its 4 waves own two 16-row blocks each and all column
// blocks, accumulate dy^T x of their slice on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation) with both
// operands read straight from global memory in matrix-operand layout (lane = 16 q + m: sample 4 j + q of k-step j,
// column m of the block - 64-byte row segments), sum the bias gradient from the same dy values, and write one partial
// [OUT, IN] (+ [OUT]) per slice; a second small kernel adds the slices in a fixed order (deterministic).
// IN: multiple of 16 up to 128; any OUT.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vcnf_hip.h"
#include "fused_common.hpp"
#include "split_half.hpp"

namespace vcnf {

struct WgradArgs {
  const float* x;
  const float* dy;
  float* part_w;      // [S][OUT][IN]
  float* part_b;      // [S][OUT] or null
  long long B, chunk; // samples per slice (multiple of 16)
  int IN, OUT, S, row_tiles;
  int col_tiles;      // split-half form: workgroups per row tile (64 input columns each)
  int relu_x;         // split-half form: the layer's input is relu(x) (x = the residual stream, nets/resnet.py:42)
  int32_t* sat;       // split-half form: tiles that clamped a value at +-65504 (or NULL)
  const float* amax;  // split-half form: largest |dy[:, o]| per output row o [OUT] or NULL: split_half.hpp::pre_scale
};

constexpr int kWgBlock = 256;

template <int NB>   // IN = 16 NB
__global__ __launch_bounds__(kWgBlock) void linear_wgrad_kernel(const WgradArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m16 = lane & 15;
  const int q = lane >> 4;
  const int rt = blockIdx.x % a.row_tiles;
  const int s = blockIdx.x / a.row_tiles;
  const int o0 = rt * 128 + wave * 32;                 // this wave's 32 output rows
  const long long b_lo = (long long)s * a.chunk;
  const long long b_hi = b_lo + a.chunk < a.B ? b_lo + a.chunk : a.B;
  floatx4 acc[2][NB];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bsum[2] = {0.f, 0.f};
  const bool rok0 = o0 + m16 < a.OUT, rok1 = o0 + 16 + m16 < a.OUT;
  constexpr int U = 4;                                 // k-steps (4 samples each) requested together
  for (long long b0 = b_lo; b0 < b_hi; b0 += 4 * U) {
    float av[U][2], xv[U][NB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long b = b0 + 4 * u + q;
      const bool ok = b < b_hi;
      const float* dyr = a.dy + b * a.OUT + o0 + m16;
      av[u][0] = (ok && rok0) ? dyr[0] : 0.f;
      av[u][1] = (ok && rok1) ? dyr[16] : 0.f;
      const float* xr = a.x + b * a.IN + m16;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) xv[u][nb] = ok ? xr[16 * nb] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bsum[0] += av[u][0];
      bsum[1] += av[u][1];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        acc[0][nb] = mfma4(av[u][0], xv[u][nb], acc[0][nb]);
        acc[1][nb] = mfma4(av[u][1], xv[u][nb], acc[1][nb]);
      }
    }
  }
  // accumulator register r of lane (q, m16): row 4 q + r of the 16-row block, column m16 of the column block
  float* pw = a.part_w + (long long)s * a.OUT * a.IN;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = o0 + 16 * mb + 4 * q + r;
      if (row < a.OUT) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) pw[(long long)row * a.IN + 16 * nb + m16] = acc[mb][nb][r];
      }
    }
  if (a.part_b) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      float t = bsum[mb];
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      const int row = o0 + 16 * mb + m16;
      if (q == 0 && row < a.OUT) a.part_b[(long long)s * a.OUT + row] = t;
    }
  }
}

// The same partial products on the fp16 split-half matrix path (round 3): dy^T x of the slice on
// v_mfma_f32_32x32x16_f16 with both operands split in registers (hi*hi + (hi*lo + lo*hi) * 2^-11, fp32 accumulation -
// the arithmetic of split_half.hpp; the reduction runs over the 16 samples of a k-step, so the accumulator rounds once
// per 16 samples instead of once per 4).  Wave = 32 output rows x all column blocks of 32 inputs; a lane's eight
// k-slots are eight consecutive samples of one column, i.e. eight 4-byte loads whose 32 lanes cover a 128-byte row
// segment - no LDS, no barrier.  The exact-fp32 kernel above is bound by its matrix instructions (157 TFLOP/s peak:
// 30 us for 131 072 x 128 x 128, 157 us for the 736-row last layer); this one by the vector work of the splits
// (~10 / 65 us).  Values beyond +-65504 are clamped and counted.
template <int KB>   // column blocks of 32 inputs per workgroup (1 or 2); wider layers are split over col_tiles workgroups
__global__ __launch_bounds__(kWgBlock, 2) void linear_wgrad_f16x3_kernel(const WgradArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c32 = lane & 31, kg = lane >> 5;
  const int ct = blockIdx.x % a.col_tiles;             // column tiles are neighbours in the grid: the second one
  const int rt = (blockIdx.x / a.col_tiles) % a.row_tiles;   // finds the slice's dy rows in L2
  const int s = blockIdx.x / (a.col_tiles * a.row_tiles);
  const int o0 = rt * 128 + wave * 32;                 // this wave's 32 output rows
  const int i0 = ct * 32 * KB;                         // first input column of this workgroup
  const long long b_lo = (long long)s * a.chunk;
  const long long b_hi = b_lo + a.chunk < a.B ? b_lo + a.chunk : a.B;
  floatx16 mainv[KB], corr[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) { mainv[kb] = floatx16{}; corr[kb] = floatx16{}; }
  float bsum = 0.f, satm = 0.f;
  const bool rok = o0 + c32 < a.OUT;
  // column o of dy travels as dy * 2^e(o) (this lane's A values are all of column o0 + c32); row o of dW and db[o]
  // leave as sums * 2^-e(o)
  const PreScale ps = pre_scale(a.amax && rok ? a.amax + o0 + c32 : nullptr);
  bool cok[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) cok[kb] = i0 + 32 * kb + c32 < a.IN;
  // A: lane (c32, kg) holds row o0 + c32, k-slots = samples b0 + 8 kg + i;  B: column i0 + 32 kb + c32, same samples.
  // Two k-steps (32 samples) per round, the NEXT round's values requested before this round's are split and
  // multiplied: a round is ~0.3 us of vector / matrix work against ~2 us of memory latency, and two waves per SIMD do
  // not hide it (first version, one k-step at a time: 2.8 us per k-step).
  constexpr int U = 2;
  float av[2][U][8], xv[2][U][KB][8];
  // buffer loads through a descriptor rebuilt per round (base = the round's first row, size = what is left of the
  // slice: reads past the slice return 0 by the hardware range check, which covers the per-lane offset): the per-lane
  // part is (column, sample half) plus a small row offset - as 64-bit per-lane addresses the 48 requests of a round
  // held 96 registers of addresses (178 spilled).  Lanes of rows / columns outside the layer point far past the end.
  const int voa = rok ? (8 * kg * a.OUT + o0 + c32) * 4 : 0x7FF00000;
  int vox[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) vox[kb] = cok[kb] ? (8 * kg * a.IN + i0 + 32 * kb + c32) * 4 : 0x7FF00000;
#define VCNF_WG_LOAD(BUF, B0)                                                             \
  {                                                                                       \
    const long long rb_ = min((long long)(B0), b_hi);                                     \
    const __amdgpu_buffer_rsrc_t dyr_ = __builtin_amdgcn_make_buffer_rsrc(                \
        const_cast<float*>(a.dy) + rb_ * a.OUT, 0, (unsigned)((b_hi - rb_) * a.OUT * 4), 0x00020000); \
    const __amdgpu_buffer_rsrc_t xr_ = __builtin_amdgcn_make_buffer_rsrc(                 \
        const_cast<float*>(a.x) + rb_ * a.IN, 0, (unsigned)((b_hi - rb_) * a.IN * 4), 0x00020000); \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                                       \
      _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                     \
        av[BUF][u][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dyr_, voa + (16 * u + i) * a.OUT * 4, 0, 0)); \
        _Pragma("unroll") for (int kb = 0; kb < KB; ++kb)                                 \
          xv[BUF][u][kb][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr_, vox[kb] + (16 * u + i) * a.IN * 4, 0, 0)); \
      }                                                                                   \
    }                                                                                     \
  }
#define VCNF_WG_COMPUTE(BUF)                                                              \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                                         \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                       \
      av[BUF][u][i] *= ps.scale;                                                          \
      bsum += av[BUF][u][i];                                                              \
      satm = fmaxf(satm, av[BUF][u][i] == av[BUF][u][i] ? 0.f : __builtin_inff());        \
    }                                                                                     \
    half8 ah, al;                                                                         \
    split8<false>(av[BUF][u], ah, al, satm);                                              \
    _Pragma("unroll") for (int kb = 0; kb < KB; ++kb) {                                   \
      _Pragma("unroll") for (int i = 0; i < 8; ++i)                                       \
        satm = fmaxf(satm, xv[BUF][u][kb][i] == xv[BUF][u][kb][i] ? 0.f : __builtin_inff()); \
      half8 bh, bl;                                                                       \
      if (a.relu_x) split8<true>(xv[BUF][u][kb], bh, bl, satm);                           \
      else split8<false>(xv[BUF][u][kb], bh, bl, satm);                                   \
      mainv[kb] = mfma32h(ah, bh, mainv[kb]);                                             \
      corr[kb] = mfma32h(ah, bl, corr[kb]);                                               \
      corr[kb] = mfma32h(al, bh, corr[kb]);                                               \
    }                                                                                     \
  }
  if (o0 < a.OUT) {
    VCNF_WG_LOAD(0, b_lo)
    for (long long b0 = b_lo; b0 < b_hi; b0 += 32 * U) {
      VCNF_WG_LOAD(1, b0 + 16 * U)                    // (past the slice: every lane reads 0)
      __builtin_amdgcn_sched_barrier(0);
      VCNF_WG_COMPUTE(0)
      __builtin_amdgcn_sched_barrier(0);
      VCNF_WG_LOAD(0, b0 + 32 * U)
      __builtin_amdgcn_sched_barrier(0);
      VCNF_WG_COMPUTE(1)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#undef VCNF_WG_LOAD
#undef VCNF_WG_COMPUTE
  // accumulator register r of lane (c32, kg): row 8 (r / 4) + 4 kg + r % 4 of the 32-row block, column c32 of block kb
  float* pw = a.part_w + (long long)s * a.OUT * a.IN;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = o0 + 8 * (r >> 2) + 4 * kg + (r & 3);
    if (row < a.OUT) {
      const float unscale = pre_scale(a.amax ? a.amax + row : nullptr).unscale;
      const float lo_unscale = kLoUnscale * unscale;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        if (cok[kb]) pw[(long long)row * a.IN + i0 + 32 * kb + c32] = fmaf(corr[kb][r], lo_unscale, mainv[kb][r] * unscale);
    }
  }
  if (a.part_b && ct == 0) {
    float t = bsum;
    t += __shfl_xor(t, 32, 64);
    if (kg == 0 && rok) a.part_b[(long long)s * a.OUT + o0 + c32] = t * ps.unscale;
  }
  if (a.sat && satm > 65504.f) atomicAdd(a.sat, 1);
}

struct WreduceArgs {
  const float* part;
  float* out;
  long long n;       // elements of one slice
  const float* part2;   // second set of partial results reduced by the same launch (the bias gradient), or NULL
  float* out2;
  long long n2;
  int blocks1;       // workgroups of the first set
  int S, accumulate;
};

// column sums of the [S, n] partial results: a workgroup owns 64 columns, its four waves take every fourth slice
// (256-byte row segments, eight loads in flight), LDS adds the four in a fixed order.  Weight and bias partials go
// through one launch (the workgroups past blocks1 own the second set): the same sums in the same order as two
// launches, one launch gap less per dense layer of the backward pass.
__global__ __launch_bounds__(kWgBlock) void wgrad_reduce_kernel(const WreduceArgs a) {
  __shared__ float sm[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const bool second = (int)blockIdx.x >= a.blocks1;
  const float* part = second ? a.part2 : a.part;
  float* out = second ? a.out2 : a.out;
  const long long n = second ? a.n2 : a.n;
  const long long col = (long long)(second ? blockIdx.x - a.blocks1 : blockIdx.x) * 64 + c;
  float t = 0.f;
  if (col < n) {
    int s = g;
    for (; s + 28 < a.S; s += 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(long long)(s + 4 * u) * n + col];
#pragma unroll
      for (int u = 0; u < 8; ++u) t += v[u];
    }
    for (; s < a.S; s += 4) t += part[(long long)s * n + col];
  }
  sm[g][c] = t;
  __syncthreads();
  if (g == 0 && col < n) {
    const float r = ((sm[0][c] + sm[1][c]) + sm[2][c]) + sm[3][c];
    out[col] = a.accumulate ? out[col] + r : r;
  }
}

// Largest |value| of every row and of every column of a cotangent g [B, N], left on the device for the split-half
// kernels' pre-scale (split_half.hpp::pre_scale; no host read): the input gradient g W scales row b of g by its own
// power of two (row b of the result depends on no other row), the weight gradient g^T x column o (row o of dW depends
// on no other column) - so an entry is carried with full precision as long as it is within 2^29 of the largest one in
// ITS row / column, whatever the rest of the tensor holds.  One launch, one read of g: a workgroup owns a set of
// rows, folds |values| (as bit patterns: an unsigned orders like the value, a NaN above infinity) into LDS
// maxima per row and per column, writes its rows, stores its columns as scratch[1 + workgroup * N + c] and takes a
// ticket from scratch[0]; the last workgroup folds the stored columns, publishes them and puts the ticket word back
// to zero.  (Folding with one global atomic per workgroup and column cost 130 us a launch: the 128 words of a
// [B, 128] cotangent's columns lie in four cache lines, and atomics on one line are served one after the other.)
// Which rows: in the fast form (whole 16-byte packs, rows of at most 4096 columns) a workgroup takes passes of
// kAmaxLoads * RP rows, pass p = workgroup + trip * workgroups, so that at any moment the workgroups read one stretch
// of memory side by side (a contiguous block of rows each - 256 KB apart for [131 072, 128] - reached 0.6 TB/s; the
// later trips are run by tests/test_gpu_grad_range.py::test_abs_max_rows_and_columns); the plain forms keep a
// contiguous block.
constexpr int kAmaxThreads = 1024;
constexpr int kAmaxBlocks = 256;            // one per compute unit: 16 waves, four loads in flight per thread
constexpr int kAmaxCols = 8192;            // LDS words for the column maxima
constexpr int kAmaxRows = 4096;            // ... and for a workgroup's rows
constexpr int kAmaxLoads = 4;              // 16-byte loads in flight per thread
struct AmaxArgs {
  const float* x;
  long long B;
  int N, rows_per_block, nblocks, vec, fast, pass_rows;
  float* row_amax;
  float* col_amax;
  unsigned* scratch;
};
__global__ __launch_bounds__(kAmaxThreads) void abs_max_rows_cols_kernel(const AmaxArgs a) {
  __shared__ unsigned colm[kAmaxCols];
  __shared__ unsigned rowm[kAmaxRows];
  __shared__ int last;
  const int tid = threadIdx.x, N = a.N;
  const long long r0 = (long long)blockIdx.x * a.rows_per_block;
  const int rows = a.fast ? a.rows_per_block : (int)min((long long)a.rows_per_block, a.B - r0);
  for (int i = tid; i < N; i += kAmaxThreads) colm[i] = 0u;
  for (int i = tid; i < rows; i += kAmaxThreads) rowm[i] = 0u;
  __syncthreads();
  const float* xb = a.x + r0 * N;
  const int total = rows * N;                                  // <= kAmaxRows * kAmaxCols: fits an int
  bool rows_written = false;
  if (a.fast) {
    // N % 4 == 0, x 16-byte aligned, a row is at most one 16-byte pack per thread: thread = (pack column pc, row lane
    // rl) keeps its four columns' maxima in registers while it walks down the rows; a row's maximum is folded across
    // the PT lanes that share the row (PT <= 64: inside the wave, the row is written at once; else per wave into LDS)
    const int P = N / 4;
    int PT = 1;
    while (PT < P) PT <<= 1;
    const int pc = tid & (PT - 1), rl = tid / PT, RP = kAmaxThreads / PT;
    const int RPP = kAmaxLoads * RP;                           // rows of a pass
    const uint4* xv = reinterpret_cast<const uint4*>(a.x);
    unsigned c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
    rows_written = PT <= 64;
    for (int rb = 0; rb < rows; rb += RPP) {                   // (uniform trip count: every lane reaches the shuffles)
      const long long g0 = ((long long)(rb / RPP) * a.nblocks + blockIdx.x) * RPP;   // first row of this pass
      uint4 v[kAmaxLoads];
#pragma unroll
      for (int u = 0; u < kAmaxLoads; ++u) {
        const long long gr = g0 + u * RP + rl;
        v[u] = (pc < P && gr < a.B) ? xv[gr * P + pc] : uint4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int u = 0; u < kAmaxLoads; ++u) {
        const long long gr = g0 + u * RP + rl;
        const int r = rb + u * RP + rl;                        // place in this workgroup's LDS table
        const unsigned e0 = v[u].x & 0x7FFFFFFFu, e1 = v[u].y & 0x7FFFFFFFu, e2 = v[u].z & 0x7FFFFFFFu, e3 = v[u].w & 0x7FFFFFFFu;
        c0 = max(c0, e0); c1 = max(c1, e1); c2 = max(c2, e2); c3 = max(c3, e3);
        unsigned m = max(max(e0, e1), max(e2, e3));
        if (PT <= 64) {
          for (int o = PT >> 1; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
          if (pc == 0 && gr < a.B) a.row_amax[gr] = __builtin_bit_cast(float, m);
        } else {                                               // PT is a multiple of 64: a wave lies in one row
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
          if ((tid & 63) == 0 && gr < a.B) atomicMax(&rowm[r], m);
        }
      }
    }
    if (pc < P) {
      atomicMax(&colm[4 * pc], c0);
      atomicMax(&colm[4 * pc + 1], c1);
      atomicMax(&colm[4 * pc + 2], c2);
      atomicMax(&colm[4 * pc + 3], c3);
    }
  } else if (a.vec) {                                          // wider rows: flat walk, LDS maxima per pack
    const int nv = total / 4;
    for (int i = tid; i < nv; i += kAmaxLoads * kAmaxThreads) {
      uint4 v[kAmaxLoads];
#pragma unroll
      for (int u = 0; u < kAmaxLoads; ++u) {
        const int j = i + u * kAmaxThreads;
        v[u] = j < nv ? reinterpret_cast<const uint4*>(xb)[j] : uint4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int u = 0; u < kAmaxLoads; ++u) {
        const int j = i + u * kAmaxThreads;
        if (j < nv) {
          const int r = (4 * j) / N, c = 4 * j - r * N;
          const unsigned e0 = v[u].x & 0x7FFFFFFFu, e1 = v[u].y & 0x7FFFFFFFu, e2 = v[u].z & 0x7FFFFFFFu, e3 = v[u].w & 0x7FFFFFFFu;
          atomicMax(&rowm[r], max(max(e0, e1), max(e2, e3)));
          atomicMax(&colm[c], e0);
          atomicMax(&colm[c + 1], e1);
          atomicMax(&colm[c + 2], e2);
          atomicMax(&colm[c + 3], e3);
        }
      }
    }
  } else {
    for (int i = tid; i < total; i += kAmaxThreads) {
      const unsigned e = __builtin_bit_cast(unsigned, xb[i]) & 0x7FFFFFFFu;
      const int r = i / N;
      atomicMax(&rowm[r], e);
      atomicMax(&colm[i - r * N], e);
    }
  }
  __syncthreads();
  if (!rows_written)
    for (int i = tid; i < rows; i += kAmaxThreads) {
      long long gr = r0 + i;
      if (a.fast) gr = ((long long)(i / a.pass_rows) * a.nblocks + blockIdx.x) * a.pass_rows + i % a.pass_rows;
      if (gr < a.B) a.row_amax[gr] = __builtin_bit_cast(float, rowm[i]);
    }
  unsigned* part = a.scratch + 1 + (long long)blockIdx.x * N;
  for (int i = tid; i < N; i += kAmaxThreads) part[i] = colm[i];
  __threadfence();
  __syncthreads();
  if (tid == 0) last = atomicAdd(a.scratch, 1u) == (unsigned)(a.nblocks - 1);
  __syncthreads();
  if (last) {                                                  // every other workgroup's columns are in scratch by now
    __threadfence();
    const int stored = a.nblocks * N;                          // (fits an int: the launcher checks)
    // (eight requests in flight: this workgroup is alone on the device by now, one load at a time is all latency)
    for (int i0 = tid; i0 < stored; i0 += 8 * kAmaxThreads) {
      unsigned v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * kAmaxThreads;
        v[u] = i < stored ? __hip_atomic_load(a.scratch + 1 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * kAmaxThreads;
        if (i < stored && v[u] > colm[i % N]) atomicMax(&colm[i % N], v[u]);
      }
    }
    __syncthreads();
    for (int i = tid; i < N; i += kAmaxThreads) a.col_amax[i] = __builtin_bit_cast(float, colm[i]);
    if (tid == 0) atomicExch(a.scratch, 0u);
  }
}

template <int NB>
static void launch_wgrad(const WgradArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((linear_wgrad_kernel<NB>), dim3((unsigned)(a.row_tiles * a.S)), dim3(kWgBlock), 0, st, a);
}

}  // namespace vcnf

using namespace vcnf;

extern "C" int vcnf_linear_wgrad_supported(int32_t in_features, int32_t out_features) {
  return (in_features >= 16 && in_features <= 128 && in_features % 16 == 0 && out_features >= 1) ? 1 : 0;
}

/* batch slices the kernel uses: enough workgroups (row tiles x slices) for two waves on every SIMD, at least 256
 * samples per slice (the partial results are S x OUT x IN floats: 32 MB at 128 x 128) */
extern "C" int64_t vcnf_linear_wgrad_slices(int64_t batch, int32_t in_features, int32_t out_features) {
  if (!vcnf_linear_wgrad_supported(in_features, out_features) || batch < 1) return 0;
  const long long row_tiles = (out_features + 127) / 128;
  long long s = 512 / row_tiles;          // row tiles x slices <= 512 workgroups: two per CU, no third round for a few stragglers
  const long long most = (batch + 255) / 256;
  if (s > most) s = most;
  return s < 1 ? 1 : s;
}

/* rows a workgroup takes and the workgroups that makes: kAmaxBlocks of them while their rows fit the LDS table.
 * fast: the form for whole 16-byte packs (rows taken in passes of *pass_rows, interleaved over the workgroups) */
static long long amax_blocks(int64_t rows, int32_t cols, bool fast, long long* rows_per_block, int* pass_rows) {
  if (fast) {
    int pt = 1;
    while (pt < cols / 4) pt <<= 1;
    const long long rpp = (long long)kAmaxLoads * (kAmaxThreads / pt);
    const long long passes = (rows + rpp - 1) / rpp;
    long long blocks = passes < kAmaxBlocks ? passes : kAmaxBlocks;
    long long trips = (passes + blocks - 1) / blocks;
    if (trips * rpp > kAmaxRows) {
      trips = kAmaxRows / rpp;
      blocks = (passes + trips - 1) / trips;
    }
    *rows_per_block = trips * rpp;
    *pass_rows = (int)rpp;
    return blocks;
  }
  long long rpb = (rows + kAmaxBlocks - 1) / kAmaxBlocks;
  const long long fit = (long long)kAmaxRows * kAmaxCols / 4 / cols;      // rows * cols of a workgroup stays an int
  if (rpb > fit) rpb = fit;
  if (rpb > kAmaxRows) rpb = kAmaxRows;
  *rows_per_block = rpb;
  *pass_rows = 0;
  return (rows + rpb - 1) / rpb;
}
static bool amax_fast_shape(int32_t cols) { return cols % 4 == 0 && cols <= 4 * kAmaxThreads; }

extern "C" int64_t vcnf_abs_max_rows_cols_scratch_floats(int64_t rows, int32_t cols) {
  long long rpb;
  int pr;
  if (rows < 1 || cols < 1 || cols > kAmaxCols) return 0;
  long long blocks = amax_blocks(rows, cols, false, &rpb, &pr);          // (which form runs depends on x's alignment too)
  if (amax_fast_shape(cols)) {
    const long long other = amax_blocks(rows, cols, true, &rpb, &pr);
    if (other > blocks) blocks = other;
  }
  return 1 + blocks * cols;
}

extern "C" int vcnf_abs_max_rows_cols_f32(const float* x, int64_t rows, int32_t cols, float* row_amax, float* col_amax,
                                          float* scratch, int64_t scratch_floats, void* stream) {
  if (!x || !row_amax || !col_amax || !scratch) return VCNF_ERR_NULL;
  if (rows < 1 || cols < 1) return VCNF_ERR_SHAPE;
  if (cols > kAmaxCols) return VCNF_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(x) & 3) return VCNF_ERR_ALIGN;
  AmaxArgs a;
  a.x = x; a.B = rows; a.N = cols; a.row_amax = row_amax; a.col_amax = col_amax;
  a.scratch = reinterpret_cast<unsigned*>(scratch);
  long long rpb;
  a.vec = (cols % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) ? 1 : 0;
  a.fast = (a.vec && amax_fast_shape(cols)) ? 1 : 0;
  const long long blocks = amax_blocks(rows, cols, a.fast != 0, &rpb, &a.pass_rows);
  if (blocks * cols > 0x7FFFFFFF) return VCNF_ERR_UNSUPPORTED;           // (the last workgroup indexes the stored columns with an int)
  if (scratch_floats < 1 + blocks * cols) return VCNF_ERR_SHAPE;
  a.rows_per_block = (int)rpb;
  a.nblocks = (int)blocks;
  hipLaunchKernelGGL(abs_max_rows_cols_kernel, dim3((unsigned)blocks), dim3(kAmaxThreads), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? VCNF_OK : VCNF_ERR_LAUNCH;
}

static int wgrad_run(const float* x, const float* dy, float* dw, float* db, float* workspace, int64_t workspace_floats,
                     int64_t batch, int32_t in_features, int32_t out_features, int accumulate, int f16x3,
                     const float* dy_amax, int32_t* sat_count, void* stream);

extern "C" int vcnf_linear_wgrad_f32(const float* x, const float* dy, float* dw, float* db, float* workspace,
                                     int64_t workspace_floats, int64_t batch, int32_t in_features,
                                     int32_t out_features, int accumulate, void* stream) {
  return wgrad_run(x, dy, dw, db, workspace, workspace_floats, batch, in_features, out_features, accumulate, 0, nullptr, nullptr, stream);
}

extern "C" int vcnf_linear_wgrad_f16x3_f32(const float* x, const float* dy, float* dw, float* db, float* workspace,
                                           int64_t workspace_floats, int64_t batch, int32_t in_features,
                                           int32_t out_features, int accumulate, int relu_input,
                                           const float* dy_amax, int32_t* sat_count, void* stream) {
  return wgrad_run(x, dy, dw, db, workspace, workspace_floats, batch, in_features, out_features, accumulate,
                   relu_input ? 2 : 1, dy_amax, sat_count, stream);
}

static int wgrad_run(const float* x, const float* dy, float* dw, float* db, float* workspace, int64_t workspace_floats,
                     int64_t batch, int32_t in_features, int32_t out_features, int accumulate, int f16x3,
                     const float* dy_amax, int32_t* sat_count, void* stream) {
  if (!vcnf_linear_wgrad_supported(in_features, out_features)) return VCNF_ERR_UNSUPPORTED;
  if (batch < 1) return VCNF_ERR_SHAPE;
  if (!x || !dy || !dw || !workspace) return VCNF_ERR_NULL;
  const long long S = vcnf_linear_wgrad_slices(batch, in_features, out_features);
  const long long per = (long long)out_features * in_features + (db ? out_features : 0);
  if (workspace_floats < S * per) return VCNF_ERR_SHAPE;
  WgradArgs a;
  a.sat = sat_count;
  a.amax = dy_amax;
  a.col_tiles = 1;
  a.relu_x = f16x3 == 2 ? 1 : 0;              // f16x3: 0 exact fp32 kernel, 1 split-half, 2 split-half on relu(x)
  a.x = x; a.dy = dy; a.part_w = workspace;
  a.part_b = db ? workspace + S * (long long)out_features * in_features : nullptr;
  a.B = batch; a.IN = in_features; a.OUT = out_features; a.S = (int)S;
  a.row_tiles = (out_features + 127) / 128;
  a.chunk = ((batch + S - 1) / S + 15) / 16 * 16;
  hipStream_t st = (hipStream_t)stream;
  // (the split-half kernel addresses its operands through 32-bit buffer descriptors)
  if (f16x3 && ((long long)batch * out_features * 4 >= (1ll << 31) || (long long)batch * in_features * 4 >= (1ll << 31))) {
    if (f16x3 == 2) return VCNF_ERR_UNSUPPORTED;     // (the exact-fp32 kernel has no ReLU on load: the caller materialises relu(x))
    f16x3 = 0;
  }
  if (f16x3) {
    a.col_tiles = (in_features + 63) / 64;
    const dim3 grid((unsigned)(a.col_tiles * a.row_tiles * a.S));
    if (in_features <= 32) hipLaunchKernelGGL((linear_wgrad_f16x3_kernel<1>), grid, dim3(kWgBlock), 0, st, a);
    else hipLaunchKernelGGL((linear_wgrad_f16x3_kernel<2>), grid, dim3(kWgBlock), 0, st, a);
  } else
  switch (in_features / 16) {
    case 1: launch_wgrad<1>(a, st); break;
    case 2: launch_wgrad<2>(a, st); break;
    case 3: launch_wgrad<3>(a, st); break;
    case 4: launch_wgrad<4>(a, st); break;
    case 5: launch_wgrad<5>(a, st); break;
    case 6: launch_wgrad<6>(a, st); break;
    case 7: launch_wgrad<7>(a, st); break;
    case 8: launch_wgrad<8>(a, st); break;
    default: return VCNF_ERR_UNSUPPORTED;
  }
  WreduceArgs r;
  r.part = a.part_w; r.out = dw; r.n = (long long)out_features * in_features; r.S = (int)S; r.accumulate = accumulate ? 1 : 0;
  r.blocks1 = (int)((r.n + 63) / 64);
  r.part2 = db ? a.part_b : nullptr; r.out2 = db; r.n2 = db ? out_features : 0;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(r.blocks1 + (r.n2 + 63) / 64)), dim3(kWgBlock), 0, st, r);
  return hipGetLastError() == hipSuccess ? VCNF_OK : VCNF_ERR_LAUNCH;
}
