// Full-covariance base distributions for MI355X (gfx950, wave64): the multivariate Gaussian and the multivariate
// Student-t over D <= 128 features.  With L lower triangular, M = L^-1, x = z - loc, y = M x, q = |y|^2 and
// consts = (cst, nu) on the device (cst holds the normaliser and -sum log diag L):
//   log p = cst + f(q),   Gaussian f = -q / 2,   Student-t f = -(nu + D) / 2 log1p(q / nu)
//   sample: z = loc + s L eps, s = 1 or sqrt(nu / (2 gamma)); its density uses q = s^2 |eps|^2, no solve
// The caller inverts L and evaluates cst (both of size [D, D] or smaller): no kernel solves or calls lgamma.
//
// A workgroup stages the triangular operand in LDS once (packed 4 x 4 blocks of the lower triangle, mvn_lds.hpp; the
// upper triangle of the caller's matrix is never read) and streams tiles of 64 (fp64: 32) samples past it.  A tile is
// read from memory once, coalesced, in packs of up to 16 bytes, into LDS rows; thread (sample s, part p) then forms
// the block rows p, p + parts, ... of the triangular product for its sample: four entries of the operand row (one
// read, the same address across the lanes of a part) against four of the sample, D (D + 1) / 2 multiply-adds per
// sample up to the diagonal blocks' padding.  log_prob adds y_i^2 as they appear and keeps no y.  Sums over a sample
// go through LDS - over a thread's block rows in ascending order, then over the parts in ascending order - and sums
// over samples walk the tile in order from LDS, tile after tile of the workgroup's range: no lane butterfly of
// stream_common.hpp and no atomic is used anywhere, the same call twice gives the same bits.  All arithmetic is
// on the vector units in the working precision, except the sums over samples of the VJPs (Acc below).
//
// The VJPs sum two outer products, tril(sum_b c_b y_b y_b^T) and d_tri = tril(sum_b s_b g_z_b eps_b^T),
// with one device function: a thread owns up to three 4 x 4 blocks of the lower triangle in registers and walks the
// tile's samples in order.  Workgroup k of vcnf_mvn_bwd_groups(batch, D) takes the tiles k, k + groups, ... and writes
// one block [D D + D + 1] (the square with zeros above the diagonal | d_loc | d_nu); reduce_partials adds the blocks
// in a fixed order.
#include "mvn_lds.hpp"
#include "stream_common.hpp"

namespace vcnf_mvn {

using namespace vcnf_stream;

constexpr int kMaxFwdBlocks = 512;
constexpr long long kMaxWorkspace = 1LL << 22;          // elements of the VJPs' partial blocks (vcnf_hip.h)
constexpr long long kMaxGroups = 256;

template <typename T>
struct Args {
  const T *x, *gamma, *loc, *tri, *consts;     // x: z, or eps when sampling
  const T *g, *gz;                             // VJPs: cotangent of logp (or NULL = 0), gz_in / g_z (or NULL = 0)
  T *out, *logp, *dgamma, *partials;           // out: z | dz | deps
  long long B;
  int D, family, ld_mode;
  T sign;
};

// ------------------------------------------------------------------ the two families
template <typename T>
__device__ __forceinline__ T density(int family, T q, T nu, int D) {
  return family == VCNF_MVN_STUDENT_T ? T(-0.5) * (nu + T(D)) * log1p_(q / nu) : T(-0.5) * q;
}

// fq = df/dq, fnu = df/dnu at fixed q
template <typename T>
__device__ __forceinline__ void density_grad(int family, T q, T nu, int D, T& fq, T& fnu) {
  if (family == VCNF_MVN_STUDENT_T) {
    const T nd = nu + T(D), den = nu + q;
    fq = -nd / (T(2) * den);
    fnu = T(-0.5) * log1p_(q / nu) + nd * q / (T(2) * nu * den);
  } else {
    fq = T(-0.5);
    fnu = T(0);
  }
}

// ------------------------------------------------------------------ staging
// the lower triangle of tri [D, D] into its packed blocks, zeros in the blocks' padding
template <typename T>
__device__ __forceinline__ void stage_tri(const T* __restrict__ tri, T* lds, int D) {
  const int Dp = padded(D);
  for (int e = threadIdx.x; e < Dp * Dp; e += kBlock) {
    const int i = e / Dp, j = e - i * Dp;
    if (j < 4 * (i / 4 + 1)) lds[tri_row(i) + j] = (i < D && j <= i) ? tri[(long long)i * D + j] : T(0);
  }
}

// rows [0, n) of src [n, D] minus sub [D] (or as they are) into the tile; zeros in the padding columns and the rows
// [n, tile_rows)
template <typename T, int V>
__device__ __forceinline__ void load_tile(const T* __restrict__ src, int n, int D, T* dst, int stride, const T* sub) {
  using PackT = Pack<T, V>;
  constexpr int TS = tile_rows<T>();
  const int Dp = padded(D), npk = n * D / V;
  for (int k = threadIdx.x; k < npk; k += kBlock) {
    PackT v = reinterpret_cast<const PackT*>(src)[k];
    const int e = k * V, r = e / D, j = e - r * D;
    if (sub) {
#pragma unroll
      for (int u = 0; u < V; ++u) v.v[u] -= sub[j + u];
    }
    *reinterpret_cast<PackT*>(dst + r * stride + j) = v;
  }
  if (Dp != D) {
    const int w = Dp - D;
    for (int k = threadIdx.x; k < TS * w; k += kBlock) dst[(k / w) * stride + D + k % w] = T(0);
  }
  if (n < TS)
    for (int k = threadIdx.x; k < (TS - n) * Dp; k += kBlock) dst[(n + k / Dp) * stride + k % Dp] = T(0);
}

template <typename T>
__device__ __forceinline__ void zero_tile(T* dst, int D, int stride) {
  const int Dp = padded(D);
  for (int k = threadIdx.x; k < tile_rows<T>() * Dp; k += kBlock) dst[(k / Dp) * stride + k % Dp] = T(0);
}

// dst [n, D] = add (or 0) + scale[r] * tile + shift (or 0), coalesced
template <typename T, int V>
__device__ __forceinline__ void store_tile(T* __restrict__ dst, int n, int D, const T* tile, int stride, const T* scale,
                                           const T* shift, const T* __restrict__ add) {
  using PackT = Pack<T, V>;
  const int npk = n * D / V;
  for (int k = threadIdx.x; k < npk; k += kBlock) {
    const int e = k * V, r = e / D, j = e - r * D;
    PackT v = *reinterpret_cast<const PackT*>(tile + r * stride + j);
    const T sc = scale ? scale[r] : T(1);
    PackT o;
    if (add) {
      o = reinterpret_cast<const PackT*>(add)[k];
    } else {
#pragma unroll
      for (int u = 0; u < V; ++u) o.v[u] = T(0);
    }
#pragma unroll
    for (int u = 0; u < V; ++u) o.v[u] += sc * v.v[u] + (shift ? shift[j + u] : T(0));
    reinterpret_cast<PackT*>(dst)[k] = o;
  }
}

// ------------------------------------------------------------------ the triangular products of one sample
// out[r] = sum_{j <= 4I + r} tri[4I + r][j] x[j]
template <typename T>
__device__ __forceinline__ void lower_block(const T* tri, const T* x, int I, T (&out)[4]) {
  using P4 = Pack<T, 4>;
  const int len = 4 * (I + 1);
  const T* m = tri + 8 * I * (I + 1);
#pragma unroll
  for (int r = 0; r < 4; ++r) out[r] = T(0);
  for (int J = 0; J <= I; ++J) {
    const P4 xv = *reinterpret_cast<const P4*>(x + 4 * J);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const P4 mv = *reinterpret_cast<const P4*>(m + r * len + 4 * J);
#pragma unroll
      for (int c = 0; c < 4; ++c) out[r] += mv.v[c] * xv.v[c];
    }
  }
}

// out[c] = sum_{i >= 4J + c} tri[i][4J + c] y[i]: the transposed product
template <typename T>
__device__ __forceinline__ void upper_block(const T* tri, const T* y, int J, int nb, T (&out)[4]) {
  using P4 = Pack<T, 4>;
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c] = T(0);
  for (int I = J; I < nb; ++I) {
    const int len = 4 * (I + 1);
    const T* m = tri + 8 * I * (I + 1) + 4 * J;
    const P4 yv = *reinterpret_cast<const P4*>(y + 4 * I);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const P4 mv = *reinterpret_cast<const P4*>(m + r * len);
#pragma unroll
      for (int c = 0; c < 4; ++c) out[c] += mv.v[c] * yv.v[r];
    }
  }
}

// the 4 x 4 blocks (I, J), J <= I, of the lower triangle a thread owns: t, t + kBlock, ... in row-major block order
struct Owned {
  int I[kMaxBlocksOwned], J[kMaxBlocksOwned];      // I < 0: none
};

__device__ __forceinline__ Owned owned_blocks(int nb) {
  Owned o;
#pragma unroll
  for (int k = 0; k < kMaxBlocksOwned; ++k) {
    const int blk = threadIdx.x + k * kBlock;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= blk) ++I;
    o.I[k] = blk < nb * (nb + 1) / 2 ? I : -1;
    o.J[k] = blk - I * (I + 1) / 2;
  }
  return o;
}

// Sums over samples are kept in fp64 registers in both precisions, the one place where the fp32 kernels leave their
// working precision: exact products, one rounding per workgroup.  For the same reason the density's VJP sums
// Y = c y y^T and not the gradient of M, G = c y x^T = Y L^T: the gradient of L is -tril(M^T Y), while the way there
// from G, -M^T G M^T, undoes the factor L^T and multiplies every rounding of G - the partial blocks', the reduction's -
// by cond(L).  Measured on the gradient of `lower` at D = 128, B = 1000 against the fp32 torch composition's own error
// (99.9th percentile): G with fp32 sums 2.7 x, with fp64 sums 2.4 x (profiles/mvn_base.md).
using Acc = double;

// acc(I, J) += sum over the tile's samples s, in order, of w[s] rows[s][4I ..] cols[s][4J ..]^T
template <typename T>
__device__ __forceinline__ void outer_product_sum(const Owned& o, const T* w, const T* rows, const T* cols, int stride,
                                                  Acc (&acc)[kMaxBlocksOwned][4][4]) {
  using P4 = Pack<T, 4>;
  for (int s = 0; s < tile_rows<T>(); ++s) {
    const T ws = w[s];
#pragma unroll
    for (int k = 0; k < kMaxBlocksOwned; ++k) {
      if (o.I[k] < 0) continue;
      const P4 rv = *reinterpret_cast<const P4*>(rows + s * stride + 4 * o.I[k]);
      const P4 cv = *reinterpret_cast<const P4*>(cols + s * stride + 4 * o.J[k]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const Acc wr = (Acc)ws * (Acc)rv.v[r];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[k][r][c] += wr * (Acc)cv.v[c];
      }
    }
  }
}

extern __shared__ __align__(32) unsigned char mvn_lds[];

// ------------------------------------------------------------------ log_prob / sample
template <typename T, int V, bool SAMPLE>
__global__ __launch_bounds__(kBlock) void mvn_fwd_kernel(const Args<T> a) {
  using P4 = Pack<T, 4>;
  constexpr int TS = tile_rows<T>(), PARTS = kBlock / TS;
  const int D = a.D, nb = block_rows(D), stride = row_stride(D);
  const Layout l = layout<T>(D, SAMPLE);
  T* lds = reinterpret_cast<T*>(mvn_lds);
  T *tri = lds + l.TRI, *loc = lds + l.LOC, *A = lds + l.A, *Bt = lds + l.B, *Q = lds + l.Q, *S = lds + l.S;
  const int t = threadIdx.x, s = t % TS, p = t / TS;
  stage_tri(a.tri, tri, D);
  for (int j = t; j < padded(D); j += kBlock) loc[j] = j < D ? a.loc[j] : T(0);
  const T cst = a.consts[0], nu = a.consts[1];
  const long long tiles = (a.B + TS - 1) / TS;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long b0 = tile * TS;
    const int n = a.B - b0 < TS ? (int)(a.B - b0) : TS;
    __syncthreads();               // the operand is staged / the tile before is read
    load_tile<T, V>(a.x + b0 * D, n, D, A, stride, SAMPLE ? nullptr : loc);
    __syncthreads();
    const T* row = A + s * stride;
    T part = T(0);
    for (int I = p; I < nb; I += PARTS) {
      T y[4];
      lower_block(tri, row, I, y);
      if (SAMPLE) {
        const P4 ev = *reinterpret_cast<const P4*>(row + 4 * I);
        P4 yv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          part += ev.v[r] * ev.v[r];
          yv.v[r] = y[r];
        }
        *reinterpret_cast<P4*>(Bt + s * stride + 4 * I) = yv;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) part += y[r] * y[r];
      }
    }
    Q[p * TS + s] = part;
    __syncthreads();
    if (t < TS) {
      T q = Q[t];
      for (int k = 1; k < PARTS; ++k) q += Q[k * TS + t];
      T sc = T(1);
      if (SAMPLE && a.family == VCNF_MVN_STUDENT_T && t < n) sc = sqrt_(nu / (T(2) * a.gamma[b0 + t]));
      q = sc * sc * q;
      S[t] = sc;
      if (t < n) put_ld(a.logp, b0 + t, a.sign * (cst + density(a.family, q, nu, D)), a.ld_mode);
    }
    if (SAMPLE) {
      __syncthreads();
      store_tile<T, V>(a.out + b0 * D, n, D, Bt, stride, S, loc, nullptr);
    }
  }
}

// ------------------------------------------------------------------ the VJPs
// OP 0, log_prob: x = z,   g = cotangent of logp, gz = gz_in (or NULL);                 out = dz
// OP 1, sample:   x = eps, g = g_lp (or NULL),    gz = g_z (or NULL), gamma, dgamma;    out = deps (or NULL)
template <typename T, int V, int OP>
__global__ __launch_bounds__(kBlock) void mvn_bwd_kernel(const Args<T> a) {
  using P4 = Pack<T, 4>;
  constexpr int TS = tile_rows<T>(), PARTS = kBlock / TS;
  const int D = a.D, Dp = padded(D), nb = block_rows(D), stride = row_stride(D);
  const Layout l = layout<T>(D, true);
  T* lds = reinterpret_cast<T*>(mvn_lds);
  T *tri = lds + l.TRI, *loc = lds + l.LOC, *A = lds + l.A, *Bt = lds + l.B, *Q = lds + l.Q, *S = lds + l.S;
  const int t = threadIdx.x, s = t % TS, p = t / TS;
  const bool student = a.family == VCNF_MVN_STUDENT_T, sums = a.partials != nullptr;
  stage_tri(a.tri, tri, D);
  if (OP == 0)
    for (int j = t; j < Dp; j += kBlock) loc[j] = j < D ? a.loc[j] : T(0);
  const T nu = a.consts[1];
  const Owned own = owned_blocks(nb);
  Acc acc[kMaxBlocksOwned][4][4];
#pragma unroll
  for (int k = 0; k < kMaxBlocksOwned; ++k)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[k][r][c] = 0;
  Acc sum_loc = 0, sum_nu = 0;                   // thread j < Dp: column j of d_loc; thread 0: d_nu

  const long long tiles = (a.B + TS - 1) / TS;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long b0 = tile * TS;
    const int n = a.B - b0 < TS ? (int)(a.B - b0) : TS;
    __syncthreads();
    load_tile<T, V>(a.x + b0 * D, n, D, A, stride, OP == 0 ? loc : nullptr);
    if (OP == 1) {
      if (a.gz)
        load_tile<T, V>(a.gz + b0 * D, n, D, Bt, stride, nullptr);
      else
        zero_tile(Bt, D, stride);
    }
    __syncthreads();
    // a sample's q: y = tri x into the second tile (log_prob), or |eps|^2 (sample)
    T* rowA = A + s * stride;
    T* rowB = Bt + s * stride;
    T part = T(0);
    for (int I = p; I < nb; I += PARTS) {
      P4 yv;
      if (OP == 0) {
        T y[4];
        lower_block(tri, rowA, I, y);
#pragma unroll
        for (int r = 0; r < 4; ++r) yv.v[r] = y[r];
        *reinterpret_cast<P4*>(rowB + 4 * I) = yv;
      } else {
        yv = *reinterpret_cast<const P4*>(rowA + 4 * I);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) part += yv.v[r] * yv.v[r];
    }
    Q[p * TS + s] = part;
    __syncthreads();
    // per-sample scalars, kept by thread t < TS for its sample t.  S[0]: the weight of the outer product (c or s),
    // S[1]: log_prob - g df/dnu; sample - the factor of eps in deps, S[2]: sample - the sample's term of d_nu
    T e2 = T(0), sc = T(1), k2 = T(0), gm = T(1), gfnu = T(0);
    if (t < TS) {
      e2 = Q[t];
      for (int k = 1; k < PARTS; ++k) e2 += Q[k * TS + t];
      const bool live = t < n;
      const T g = live && a.g ? a.g[b0 + t] : T(0);
      T fq, fnu;
      if (OP == 0) {
        density_grad(a.family, e2, nu, D, fq, fnu);
        S[t] = T(2) * g * fq;
        S[TS + t] = g * fnu;
      } else {
        if (student && live) {
          gm = a.gamma[b0 + t];
          sc = sqrt_(nu / (T(2) * gm));
        }
        density_grad(a.family, sc * sc * e2, nu, D, fq, fnu);
        k2 = T(2) * g * fq;
        gfnu = g * fnu;
        S[t] = sc;
        S[TS + t] = k2 * sc * sc;
      }
    }
    __syncthreads();
    if (sums) {
      outer_product_sum(own, S, Bt, OP == 0 ? Bt : A, stride, acc);      // c y y^T | s g_z eps^T
      if (OP == 1 && t < Dp)
        for (int r = 0; r < TS; ++r) sum_loc += (Acc)Bt[r * stride + t];
    }
    __syncthreads();
    // the transposed product of the second tile's rows, into the first tile
    part = T(0);
    for (int J = p; J < nb; J += PARTS) {
      T w[4];
      upper_block(tri, rowB, J, nb, w);
      P4 o;
      if (OP == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) o.v[c] = w[c];
      } else {
        const P4 ev = *reinterpret_cast<const P4*>(rowA + 4 * J);
        const T ss = S[s], ke = S[TS + s];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          part += w[c] * ev.v[c];
          o.v[c] = ss * w[c] + ke * ev.v[c];
        }
      }
      *reinterpret_cast<P4*>(rowA + 4 * J) = o;
    }
    if (OP == 1) Q[p * TS + s] = part;
    __syncthreads();
    if (OP == 0) {
      // dz = gz_in + c tri^T y;  d_loc = -sum c tri^T y;  d_nu = sum g df/dnu
      store_tile<T, V>(a.out + b0 * D, n, D, A, stride, S, nullptr, a.gz ? a.gz + b0 * D : nullptr);
      if (sums && t < Dp)
        for (int r = 0; r < TS; ++r) sum_loc -= (Acc)S[r] * (Acc)A[r * stride + t];
      if (sums && t == 0)
        for (int r = 0; r < TS; ++r) sum_nu += (Acc)S[TS + r];
    } else {
      if (a.out) store_tile<T, V>(a.out + b0 * D, n, D, A, stride, nullptr, nullptr, nullptr);
      if (t < TS) {
        T wdot = Q[t];
        for (int k = 1; k < PARTS; ++k) wdot += Q[k * TS + t];
        const T ds = wdot + k2 * sc * e2;
        if (student && t < n) a.dgamma[b0 + t] = -ds * sc / (T(2) * gm);
        S[2 * TS + t] = student ? ds * sc / (T(2) * nu) + gfnu : T(0);
      }
      if (sums) {
        __syncthreads();
        if (t == 0)
          for (int r = 0; r < TS; ++r) sum_nu += (Acc)S[2 * TS + r];
      }
    }
  }
  if (!sums) return;
  // the workgroup's block: the owned 4 x 4 blocks through the packed triangle in LDS, then the square row by row
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kMaxBlocksOwned; ++k) {
    if (own.I[k] < 0) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      P4 v;
#pragma unroll
      for (int c = 0; c < 4; ++c) v.v[c] = (T)acc[k][r][c];
      *reinterpret_cast<P4*>(tri + tri_row(4 * own.I[k] + r) + 4 * own.J[k]) = v;
    }
  }
  __syncthreads();
  T* block = a.partials + (long long)blockIdx.x * ((long long)D * D + D + 1);
  for (int e = t; e < D * D; e += kBlock) {
    const int i = e / D, j = e - i * D;
    block[e] = j <= i ? tri[tri_row(i) + j] : T(0);
  }
  if (t < D) block[D * D + t] = (T)sum_loc;
  if (t == 0) block[D * D + D] = (T)sum_nu;
}

// element e of the summed block goes to d_tri [D, D] | d_loc [D] | d_nu [1]
template <typename T>
struct BlockDest {
  T *d_tri, *d_loc, *d_nu;
  long long DD, D;
  __device__ T* operator()(long long e) const { return e < DD ? d_tri + e : e < DD + D ? d_loc + (e - DD) : d_nu; }
};

// ------------------------------------------------------------------ host side
static inline bool ok_family(int f) { return f == VCNF_MVN_GAUSSIAN || f == VCNF_MVN_STUDENT_T; }

static int check_shape(int64_t batch, int32_t D) { return batch < 0 || D < 1 || D > kMaxD ? VCNF_ERR_SHAPE : VCNF_OK; }

// workgroups of a VJP = partial blocks: one per 64 samples, at most kMaxGroups and at most kMaxWorkspace elements
static long long bwd_groups(int64_t batch, int32_t D) {
  const long long block = (long long)D * D + D + 1;
  long long cap = kMaxWorkspace / block;
  cap = cap > kMaxGroups ? kMaxGroups : cap;
  const long long n = (batch + 63) / 64;
  return n < 1 ? 1 : n > cap ? cap : n;
}

// MAX: the largest byte count of the kernel instance (its limit is raised once, to that)
template <auto Kernel, typename T>
static int launch(dim3 grid, size_t lds, size_t max_lds, const Args<T>& a, hipStream_t st) {
  if (lds > kLdsNoAttribute && !vcnf::lds_limit_once<Kernel>(max_lds)) return VCNF_ERR_LAUNCH;
  hipLaunchKernelGGL(Kernel, grid, dim3(kBlock), lds, st, a);
  return launched();
}

template <typename T>
static int forward(const T* in, const T* gamma, const T* loc, const T* tri, const T* consts, T* z, T* logp, int64_t batch,
                   int32_t D, int family, int ld_mode, T sign, bool sample, void* stream) {
  if (const int st = check_shape(batch, D)) return st;
  if (!ok_family(family) || !ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!in || !loc || !tri || !consts || !logp || (sample && (!z || (family == VCNF_MVN_STUDENT_T && !gamma)))) return VCNF_ERR_NULL;
  if (!all_aligned({in, gamma, loc, tri, consts, z, logp}, sizeof(T))) return VCNF_ERR_ALIGN;
  Args<T> a{in, gamma, loc, tri, consts, nullptr, nullptr, z, logp, nullptr, nullptr, batch, D, family, ld_mode, sign};
  constexpr int TS = tile_rows<T>();
  long long tiles = (batch + TS - 1) / TS;
  const dim3 grid((unsigned)(tiles > kMaxFwdBlocks ? kMaxFwdBlocks : tiles));
  return with_pack<T>(D, {in, z}, [&](auto V) {
    return with_flags([&](auto SAMPLE) {
      return launch<mvn_fwd_kernel<T, V(), SAMPLE()>>(grid, bytes<T>(D, SAMPLE()), bytes<T>(kMaxD, SAMPLE()), a,
                                                      (hipStream_t)stream);
    }, sample);
  });
}

template <typename T, int OP>
static int backward(Args<T> a, std::initializer_list<const void*> streamed, hipStream_t st) {
  const dim3 grid((unsigned)bwd_groups(a.B, a.D));
  return with_pack<T>(a.D, streamed, [&](auto V) {
    return launch<mvn_bwd_kernel<T, V(), OP>>(grid, bytes<T>(a.D, true), bytes<T>(kMaxD, true), a, st);
  });
}

template <typename T>
static int log_prob_bwd(const T* z, const T* loc, const T* tri, const T* consts, const T* g, const T* gz_in, T* dz, T* partials,
                        int64_t batch, int32_t D, int family, void* stream) {
  if (const int st = check_shape(batch, D)) return st;
  if (!ok_family(family)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!z || !loc || !tri || !consts || !g || !dz) return VCNF_ERR_NULL;
  if (!all_aligned({z, loc, tri, consts, g, gz_in, dz, partials}, sizeof(T))) return VCNF_ERR_ALIGN;
  const Args<T> a{z, nullptr, loc, tri, consts, g, gz_in, dz, nullptr, nullptr, partials, batch, D, family, VCNF_LD_STORE, T(1)};
  return backward<T, 0>(a, {z, gz_in, dz}, (hipStream_t)stream);
}

template <typename T>
static int sample_bwd(const T* eps, const T* gamma, const T* tri, const T* consts, const T* g_z, const T* g_lp, T* deps,
                      T* dgamma, T* partials, int64_t batch, int32_t D, int family, void* stream) {
  if (const int st = check_shape(batch, D)) return st;
  if (!ok_family(family)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!eps || !tri || !consts || (family == VCNF_MVN_STUDENT_T && (!gamma || !dgamma))) return VCNF_ERR_NULL;
  if (!all_aligned({eps, gamma, tri, consts, g_z, g_lp, deps, dgamma, partials}, sizeof(T))) return VCNF_ERR_ALIGN;
  const Args<T> a{eps, gamma, nullptr, tri, consts, g_lp, g_z, deps, nullptr, dgamma, partials, batch, D, family, VCNF_LD_STORE, T(1)};
  return backward<T, 1>(a, {eps, g_z, deps}, (hipStream_t)stream);
}

template <typename T>
static int reduce_partials(const T* partials, int64_t groups, int32_t D, T* d_loc, T* d_tri, T* d_nu, void* stream) {
  if (groups < 1 || D < 1 || D > kMaxD) return VCNF_ERR_SHAPE;
  if (!partials || !d_loc || !d_tri || !d_nu) return VCNF_ERR_NULL;
  if (!all_aligned({partials, d_loc, d_tri, d_nu}, sizeof(T))) return VCNF_ERR_ALIGN;
  const long long DD = (long long)D * D;
  return launch_reduce_partials(partials, groups, DD + D + 1, BlockDest<T>{d_tri, d_loc, d_nu, DD, D}, stream);
}

}  // namespace vcnf_mvn

using namespace vcnf_mvn;

extern "C" int64_t vcnf_mvn_bwd_groups(int64_t batch, int32_t features) {
  if (check_shape(batch, features) != VCNF_OK) return 0;
  return bwd_groups(batch, features);
}

#define VCNF_MVN_ENTRY_POINTS(T, SFX)                                                                                  \
  extern "C" int vcnf_mvn_log_prob_##SFX(const T* z, const T* loc, const T* tri_inv, const T* consts, T* logp,         \
                                         int64_t batch, int32_t features, int family, int ld_mode, T sign,             \
                                         void* stream) {                                                               \
    return forward<T>(z, nullptr, loc, tri_inv, consts, nullptr, logp, batch, features, family, ld_mode, sign, false,  \
                      stream);                                                                                         \
  }                                                                                                                    \
  extern "C" int vcnf_mvn_sample_##SFX(const T* eps, const T* gamma, const T* loc, const T* tri, const T* consts,      \
                                       T* z, T* logp, int64_t batch, int32_t features, int family, void* stream) {     \
    return forward<T>(eps, gamma, loc, tri, consts, z, logp, batch, features, family, VCNF_LD_STORE, T(1), true,       \
                      stream);                                                                                         \
  }                                                                                                                    \
  extern "C" int vcnf_mvn_log_prob_bwd_##SFX(const T* z, const T* loc, const T* tri_inv, const T* consts, const T* g,  \
                                             const T* gz_in, T* dz, T* partials, int64_t batch, int32_t features,      \
                                             int family, void* stream) {                                               \
    return log_prob_bwd<T>(z, loc, tri_inv, consts, g, gz_in, dz, partials, batch, features, family, stream);          \
  }                                                                                                                    \
  extern "C" int vcnf_mvn_sample_bwd_##SFX(const T* eps, const T* gamma, const T* tri, const T* consts,                \
                                           const T* g_z, const T* g_lp, T* deps, T* dgamma, T* partials,               \
                                           int64_t batch, int32_t features, int family, void* stream) {                \
    return sample_bwd<T>(eps, gamma, tri, consts, g_z, g_lp, deps, dgamma, partials, batch, features, family, stream); \
  }                                                                                                                    \
  extern "C" int vcnf_mvn_reduce_partials_##SFX(const T* partials, int64_t groups, int32_t features, T* d_loc,         \
                                                T* d_tri, T* d_nu, void* stream) {                                     \
    return reduce_partials<T>(partials, groups, features, d_loc, d_tri, d_nu, stream);                                 \
  }

VCNF_MVN_ENTRY_POINTS(float, f32)
VCNF_MVN_ENTRY_POINTS(double, f64)
