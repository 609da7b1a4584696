// Heavy-tailed product base distributions for MI355X (gfx950, wave64): Student-t and the generalised Gaussian, one
// tail parameter per feature.  With u = (z - loc) / exp(log_scale) and the rows shape (nu or beta) and cst [D]:
//   logp[b] = sum_d (cst[d] - log_scale[d] + f(u; shape[d]))
//   Student-t             f = -(nu + 1) / 2 log1p(u^2 / nu)
//   generalised Gaussian  f = -|u|^beta,  |u|^beta = exp(beta log|u|) and 0 at u == 0
// cst is the row of normalisers; the caller computes it (and everything else of size [D]), so no kernel evaluates a
// special function, and the random draws of sampling are the caller's too: the sample kernel maps (eps, gamma) to
//   Student-t             u = eps sqrt(nu / (2 gamma))
//   generalised Gaussian  u = sign(eps) gamma^(1 / beta),  f = -gamma
// and writes z = loc + exp(log_scale) u with its log density in the same launch.
//
// The kernels are streams over [B, D].  A group of G <= 64 lanes owns a sample and lane g the packs g, g + G, ... of its
// row (16-byte packs when D and the buffers allow).  A lane meets the same features in every sample it visits, so up to
// kRegPacks packs of the parameter rows live in its registers, read once per launch; longer rows are read from memory
// (through the cache) beside the samples.  The VJP kernels keep the parameter sums in registers the same way: over a
// lane's samples in ascending order, then over the workgroup's lane groups through LDS in ascending order; rows too long
// for that go to a kernel in which a lane owns one pack of features and walks the samples.  Every workgroup writes one
// block [3, D] (d_loc | d_log_scale | the data part of d_shape) and reduce_partials adds the blocks in a fixed order.
// No atomics anywhere: the same call twice gives the same bits.
#include "stream_common.hpp"

namespace vcnf_tail {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr int kRegPacks = 2;                  // packs of a row a lane keeps in registers
constexpr int kMaxFwdBlocks = 2048;

// ------------------------------------------------------------------ the two families
// f(u; shape)
template <int F, typename T>
__device__ __forceinline__ T density(T u, T sh) {
  if (F == VCNF_TAIL_STUDENT_T) return T(-0.5) * (sh + T(1)) * log1p_(u * u / sh);
  const T a = abs_(u);
  return a == T(0) ? T(0) : -exp_(sh * log_(a));
}

// fu = df/du, fs = df/dshape.  Generalised Gaussian at u == 0: both 0 for every beta (the limit of -|u|^beta log|u|;
// for beta < 1, where df/du is unbounded, a convention)
template <int F, typename T>
__device__ __forceinline__ void density_grad(T u, T sh, T& fu, T& fs) {
  if (F == VCNF_TAIL_STUDENT_T) {
    const T uu = u * u, den = sh + uu;
    fu = -(sh + T(1)) * u / den;
    fs = T(-0.5) * log1p_(uu / sh) + (sh + T(1)) * uu / (T(2) * sh * den);
  } else {
    const T a = abs_(u);
    if (a == T(0)) {
      fu = fs = T(0);
    } else {
      const T l = log_(a), p = exp_(sh * l);
      fu = -sh * p / u;
      fs = -p * l;
    }
  }
}

// ------------------------------------------------------------------ parameter rows
template <typename T>
struct Rows {
  const T *loc, *ls, *shape, *cst;             // cst is NULL in the VJPs
  int D;
};

// one pack of the rows as a lane holds it: sc = exp(log_scale) when sampling, 1 / exp(log_scale) for the density;
// k = cst - log_scale
template <typename T, int V>
struct RowPack {
  T loc[V], sc[V], sh[V], k[V];
};

template <typename T, int V, bool SAMPLE>
__device__ __forceinline__ RowPack<T, V> load_rows(const Rows<T>& r, int v) {
  RowPack<T, V> p;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int i = v * V + j;
    const T ls = r.ls[i], e = exp_(ls);
    p.loc[j] = r.loc[i];
    p.sc[j] = SAMPLE ? e : T(1) / e;
    p.sh[j] = r.shape[i];
    p.k[j] = r.cst ? r.cst[i] - ls : T(0);
  }
  return p;
}

// u of the sample kernels from the two draws
template <int F, typename T>
__device__ __forceinline__ T draw_u(T e, T gm, T sh) {
  if (F == VCNF_TAIL_STUDENT_T) return e * sqrt_(sh / (T(2) * gm));
  const T sg = e > T(0) ? T(1) : e < T(0) ? T(-1) : T(0);
  return sg * exp_(log_(gm) / sh);
}

// ------------------------------------------------------------------ log_prob / sample
template <typename T>
struct FwdArgs {
  Rows<T> r;
  const T *in, *gamma;       // z, or eps and gamma when sampling
  T *z, *logp;
  long long B;
  int G, ld_mode;
  T sign;
};

template <typename T, int V, int F, bool REG, bool SAMPLE>
__global__ __launch_bounds__(kBlock) void tail_fwd_kernel(const FwdArgs<T> a) {
  using PackT = Pack<T, V>;
  using RowT = RowPack<T, V>;
  const int D = a.r.D, G = a.G, g = threadIdx.x & (G - 1), per_block = kBlock / G;
  const int nv = D / V;
  RowT rp[REG ? kRegPacks : 1];
  if (REG) {
#pragma unroll
    for (int p = 0; p < kRegPacks; ++p)
      if (g + p * G < nv) rp[p] = load_rows<T, V, SAMPLE>(a.r, g + p * G);
  }
  for (long long b = (long long)blockIdx.x * per_block + threadIdx.x / G; b < a.B; b += (long long)gridDim.x * per_block) {
    const PackT* __restrict__ in = reinterpret_cast<const PackT*>(a.in + b * D);
    const PackT* __restrict__ gm = SAMPLE ? reinterpret_cast<const PackT*>(a.gamma + b * D) : nullptr;
    PackT* __restrict__ zo = SAMPLE ? reinterpret_cast<PackT*>(a.z + b * D) : nullptr;
    T s = 0;
    auto pack = [&](int v, const RowT& r) {
      const PackT x = in[v];
      if (SAMPLE) {
        const PackT y = gm[v];
        PackT o;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T u = draw_u<F>(x.v[j], y.v[j], r.sh[j]);
          o.v[j] = r.loc[j] + r.sc[j] * u;
          s += r.k[j] + (F == VCNF_TAIL_GEN_GAUSSIAN ? -y.v[j] : density<F>(u, r.sh[j]));
        }
        zo[v] = o;
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) s += r.k[j] + density<F>((x.v[j] - r.loc[j]) * r.sc[j], r.sh[j]);
      }
    };
    if (REG) {
#pragma unroll
      for (int p = 0; p < kRegPacks; ++p)
        if (g + p * G < nv) pack(g + p * G, rp[p]);
    } else {
      for (int v = g; v < nv; v += G) pack(v, load_rows<T, V, SAMPLE>(a.r, v));
    }
    s = lanes_sum(s, 1, G);
    if (g == 0) {
      const T lp = a.sign * s;
      put_ld(a.logp, b, lp, a.ld_mode);
    }
  }
}

// ------------------------------------------------------------------ the VJPs
// OP 0, log_prob:  x = z,   y = gz_in (or NULL), g = cotangent of logp;           out1 = dz
// OP 1, sample:    x = eps, y = gamma,           g = g_lp (or NULL), gz = g_z (or NULL); out1 = deps (or NULL), out2 = dgamma
template <typename T>
struct BwdArgs {
  Rows<T> r;
  const T *x, *y, *g, *gz;
  T *out1, *out2, *partials;
  long long B;
  int G;
};

template <typename T, int V>
struct Sums {
  T loc[V], ls[V], sh[V];
};

template <typename T, int V>
__device__ __forceinline__ void clear(Sums<T, V>& s) {
#pragma unroll
  for (int j = 0; j < V; ++j) s.loc[j] = s.ls[j] = s.sh[j] = T(0);
}

// one pack of one sample: the elementwise outputs, and the sample's terms added to the lane's parameter sums
template <typename T, int V, int F, int OP>
__device__ __forceinline__ void bwd_pack(const BwdArgs<T>& a, long long b, int v, T gb, const RowPack<T, V>& r, Sums<T, V>& acc) {
  using PackT = Pack<T, V>;
  const long long at = b * (a.r.D / V) + v;
  const PackT x = reinterpret_cast<const PackT*>(a.x)[at];
  if (OP == 0) {
    PackT dz;
    if (a.y) {
      dz = reinterpret_cast<const PackT*>(a.y)[at];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) dz.v[j] = T(0);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const T u = (x.v[j] - r.loc[j]) * r.sc[j];
      T fu, fs;
      density_grad<F>(u, r.sh[j], fu, fs);
      const T t = gb * fu * r.sc[j];
      dz.v[j] += t;
      acc.loc[j] -= t;
      acc.ls[j] += gb * (T(-1) - fu * u);
      acc.sh[j] += gb * fs;
    }
    reinterpret_cast<PackT*>(a.out1)[at] = dz;
  } else {
    const PackT y = reinterpret_cast<const PackT*>(a.y)[at];
    PackT gz, de, dg;
    if (a.gz) {
      gz = reinterpret_cast<const PackT*>(a.gz)[at];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) gz.v[j] = T(0);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const T e = x.v[j], gm = y.v[j], sh = r.sh[j];
      const T u = draw_u<F>(e, gm, sh);
      const T gzs = gz.v[j] * r.sc[j];
      if (F == VCNF_TAIL_STUDENT_T) {
        T fu, fs;
        density_grad<F>(u, sh, fu, fs);
        const T gu = gzs + gb * fu;
        de.v[j] = gu * sqrt_(sh / (T(2) * gm));
        dg.v[j] = -gu * u / (T(2) * gm);
        acc.sh[j] += gu * u / (T(2) * sh) + gb * fs;
      } else {
        // f = -gamma whatever beta; u == 0 (eps == 0 or gamma == 0) moves with neither draw
        const bool zero = u == T(0);
        de.v[j] = T(0);
        dg.v[j] = (zero ? T(0) : gzs * u / (sh * gm)) - gb;
        acc.sh[j] += zero ? T(0) : -gzs * u * log_(gm) / (sh * sh);
      }
      acc.loc[j] += gz.v[j];
      acc.ls[j] += gzs * u - gb;
    }
    if (a.out1) reinterpret_cast<PackT*>(a.out1)[at] = de;
    reinterpret_cast<PackT*>(a.out2)[at] = dg;
  }
}

// rows of at most kRegPacks * 64 packs: a lane group per sample
template <typename T, int V, int F, int OP>
__global__ __launch_bounds__(kBlock) void tail_bwd_rows_kernel(const BwdArgs<T> a) {
  using RowT = RowPack<T, V>;
  // [lane group][3][D] with D <= kRegPacks G V: at most kBlock * 3 * kRegPacks packs of 16 bytes
  __shared__ __align__(16) unsigned char tail_lds[kBlock * 3 * kRegPacks * 16];
  T* red = reinterpret_cast<T*>(tail_lds);
  const int D = a.r.D, G = a.G, g = threadIdx.x & (G - 1), slot = threadIdx.x / G, per_block = kBlock / G;
  const int nv = D / V;
  RowT rp[kRegPacks];
  Sums<T, V> acc[kRegPacks];
#pragma unroll
  for (int p = 0; p < kRegPacks; ++p) {
    clear(acc[p]);
    if (g + p * G < nv) rp[p] = load_rows<T, V, OP == 1>(a.r, g + p * G);
  }
  for (long long b = (long long)blockIdx.x * per_block + slot; b < a.B; b += (long long)gridDim.x * per_block) {
    const T gb = a.g ? a.g[b] : T(0);
#pragma unroll
    for (int p = 0; p < kRegPacks; ++p)
      if (g + p * G < nv) bwd_pack<T, V, F, OP>(a, b, g + p * G, gb, rp[p], acc[p]);
  }
  if (!a.partials) return;
#pragma unroll
  for (int p = 0; p < kRegPacks; ++p) {
    const int v = g + p * G;
    if (v < nv) {
      T* row = red + (long long)slot * 3 * D + v * V;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        row[j] = acc[p].loc[j];
        row[D + j] = acc[p].ls[j];
        row[2 * D + j] = acc[p].sh[j];
      }
    }
  }
  __syncthreads();
  T* block = a.partials + (long long)blockIdx.x * 3 * D;
  for (int e = threadIdx.x; e < 3 * D; e += kBlock) {
    T s = red[e];
    for (int k = 1; k < per_block; ++k) s += red[k * 3 * D + e];
    block[e] = s;
  }
}

// longer rows: a lane owns one pack of features and walks the samples b = k, k + groups, ... of its workgroup row k
template <typename T, int V, int F, int OP>
__global__ __launch_bounds__(kBlock) void tail_bwd_cols_kernel(const BwdArgs<T> a) {
  const int D = a.r.D, nv = D / V;
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= nv) return;
  const RowPack<T, V> rp = load_rows<T, V, OP == 1>(a.r, v);
  Sums<T, V> acc;
  clear(acc);
  for (long long b = blockIdx.y; b < a.B; b += gridDim.y) bwd_pack<T, V, F, OP>(a, b, v, a.g ? a.g[b] : T(0), rp, acc);
  if (!a.partials) return;
  T* block = a.partials + (long long)blockIdx.y * 3 * D + v * V;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    block[j] = acc.loc[j];
    block[D + j] = acc.ls[j];
    block[2 * D + j] = acc.sh[j];
  }
}

// element e of the summed block [3, D] goes to d_loc | d_log_scale | d_shape [D]
template <typename T>
struct RowsDest {
  T *d_loc, *d_ls, *d_shape;
  int D;
  __device__ T* operator()(long long e) const {
    return e < D ? d_loc + e : e < 2LL * D ? d_ls + (e - D) : d_shape + (e - 2LL * D);
  }
};

// ------------------------------------------------------------------ host side
constexpr IntList<VCNF_TAIL_STUDENT_T, VCNF_TAIL_GEN_GAUSSIAN> kFamilies{};
static inline bool ok_family(int f) { return in_list(kFamilies, f); }

static int check_shape(int64_t batch, int32_t D) { return batch < 0 || D < 1 ? VCNF_ERR_SHAPE : VCNF_OK; }

// number of partial blocks = workgroups (workgroup rows) of a VJP: a pure function of the shape
static long long bwd_groups(int64_t batch, int32_t D) {
  long long cap = (1LL << 21) / (3LL * D);          // workspace of at most 2^21 elements, or 128 blocks
  cap = cap < 128 ? 128 : cap > 2048 ? 2048 : cap;
  const long long n = (batch + 15) / 16;
  return n < 1 ? 1 : n > cap ? cap : n;
}

template <typename T, int V, int F, int OP>
static int launch_bwd(BwdArgs<T> a, hipStream_t st) {
  const int nv = a.r.D / V;
  const unsigned groups = (unsigned)bwd_groups(a.B, a.r.D);
  if (nv <= kRegPacks * 64) {
    a.G = pick_lanes((nv + kRegPacks - 1) / kRegPacks);
    hipLaunchKernelGGL((tail_bwd_rows_kernel<T, V, F, OP>), dim3(groups), dim3(kBlock), 0, st, a);
  } else {
    hipLaunchKernelGGL((tail_bwd_cols_kernel<T, V, F, OP>), dim3((unsigned)((nv + kBlock - 1) / kBlock), groups), dim3(kBlock),
                       0, st, a);
  }
  return launched();
}

// launch(V, F): the pack width of the streamed buffers and the family as constants
template <typename T, typename L>
static int with_pack_family(int32_t D, std::initializer_list<const void*> bufs, int family, L&& launch) {
  return with_pack<T>(D, bufs, [&](auto V) {
    return launch_listed(kFamilies, family, [&](auto F) { return launch(V, F); });
  });
}

template <typename T>
static int forward(const T* in, const T* gamma, const T* loc, const T* ls, const T* shape, const T* cst, T* z, T* logp,
                   int64_t batch, int32_t D, int family, int ld_mode, T sign, bool sample, void* stream) {
  if (const int st = check_shape(batch, D)) return st;
  if (!ok_family(family) || !ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!in || !loc || !ls || !shape || !cst || !logp || (sample && (!gamma || !z))) return VCNF_ERR_NULL;
  if (!all_aligned({in, gamma, loc, ls, shape, cst, z, logp}, sizeof(T))) return VCNF_ERR_ALIGN;
  FwdArgs<T> a{Rows<T>{loc, ls, shape, cst, D}, in, gamma, z, logp, batch, 1, ld_mode, sign};
  return with_pack_family<T>(D, {in, gamma, z}, family, [&](auto V, auto F) {
    const int nv = D / V();
    const bool reg = nv <= kRegPacks * 64;
    a.G = reg ? pick_lanes((nv + kRegPacks - 1) / kRegPacks) : 64;
    const dim3 grid = grid_for(batch, a.G, kBlock, kMaxFwdBlocks);
    return with_flags([&](auto REG, auto SAMPLE) {
      hipLaunchKernelGGL((tail_fwd_kernel<T, V(), F(), REG(), SAMPLE()>), grid, dim3(kBlock), 0, (hipStream_t)stream, a);
      return launched();
    }, reg, sample);
  });
}

template <typename T>
static int log_prob_bwd(const T* z, const T* loc, const T* ls, const T* shape, const T* g, const T* gz_in, T* dz, T* partials,
                        int64_t batch, int32_t D, int family, void* stream) {
  if (const int st = check_shape(batch, D)) return st;
  if (!ok_family(family)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!z || !loc || !ls || !shape || !g || !dz) return VCNF_ERR_NULL;
  if (!all_aligned({z, loc, ls, shape, g, gz_in, dz, partials}, sizeof(T))) return VCNF_ERR_ALIGN;
  const BwdArgs<T> a{Rows<T>{loc, ls, shape, nullptr, D}, z, gz_in, g, nullptr, dz, nullptr, partials, batch, 1};
  return with_pack_family<T>(D, {z, gz_in, dz}, family,
                             [&](auto V, auto F) { return launch_bwd<T, V(), F(), 0>(a, (hipStream_t)stream); });
}

template <typename T>
static int sample_bwd(const T* eps, const T* gamma, const T* loc, const T* ls, const T* shape, const T* g_z, const T* g_lp,
                      T* deps, T* dgamma, T* partials, int64_t batch, int32_t D, int family, void* stream) {
  if (const int st = check_shape(batch, D)) return st;
  if (!ok_family(family)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!eps || !gamma || !loc || !ls || !shape || !dgamma) return VCNF_ERR_NULL;
  if (!all_aligned({eps, gamma, loc, ls, shape, g_z, g_lp, deps, dgamma, partials}, sizeof(T))) return VCNF_ERR_ALIGN;
  const BwdArgs<T> a{Rows<T>{loc, ls, shape, nullptr, D}, eps, gamma, g_lp, g_z, deps, dgamma, partials, batch, 1};
  return with_pack_family<T>(D, {eps, gamma, g_z, deps, dgamma}, family,
                             [&](auto V, auto F) { return launch_bwd<T, V(), F(), 1>(a, (hipStream_t)stream); });
}

template <typename T>
static int reduce_partials(const T* partials, int64_t groups, int32_t D, T* d_loc, T* d_ls, T* d_shape, void* stream) {
  if (groups < 1 || D < 1) return VCNF_ERR_SHAPE;
  if (!partials || !d_loc || !d_ls || !d_shape) return VCNF_ERR_NULL;
  if (!all_aligned({partials, d_loc, d_ls, d_shape}, sizeof(T))) return VCNF_ERR_ALIGN;
  return launch_reduce_partials(partials, groups, 3LL * D, RowsDest<T>{d_loc, d_ls, d_shape, D}, stream);
}

}  // namespace vcnf_tail

using namespace vcnf_tail;

extern "C" int64_t vcnf_tail_bwd_groups(int64_t batch, int32_t features) {
  if (check_shape(batch, features) != VCNF_OK) return 0;
  return bwd_groups(batch, features);
}

#define VCNF_TAIL_ENTRY_POINTS(T, SFX)                                                                                 \
  extern "C" int vcnf_tail_log_prob_##SFX(const T* z, const T* loc, const T* log_scale, const T* shape, const T* cst,  \
                                          T* logp, int64_t batch, int32_t features, int family, int ld_mode, T sign,   \
                                          void* stream) {                                                              \
    return forward<T>(z, nullptr, loc, log_scale, shape, cst, nullptr, logp, batch, features, family, ld_mode, sign,   \
                      false, stream);                                                                                  \
  }                                                                                                                    \
  extern "C" int vcnf_tail_sample_##SFX(const T* eps, const T* gamma, const T* loc, const T* log_scale, const T* shape, \
                                        const T* cst, T* z, T* logp, int64_t batch, int32_t features, int family,      \
                                        void* stream) {                                                                \
    return forward<T>(eps, gamma, loc, log_scale, shape, cst, z, logp, batch, features, family, VCNF_LD_STORE, T(1),   \
                      true, stream);                                                                                   \
  }                                                                                                                    \
  extern "C" int vcnf_tail_log_prob_bwd_##SFX(const T* z, const T* loc, const T* log_scale, const T* shape,            \
                                              const T* g, const T* gz_in, T* dz, T* partials, int64_t batch,           \
                                              int32_t features, int family, void* stream) {                            \
    return log_prob_bwd<T>(z, loc, log_scale, shape, g, gz_in, dz, partials, batch, features, family, stream);         \
  }                                                                                                                    \
  extern "C" int vcnf_tail_sample_bwd_##SFX(const T* eps, const T* gamma, const T* loc, const T* log_scale,            \
                                            const T* shape, const T* g_z, const T* g_lp, T* deps, T* dgamma,           \
                                            T* partials, int64_t batch, int32_t features, int family, void* stream) {  \
    return sample_bwd<T>(eps, gamma, loc, log_scale, shape, g_z, g_lp, deps, dgamma, partials, batch, features,        \
                         family, stream);                                                                              \
  }                                                                                                                    \
  extern "C" int vcnf_tail_reduce_partials_##SFX(const T* partials, int64_t groups, int32_t features, T* d_loc,        \
                                                 T* d_log_scale, T* d_shape, void* stream) {                           \
    return reduce_partials<T>(partials, groups, features, d_loc, d_log_scale, d_shape, stream);                        \
  }

VCNF_TAIL_ENTRY_POINTS(float, f32)
VCNF_TAIL_ENTRY_POINTS(double, f64)
