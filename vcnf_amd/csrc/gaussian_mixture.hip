// Gaussian mixture base distribution for MI355X (gfx950, wave64): the arithmetic of the reference's GaussianMixture
// (normflow 1.2 distributions/base.py) with the parameters given as tables loc / log_scale [M, D] and the log mixture
// weights log_w [M]:
//   a[b, m] = log_w[m] - sum_d log_scale[m, d] - 0.5 D log(2 pi) - 0.5 sum_d ((z[b, d] - loc[m, d]) / exp(log_scale[m, d]))^2
//   logp[b] = logsumexp_m a[b, m]
//
// Every workgroup stages inv = 1 / exp(log_scale), loc and the per-mode constant c[m] (everything of a[b, m] that does not
// depend on z) in LDS once and then streams its samples.  A group of G <= 64 lanes owns a sample: lane g holds the packs
// g, g + G, ... of the row (16-byte packs when D allows) in registers, so z is read from memory once; rows of more than
// kRegPacks * 64 packs are re-read through the cache for every mode instead.  Per mode the lanes' partial sums are added
// with a shuffle butterfly and every lane of the group carries the running (max, sum) of the logsumexp, which stays
// finite wherever the result is (rows whose every a[b, m] is far below the exp range included).
//   sample:  z = eps * exp(log_scale[mode]) + loc[mode] from the mode's table row in memory, then the density of that
//            z in the same launch.  A mode outside [0, M) reads row 0 and writes NaN into that sample's z row and logp.
//   VJP:     one wave per workgroup.  With the forward's logp as lse the responsibilities r = exp(a - lse) need no
//            second pass over the modes.  The wave adds the contributions of its samples to d_loc / d_log_scale / d_log_w
//            with a shuffle butterfly across the lane groups and keeps the running sums in LDS (in its block of the
//            caller's workspace when LDS cannot hold them), each table entry owned by one lane; the workgroup's block
//            [M, 2 D + 1] goes to the workspace and reduce_partials adds the blocks in a fixed order.
// No atomics anywhere: the same call twice gives the same bits.
#include "stream_common.hpp"

namespace vcnf_gmm {

using namespace vcnf_stream;

constexpr int kFwdBlock = 256;
constexpr int kBwdBlock = 64;                 // one wave: the cross-sample sums are shuffles, no barrier in the loop
constexpr int kRegPacks = 4;                  // packs of a row a lane keeps in registers
constexpr int kMaxFwdBlocks = 2048;
constexpr int kMaxTable = VCNF_GMM_MAX_TABLE; // M * D
constexpr size_t kLdsBytes = 160 * 1024;

// Every sum over lanes in this unit is the ascending lanes_sum: inside a lane group (1, G), across the groups (G, 64).

// c[m] = log_w[m] - sum_d log_scale[m, d] + norm, summed by one whole wave in a fixed order
template <typename T>
__device__ __forceinline__ T mode_const_wave(const T* __restrict__ ls, const T* __restrict__ logw, int m, int D, T norm) {
  const int lane = threadIdx.x & 63;
  T s = 0;
  for (int d = lane; d < D; d += 64) s += ls[(long long)m * D + d];
  s = lanes_sum(s, 1, 64);
  return logw[m] - s + norm;
}

// the same by one lane on its own: inside the sample loops when LDS has no room for c (then D <= 2)
template <typename T>
__device__ __forceinline__ T mode_const_lane(const T* __restrict__ ls, const T* __restrict__ logw, int m, int D, T norm) {
  T s = 0;
  for (int d = 0; d < D; ++d) s += ls[(long long)m * D + d];
  return logw[m] - s + norm;
}

// LDS image: inv [M D] | loc [M D] | c [M] (when it fits).  Ends with a barrier.
template <typename T>
__device__ __forceinline__ void stage_tables(T* inv, T* loc, T* cs, const T* __restrict__ g_loc,
                                             const T* __restrict__ g_ls, const T* __restrict__ g_logw, int M, int D, T norm) {
  const int n = M * D;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    inv[i] = T(1) / exp_(g_ls[i]);
    loc[i] = g_loc[i];
  }
  if (cs) {
    const int waves = blockDim.x >> 6;
    for (int m = threadIdx.x >> 6; m < M; m += waves) {
      const T c = mode_const_wave(g_ls, g_logw, m, D, norm);
      if ((threadIdx.x & 63) == 0) cs[m] = c;
    }
  }
  __syncthreads();
}

// q = sum over the lane's elements of ((z - loc[m]) inv[m])^2
template <typename T, int V, bool REG>
__device__ __forceinline__ T slice_q(const Pack<T, V>* zr, const Pack<T, V>* __restrict__ src, const T* inv_m,
                                     const T* loc_m, int g, int G, int nv) {
  using PackT = Pack<T, V>;
  const PackT* im = reinterpret_cast<const PackT*>(inv_m);
  const PackT* lm = reinterpret_cast<const PackT*>(loc_m);
  T q = 0;
  if (REG) {
#pragma unroll
    for (int p = 0; p < kRegPacks; ++p) {
      const int v = g + p * G;
      if (v < nv) {
        const PackT i = im[v], l = lm[v];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T u = (zr[p].v[j] - l.v[j]) * i.v[j];
          q += u * u;
        }
      }
    }
  } else {
    for (int v = g; v < nv; v += G) {
      const PackT x = src[v], i = im[v], l = lm[v];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const T u = (x.v[j] - l.v[j]) * i.v[j];
        q += u * u;
      }
    }
  }
  return q;
}

template <typename T>
struct Tables {
  const T *loc, *ls, *logw;
  int D, M, c_lds;           // c_lds: c[m] fits in LDS beside the tables (else it is summed from memory where needed)
  T norm;                    // -0.5 D log(2 pi)
};

// ------------------------------------------------------------------ log_prob / sample
template <typename T>
struct FwdArgs {
  Tables<T> t;
  const T* in;               // z, or eps when sampling
  const int32_t* mode;       // sampling only
  T *z, *logp;
  long long B;
  int G, ld_mode, sample;
  T sign;
};

template <typename T, int V, bool REG>
__global__ __launch_bounds__(kFwdBlock) void gmm_fwd_kernel(const FwdArgs<T> a) {
  using PackT = Pack<T, V>;
  extern __shared__ __align__(16) unsigned char gmm_lds[];
  const int D = a.t.D, M = a.t.M;
  T* inv = reinterpret_cast<T*>(gmm_lds);
  T* loc = inv + M * D;
  T* cs = a.t.c_lds ? loc + M * D : nullptr;
  stage_tables(inv, loc, cs, a.t.loc, a.t.ls, a.t.logw, M, D, a.t.norm);

  const int G = a.G, g = threadIdx.x & (G - 1), per_block = kFwdBlock / G;
  const int nv = D / V;
  for (long long b = (long long)blockIdx.x * per_block + threadIdx.x / G; b < a.B; b += (long long)gridDim.x * per_block) {
    const PackT* __restrict__ in = reinterpret_cast<const PackT*>(a.in + b * D);
    const PackT* src = in;
    PackT zr[REG ? kRegPacks : 1];
    bool bad = false;
    if (a.sample) {
      const int md = a.mode[b];
      bad = md < 0 || md >= M;
      const T* __restrict__ lrow = a.t.loc + (long long)(bad ? 0 : md) * D;
      const T* __restrict__ srow = a.t.ls + (long long)(bad ? 0 : md) * D;
      PackT* __restrict__ out = reinterpret_cast<PackT*>(a.z + b * D);
      src = out;                                  // rows that are not kept in registers are re-read from z
      auto draw = [&](int v) {
        const PackT e = in[v];
        PackT o;
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[j] = e.v[j] * exp_(srow[v * V + j]) + lrow[v * V + j];
        PackT w = o;
        if (bad) {
#pragma unroll
          for (int j = 0; j < V; ++j) w.v[j] = T(NAN);
        }
        out[v] = w;
        return o;
      };
      if (REG) {
#pragma unroll
        for (int p = 0; p < kRegPacks; ++p)
          if (g + p * G < nv) zr[p] = draw(g + p * G);
      } else {
        for (int v = g; v < nv; v += G) draw(v);
      }
    } else if (REG) {
#pragma unroll
      for (int p = 0; p < kRegPacks; ++p)
        if (g + p * G < nv) zr[p] = in[g + p * G];
    }
    // running logsumexp over the modes: mx = max so far, s = sum of exp(a - mx)
    T mx = -INFINITY, s = 0;
    for (int m = 0; m < M; ++m) {
      T q = slice_q<T, V, REG>(zr, src, inv + m * D, loc + m * D, g, G, nv);
      q = lanes_sum(q, 1, G);
      const T c = cs ? cs[m] : mode_const_lane(a.t.ls, a.t.logw, m, D, a.t.norm);
      const T am = c - T(0.5) * q;
      T e = exp_(-abs_(am - mx));
      if (am == -INFINITY) e = 0;                 // contributes nothing (and -inf - -inf is not a number)
      if (am > mx) {
        s = s * e + T(1);
        mx = am;
      } else {
        s += e;
      }
    }
    if (g == 0) {
      const T lp = bad ? T(NAN) : a.sign * (mx + log_(s));
      put_ld(a.logp, b, lp, a.ld_mode);
    }
  }
}

// ------------------------------------------------------------------ VJP of log_prob
template <typename T>
struct BwdArgs {
  Tables<T> t;
  const T *z, *lse, *g, *gz_in;
  T *dz, *partials;
  long long B;
  int G;
};

// ACC_LDS: the running parameter sums live in LDS behind the tables, else in the workgroup's block of the workspace
template <typename T, int V, bool REG, bool ACC_LDS>
__global__ __launch_bounds__(kBwdBlock) void gmm_bwd_kernel(const BwdArgs<T> a) {
  using PackT = Pack<T, V>;
  extern __shared__ __align__(16) unsigned char gmm_lds[];
  const int D = a.t.D, M = a.t.M;
  const int W = 2 * D + 1;                       // row of the partial block: d_loc [D] | d_log_scale [D] | d_log_w
  T* inv = reinterpret_cast<T*>(gmm_lds);
  T* loc = inv + M * D;
  T* cs = a.t.c_lds ? loc + M * D : nullptr;
  T* block = a.partials + (long long)blockIdx.x * M * W;
  T* acc = ACC_LDS ? loc + M * D + (a.t.c_lds ? M : 0) : block;
  const bool sums = a.partials != nullptr;       // without a workspace only dz is wanted
  if (sums)
    for (int i = threadIdx.x; i < M * W; i += kBwdBlock) acc[i] = 0;
  stage_tables(inv, loc, cs, a.t.loc, a.t.ls, a.t.logw, M, D, a.t.norm);

  const int G = a.G, lane = threadIdx.x, g = lane & (G - 1), per_wave = 64 / G;
  const bool owner = lane < G;                   // the first lane group adds the wave's sums to the running ones
  const int nv = D / V;
  // every lane stays in the loop (the sums across the lane groups need the whole wave); a slot past the batch adds zeros
  for (long long b0 = (long long)blockIdx.x * per_wave; b0 < a.B; b0 += (long long)gridDim.x * per_wave) {
    const long long b = b0 + lane / G;
    const bool valid = b < a.B;
    const long long br = valid ? b : 0;
    const PackT* __restrict__ zin = reinterpret_cast<const PackT*>(a.z + br * D);
    const PackT* __restrict__ gzin = a.gz_in ? reinterpret_cast<const PackT*>(a.gz_in + br * D) : nullptr;
    PackT* __restrict__ dzo = reinterpret_cast<PackT*>(a.dz + br * D);
    const T gb = a.g[br], lse = a.lse[br];
    PackT zr[REG ? kRegPacks : 1], dzr[REG ? kRegPacks : 1];
    if (REG) {
#pragma unroll
      for (int p = 0; p < kRegPacks; ++p) {
        const int v = g + p * G;
        if (v < nv) {
          zr[p] = zin[v];
          if (gzin) {
            dzr[p] = gzin[v];
          } else {
#pragma unroll
            for (int j = 0; j < V; ++j) dzr[p].v[j] = 0;
          }
        }
      }
    }
    for (int m = 0; m < M; ++m) {
      const T* inv_m = inv + m * D;
      const T* loc_m = loc + m * D;
      T q = slice_q<T, V, REG>(zr, zin, inv_m, loc_m, g, G, nv);
      q = lanes_sum(q, 1, G);
      const T c = cs ? cs[m] : mode_const_lane(a.t.ls, a.t.logw, m, D, a.t.norm);
      const T gr = valid ? gb * exp_(c - T(0.5) * q - lse) : T(0);      // g x responsibility
      T* acc_m = acc + m * W;
      // one pack of the lane's slice: dz, and the sums of d_loc / d_log_scale over the wave's samples
      auto pack = [&](int v, const PackT& x, PackT& dzp) {
        const bool have = v < nv;
        PackT tl, tq;
        if (have && valid) {
          const PackT i = reinterpret_cast<const PackT*>(inv_m)[v], l = reinterpret_cast<const PackT*>(loc_m)[v];
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T u = (x.v[j] - l.v[j]) * i.v[j];
            tl.v[j] = gr * u * i.v[j];
            tq.v[j] = gr * (u * u - T(1));
            dzp.v[j] -= tl.v[j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) tl.v[j] = tq.v[j] = 0;
        }
        if (!sums) return;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          tl.v[j] = lanes_sum(tl.v[j], G, 64);
          tq.v[j] = lanes_sum(tq.v[j], G, 64);
        }
        if (owner && have) {
          T* al = acc_m + v * V;
          T* aq = acc_m + D + v * V;
          T ol[V], oq[V];
#pragma unroll
          for (int j = 0; j < V; ++j) {
            ol[j] = al[j];
            oq[j] = aq[j];
          }
#pragma unroll
          for (int j = 0; j < V; ++j) {
            al[j] = ol[j] + tl.v[j];
            aq[j] = oq[j] + tq.v[j];
          }
        }
      };
      if (REG) {
#pragma unroll
        for (int p = 0; p < kRegPacks; ++p)
          if (p * G < nv) pack(g + p * G, zr[p], dzr[p]);
      } else {
        for (int v0 = 0; v0 < nv; v0 += G) {
          const int v = v0 + g;
          PackT x, dzp;
          if (v < nv && valid) {               // a slot past the batch touches no row
            x = zin[v];
            if (m > 0) {
              dzp = dzo[v];
            } else if (gzin) {
              dzp = gzin[v];
            } else {
#pragma unroll
              for (int j = 0; j < V; ++j) dzp.v[j] = 0;
            }
          }
          pack(v, x, dzp);
          if (v < nv && valid) dzo[v] = dzp;
        }
      }
      if (sums) {
        const T sw = lanes_sum(g == 0 ? gr : T(0), G, 64);
        if (lane == 0) acc_m[2 * D] += sw;
      }
    }
    if (REG && valid) {
#pragma unroll
      for (int p = 0; p < kRegPacks; ++p)
        if (g + p * G < nv) dzo[g + p * G] = dzr[p];
    }
  }
  if (ACC_LDS && sums) {
    __syncthreads();
    for (int i = threadIdx.x; i < M * W; i += kBwdBlock) block[i] = acc[i];
  }
}

// element (m, c) of the summed block [M, 2 D + 1] goes to d_loc [M, D] | d_log_scale [M, D] | d_log_w [M]
template <typename T>
struct TableDest {
  T *d_loc, *d_ls, *d_w;
  int D;
  __device__ T* operator()(long long e) const {
    const int W = 2 * D + 1;
    const int m = (int)(e / W), c = (int)(e - (long long)m * W);
    return c < D ? d_loc + m * D + c : c < 2 * D ? d_ls + m * D + c - D : d_w + m;
  }
};

// ------------------------------------------------------------------ host side
static int check_shape(int64_t batch, int32_t D, int32_t M) {
  if (batch < 0 || D < 1 || M < 1 || (long long)D * M > kMaxTable) return VCNF_ERR_SHAPE;
  return VCNF_OK;
}

// number of partial blocks = workgroups of the VJP: a pure function of the shape
static long long bwd_groups(int64_t batch, int32_t D, int32_t M) {
  const long long elems = (long long)M * (2LL * D + 1);
  long long cap = (1LL << 23) / elems;             // workspace of at most 2^23 elements, or 256 blocks
  cap = cap < 256 ? 256 : cap > 4096 ? 4096 : cap;
  long long n = (batch + 31) / 32;                 // one wave per workgroup: at least 32 samples each
  return n < 1 ? 1 : n > cap ? cap : n;
}

template <typename T>
static Tables<T> make_tables(const T* loc, const T* ls, const T* logw, int32_t D, int32_t M) {
  const size_t with_c = ((size_t)2 * M * D + M) * sizeof(T);
  return Tables<T>{loc, ls, logw, D, M, with_c <= kLdsBytes ? 1 : 0, (T)(-0.5 * (double)D * log(2.0 * M_PI))};
}

template <typename T>
static size_t table_bytes(const Tables<T>& t) {
  return ((size_t)2 * t.M * t.D + (t.c_lds ? t.M : 0)) * sizeof(T);
}

// a workgroup may take all of the CU's 160 KiB; beyond 64 KiB the runtime wants to be told (per device, so every time:
// unlike host_common.hpp's lds_limit_once, which tells it once per kernel instance, this sets the attribute on every
// launch above 64 KiB)
template <typename K>
static bool allow_lds(K kernel, size_t lds) {
  return lds <= 64 * 1024 || hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes) == hipSuccess;
}

template <typename T, int V, bool REG>
static int launch_fwd(const FwdArgs<T>& a, dim3 grid, size_t lds, hipStream_t st) {
  if (!allow_lds(&gmm_fwd_kernel<T, V, REG>, lds)) return VCNF_ERR_LAUNCH;
  hipLaunchKernelGGL((gmm_fwd_kernel<T, V, REG>), grid, dim3(kFwdBlock), lds, st, a);
  return launched();
}

template <typename T, int V, bool REG, bool ACC_LDS>
static int launch_bwd(const BwdArgs<T>& a, dim3 grid, size_t lds, hipStream_t st) {
  if (!allow_lds(&gmm_bwd_kernel<T, V, REG, ACC_LDS>, lds)) return VCNF_ERR_LAUNCH;
  hipLaunchKernelGGL((gmm_bwd_kernel<T, V, REG, ACC_LDS>), grid, dim3(kBwdBlock), lds, st, a);
  return launched();
}

template <typename T>
static int forward(const T* in, const int32_t* mode, const T* loc, const T* ls, const T* logw, T* z, T* logp, int64_t batch,
                   int32_t D, int32_t M, int ld_mode, T sign, int sample, void* stream) {
  if (const int st = check_shape(batch, D, M)) return st;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!in || !loc || !ls || !logw || !logp || (sample && (!z || !mode))) return VCNF_ERR_NULL;
  if (!all_aligned({in, loc, ls, logw, logp, z}, sizeof(T)) || !aligned(mode, 4)) return VCNF_ERR_ALIGN;
  FwdArgs<T> a{make_tables(loc, ls, logw, D, M), in, mode, z, logp, batch, 1, ld_mode, sample, sign};
  const size_t lds = table_bytes(a.t);
  return with_pack<T>(D, {in, z}, [&](auto V) {
    const int nv = D / V();
    a.G = pick_lanes(nv);
    const dim3 grid = grid_for(batch, a.G, kFwdBlock, kMaxFwdBlocks);
    return with_flags([&](auto REG) { return launch_fwd<T, V(), REG()>(a, grid, lds, (hipStream_t)stream); },
                      nv <= kRegPacks * a.G);
  });
}

template <typename T>
static int backward(const T* z, const T* loc, const T* ls, const T* logw, const T* lse, const T* g, const T* gz_in, T* dz,
                    T* partials, int64_t batch, int32_t D, int32_t M, void* stream) {
  if (const int st = check_shape(batch, D, M)) return st;
  if (batch == 0) return VCNF_OK;
  if (!z || !loc || !ls || !logw || !lse || !g || !dz) return VCNF_ERR_NULL;
  if (!all_aligned({z, loc, ls, logw, lse, g, gz_in, dz, partials}, sizeof(T))) return VCNF_ERR_ALIGN;
  BwdArgs<T> a{make_tables(loc, ls, logw, D, M), z, lse, g, gz_in, dz, partials, batch, 1};
  size_t lds = table_bytes(a.t);
  const size_t acc = (size_t)M * (2 * D + 1) * sizeof(T);
  const bool acc_lds = partials && lds + acc <= kLdsBytes;
  if (acc_lds) lds += acc;
  const dim3 grid((unsigned)bwd_groups(batch, D, M));
  return with_pack<T>(D, {z, gz_in, dz}, [&](auto V) {
    const int nv = D / V();
    a.G = pick_lanes(nv);
    return with_flags(
        [&](auto REG, auto ACC_LDS) { return launch_bwd<T, V(), REG(), ACC_LDS()>(a, grid, lds, (hipStream_t)stream); },
        nv <= kRegPacks * a.G, acc_lds);
  });
}

template <typename T>
static int reduce_partials(const T* partials, int64_t groups, int32_t M, int32_t D, T* d_loc, T* d_ls, T* d_w, void* stream) {
  if (groups < 1) return VCNF_ERR_SHAPE;
  if (const int st = check_shape(0, D, M)) return st;
  if (!partials || !d_loc || !d_ls || !d_w) return VCNF_ERR_NULL;
  if (!all_aligned({partials, d_loc, d_ls, d_w}, sizeof(T))) return VCNF_ERR_ALIGN;
  return launch_reduce_partials(partials, groups, (long long)M * (2LL * D + 1), TableDest<T>{d_loc, d_ls, d_w, D}, stream);
}

}  // namespace vcnf_gmm

using namespace vcnf_gmm;

extern "C" int64_t vcnf_gmm_bwd_groups(int64_t batch, int32_t features, int32_t modes) {
  if (check_shape(batch, features, modes) != VCNF_OK) return 0;
  return bwd_groups(batch, features, modes);
}

#define VCNF_GMM_ENTRY_POINTS(T, SFX)                                                                                  \
  extern "C" int vcnf_gmm_log_prob_##SFX(const T* z, const T* loc, const T* log_scale, const T* log_w, T* logp,        \
                                         int64_t batch, int32_t features, int32_t modes, int ld_mode, T sign,          \
                                         void* stream) {                                                               \
    return forward<T>(z, nullptr, loc, log_scale, log_w, nullptr, logp, batch, features, modes, ld_mode, sign, 0,      \
                      stream);                                                                                         \
  }                                                                                                                    \
  extern "C" int vcnf_gmm_sample_##SFX(const T* eps, const int32_t* mode, const T* loc, const T* log_scale,            \
                                       const T* log_w, T* z, T* logp, int64_t batch, int32_t features, int32_t modes,  \
                                       void* stream) {                                                                 \
    return forward<T>(eps, mode, loc, log_scale, log_w, z, logp, batch, features, modes, VCNF_LD_STORE, T(1), 1,       \
                      stream);                                                                                         \
  }                                                                                                                    \
  extern "C" int vcnf_gmm_log_prob_bwd_##SFX(const T* z, const T* loc, const T* log_scale, const T* log_w,             \
                                             const T* lse, const T* g, const T* gz_in, T* dz, T* partials,             \
                                             int64_t batch, int32_t features, int32_t modes, void* stream) {           \
    return backward<T>(z, loc, log_scale, log_w, lse, g, gz_in, dz, partials, batch, features, modes, stream);         \
  }                                                                                                                    \
  extern "C" int vcnf_gmm_reduce_partials_##SFX(const T* partials, int64_t groups, int32_t modes, int32_t features,    \
                                                T* d_loc, T* d_log_scale, T* d_log_w, void* stream) {                  \
    return reduce_partials<T>(partials, groups, modes, features, d_loc, d_log_scale, d_log_w, stream);                 \
  }

VCNF_GMM_ENTRY_POINTS(float, f32)
VCNF_GMM_ENTRY_POINTS(double, f64)
