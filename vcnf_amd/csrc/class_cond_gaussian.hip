// Class-conditional diagonal Gaussian end caps for MI355X (gfx950, wave64): the arithmetic of the reference's
// GlowBase (distributions/base.py:778-869) and ClassCondDiagGaussian (:715-775) with the parameters given as
// tables loc_rows / log_scale_rows [R, C] and an optional per-sample row index (the class label).  z[b, c, p] is a
// contiguous row of d = C * P elements; sample b uses table row row_index[b], or row b (R == B) / row 0 (R == 1)
// without an index.  A label outside [0, R) reads row 0 and that sample's outputs are written as NaN: no
// out-of-bounds access and nothing for the host to check, so the calls stay capturable.
//
// All kernels are HBM-bound maps with a reduction: every input element is read once, with 16-byte accesses when a
// pack of V elements stays inside one channel (P % V == 0) or the rows are flat (P == 1, C % V == 0).
//   forward (log_prob / sample): a group of G <= 64 lanes owns a sample and strides over its row (the lane ownership
//     and shuffle row sum of diag_gaussian_vec4_kernel); exp(log_scale) is evaluated when the lane's channel changes.
//   VJPs: a group of lanes owns one (sample, channel) segment of P elements, so the pixel sums of d_loc / d_ls are
//     shuffle sums inside the group; flat rows need no sum at all.
//   reduce_rows: the per-sample [B, C] gradients summed onto the R table rows in a fixed order.
// No atomics anywhere: the same call twice gives the same bits.
#include "stream_common.hpp"

namespace vcnf_cc {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 256 * 16;
constexpr int kReduceWaves = 16;

// Row and segment sums are lanes_sum_descending throughout this unit.

static inline dim3 grid_for(long long groups, int G) { return vcnf_stream::grid_for(groups, G, kBlock, kMaxBlocks); }

// table row of sample b; bad: the label is outside the table (row 0 is read instead, R >= 1)
__device__ __forceinline__ long long pick_row(const int32_t* idx, long long R, long long b, bool& bad) {
  if (!idx) {
    bad = false;
    return R == 1 ? 0 : b;
  }
  const long long r = idx[b];
  bad = r < 0 || r >= R;
  return bad ? 0 : r;
}

// ------------------------------------------------------------------ log_prob / sample
template <typename T>
struct FwdArgs {
  const T *in, *loc, *ls;
  const int32_t* idx;
  T *z, *logp;
  long long B, R;
  int C, P, G, ld_mode, sample;
  T log_temp, ld_sign, norm;   // norm = -0.5 * d * log(2 pi)
};

template <typename T, int V, bool FLAT>
__global__ __launch_bounds__(kBlock) void cc_gaussian_fwd_kernel(const FwdArgs<T> a) {
  using PackT = Pack<T, V>;
  const int g = threadIdx.x & (a.G - 1);
  const int per_block = kBlock / a.G;
  const int d = a.C * a.P;
  const int nv = d / V;                       // packs per row
  const int pv = FLAT ? 1 : a.P / V;          // packs per channel
  for (long long b = (long long)blockIdx.x * per_block + threadIdx.x / a.G; b < a.B;
       b += (long long)gridDim.x * per_block) {
    bool bad;
    const long long row = pick_row(a.idx, a.R, b, bad);
    const T* __restrict__ loc = a.loc + row * a.C;
    const T* __restrict__ lsr = a.ls + row * a.C;
    const PackT* __restrict__ in = reinterpret_cast<const PackT*>(a.in + b * d);
    PackT* __restrict__ out = reinterpret_cast<PackT*>(a.z + b * d);
    T acc = 0;
    int c_have = -1;
    T ls = 0, sc = 1, lc = 0;
    for (int v = g; v < nv; v += a.G) {
      const PackT x = in[v];
      PackT o;
      if (FLAT) {                              // a pack spans V channels
        const PackT l = reinterpret_cast<const PackT*>(loc)[v], s = reinterpret_cast<const PackT*>(lsr)[v];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          ls = s.v[j] + a.log_temp;
          sc = exp_(ls);
          if (a.sample) {
            o.v[j] = l.v[j] + sc * x.v[j];
            acc += ls + T(0.5) * x.v[j] * x.v[j];
          } else {
            const T u = (x.v[j] - l.v[j]) / sc;
            acc += ls + T(0.5) * u * u;
          }
        }
      } else {                                 // a pack lies inside one channel
        const int c = v / pv;
        if (c != c_have) {
          c_have = c;
          ls = lsr[c] + a.log_temp;
          sc = exp_(ls);
          lc = loc[c];
        }
        T q = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (a.sample) {
            o.v[j] = lc + sc * x.v[j];
            q += x.v[j] * x.v[j];
          } else {
            const T u = (x.v[j] - lc) / sc;
            q += u * u;
          }
        }
        acc += T(V) * ls + T(0.5) * q;
      }
      if (a.sample) {
        if (bad) {
#pragma unroll
          for (int j = 0; j < V; ++j) o.v[j] = T(NAN);
        }
        out[v] = o;
      }
    }
    acc = lanes_sum_descending(acc, a.G);
    if (g == 0) {
      const T lp = bad ? T(NAN) : a.ld_sign * (a.norm - acc);
      put_ld(a.logp, b, lp, a.ld_mode);
    }
  }
}

// ------------------------------------------------------------------ VJPs
// SAMPLE = false: in = z, gvec = g[B]:               out = dz,    d_loc = sum_p g u / s,  d_ls = sum_p g (u^2 - 1)
// SAMPLE = true:  in = eps, gz[B, d], gvec = g_lp[B]: out = d_eps, d_loc = sum_p g_z,      d_ls = sum_p g_z s eps - P g_lp
template <typename T>
struct BwdArgs {
  const T *in, *gz, *loc, *ls, *gvec;
  const int32_t* idx;
  T *out, *d_loc, *d_ls;
  long long B, R;
  int C, P, G;
  T log_temp;
};

template <typename T, int V, bool SAMPLE>
__global__ __launch_bounds__(kBlock) void cc_gaussian_bwd_kernel(const BwdArgs<T> a) {
  using PackT = Pack<T, V>;
  const int g = threadIdx.x & (a.G - 1);
  const int per_block = kBlock / a.G;
  const int pv = a.P / V;
  const long long segments = a.B * a.C;        // one (sample, channel) segment per lane group
  for (long long r = (long long)blockIdx.x * per_block + threadIdx.x / a.G; r < segments;
       r += (long long)gridDim.x * per_block) {
    const long long b = r / a.C;
    const int c = (int)(r - b * a.C);
    bool bad;
    const long long row = pick_row(a.idx, a.R, b, bad);
    const T sc = exp_(a.ls[row * a.C + c] + a.log_temp);
    const T inv = T(1) / sc;
    const T lc = SAMPLE ? T(0) : a.loc[row * a.C + c];
    const T gb = a.gvec[b];
    const PackT* __restrict__ in = reinterpret_cast<const PackT*>(a.in) + r * pv;
    const PackT* __restrict__ gz = reinterpret_cast<const PackT*>(a.gz) + r * pv;
    PackT* __restrict__ out = reinterpret_cast<PackT*>(a.out) + r * pv;
    T s1 = 0, s2 = 0;
    for (int v = g; v < pv; v += a.G) {
      const PackT x = in[v];
      PackT o;
      if (SAMPLE) {
        const PackT gzv = gz[v];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          o.v[j] = gzv.v[j] * sc - gb * x.v[j];
          s1 += gzv.v[j];
          s2 += gzv.v[j] * sc * x.v[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T u = (x.v[j] - lc) * inv;
          const T t = gb * u * inv;
          o.v[j] = -t;
          s1 += t;
          s2 += u * u;
        }
      }
      if (bad) {
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[j] = T(NAN);
      }
      out[v] = o;
    }
    s1 = lanes_sum_descending(s1, a.G);
    s2 = lanes_sum_descending(s2, a.G);
    if (g == 0) {
      const T dls = SAMPLE ? s2 - T(a.P) * gb : gb * (s2 - T(a.P));
      a.d_loc[r] = bad ? T(NAN) : s1;
      a.d_ls[r] = bad ? T(NAN) : dls;
    }
  }
}

// flat rows (P == 1, C % V == 0): every element is its own channel, a lane owns a pack of V channels
template <typename T, int V, bool SAMPLE>
__global__ __launch_bounds__(kBlock) void cc_gaussian_bwd_flat_kernel(const BwdArgs<T> a) {
  using PackT = Pack<T, V>;
  const int cv = a.C / V;
  const long long packs = a.B * cv;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < packs; e += (long long)gridDim.x * kBlock) {
    const long long b = e / cv;
    const int v = (int)(e - b * cv);
    bool bad;
    const long long row = pick_row(a.idx, a.R, b, bad);
    const PackT s = reinterpret_cast<const PackT*>(a.ls + row * a.C)[v];
    const T gb = a.gvec[b];
    const PackT x = reinterpret_cast<const PackT*>(a.in)[e];
    PackT o, dl, ds;
    if (SAMPLE) {
      const PackT gzv = reinterpret_cast<const PackT*>(a.gz)[e];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const T sc = exp_(s.v[j] + a.log_temp);
        o.v[j] = gzv.v[j] * sc - gb * x.v[j];
        dl.v[j] = gzv.v[j];
        ds.v[j] = gzv.v[j] * sc * x.v[j] - gb;
      }
    } else {
      const PackT l = reinterpret_cast<const PackT*>(a.loc + row * a.C)[v];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const T inv = T(1) / exp_(s.v[j] + a.log_temp);
        const T u = (x.v[j] - l.v[j]) * inv;
        dl.v[j] = gb * u * inv;
        o.v[j] = -dl.v[j];
        ds.v[j] = gb * (u * u - T(1));
      }
    }
    if (bad) {
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = dl.v[j] = ds.v[j] = T(NAN);
    }
    reinterpret_cast<PackT*>(a.out)[e] = o;
    reinterpret_cast<PackT*>(a.d_loc)[e] = dl;
    reinterpret_cast<PackT*>(a.d_ls)[e] = ds;
  }
}

// ------------------------------------------------------------------ per-sample gradients onto the table rows
// out[r, c] = sum over the samples b with idx[b] == r of rows[b, c].  Block (c tile of 64 columns, table row r): a lane
// owns a column, wave w takes the samples b = w (mod kReduceWaves) in ascending order, the partials of the waves are
// added in wave order.  Only the matching rows are read, so rows[] is read once over the whole grid.
template <typename T>
struct ReduceArgs {
  const T* rows;
  const int32_t* idx;
  T* out;
  long long B;
  int C;
};

template <typename T>
__global__ __launch_bounds__(64 * kReduceWaves) void cc_gaussian_reduce_rows_kernel(const ReduceArgs<T> a) {
  __shared__ T part[kReduceWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int r = blockIdx.y;
  T acc = 0;
  for (long long b0 = (long long)w * 64; b0 < a.B; b0 += 64 * kReduceWaves) {
    const int mine = (b0 + lane < a.B) ? a.idx[b0 + lane] : -1;      // 64 labels per load, one per lane
    const int n = (int)((a.B - b0 < 64) ? a.B - b0 : 64);
    for (int j = 0; j < n; ++j)
      if (__shfl(mine, j, 64) == r && c < a.C) acc += a.rows[(b0 + j) * a.C + c];
  }
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && c < a.C) {
    T s = part[0][lane];
    for (int k = 1; k < kReduceWaves; ++k) s += part[k][lane];
    a.out[(long long)r * a.C + c] = s;
  }
}

static int check_shape(int64_t batch, int32_t C, int32_t P, int64_t R, const int32_t* idx) {
  if (batch < 0 || C < 1 || P < 1 || R < 1 || (long long)C * P > (1LL << 30)) return VCNF_ERR_SHAPE;
  if (!idx && R != 1 && R != batch && batch != 0) return VCNF_ERR_SHAPE;
  return VCNF_OK;
}

template <typename T>
static int forward(const T* in, const T* loc, const T* ls, const int32_t* idx, T log_temp, T* z, T* logp, int64_t batch,
                   int32_t C, int32_t P, int64_t R, int ld_mode, T ld_sign, int sample, void* stream) {
  constexpr int V = 16 / sizeof(T);
  if (const int st = check_shape(batch, C, P, R, idx)) return st;
  if (!ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!in || !loc || !ls || !logp || (sample && !z)) return VCNF_ERR_NULL;
  if (!all_aligned({in, loc, ls, logp, z}, sizeof(T)) || !aligned(idx, 4)) return VCNF_ERR_ALIGN;
  const long long d = (long long)C * P;
  FwdArgs<T> a{in, loc, ls, idx, z, logp, batch, R, C, P, 1, ld_mode, sample,
               log_temp, ld_sign, (T)(-0.5 * (double)d * log(2.0 * M_PI))};
  hipStream_t st = (hipStream_t)stream;
  const bool io16 = aligned(in, 16) && aligned(z, 16);
  if (io16 && P % V == 0) {
    a.G = pick_lanes(d / V);
    hipLaunchKernelGGL((cc_gaussian_fwd_kernel<T, V, false>), grid_for(batch, a.G), dim3(kBlock), 0, st, a);
  } else if (io16 && P == 1 && C % V == 0 && aligned(loc, 16) && aligned(ls, 16)) {
    a.G = pick_lanes(d / V);
    hipLaunchKernelGGL((cc_gaussian_fwd_kernel<T, V, true>), grid_for(batch, a.G), dim3(kBlock), 0, st, a);
  } else {
    a.G = pick_lanes(d);
    hipLaunchKernelGGL((cc_gaussian_fwd_kernel<T, 1, false>), grid_for(batch, a.G), dim3(kBlock), 0, st, a);
  }
  return launched();
}

template <typename T, bool SAMPLE>
static int backward(const T* in, const T* gz, const T* loc, const T* ls, const int32_t* idx, T log_temp, const T* gvec,
                    T* out, T* d_loc, T* d_ls, int64_t batch, int32_t C, int32_t P, int64_t R, void* stream) {
  constexpr int V = 16 / sizeof(T);
  if (const int st = check_shape(batch, C, P, R, idx)) return st;
  if (batch == 0) return VCNF_OK;
  if (!in || (SAMPLE ? !gz : !loc) || !ls || !gvec || !out || !d_loc || !d_ls) return VCNF_ERR_NULL;
  if (!all_aligned({in, gz, loc, ls, gvec, out, d_loc, d_ls}, sizeof(T)) || !aligned(idx, 4)) return VCNF_ERR_ALIGN;
  BwdArgs<T> a{in, gz, loc, ls, gvec, idx, out, d_loc, d_ls, batch, R, C, P, 1, log_temp};
  hipStream_t st = (hipStream_t)stream;
  const bool io16 = aligned(in, 16) && aligned(gz, 16) && aligned(out, 16);
  if (io16 && P % V == 0) {
    a.G = pick_lanes(P / V);
    hipLaunchKernelGGL((cc_gaussian_bwd_kernel<T, V, SAMPLE>), grid_for(batch * C, a.G), dim3(kBlock), 0, st, a);
  } else if (io16 && P == 1 && C % V == 0 && aligned(loc, 16) && aligned(ls, 16) && aligned(d_loc, 16) && aligned(d_ls, 16)) {
    hipLaunchKernelGGL((cc_gaussian_bwd_flat_kernel<T, V, SAMPLE>), grid_for(batch * (C / V), 1), dim3(kBlock), 0, st, a);
  } else if (P == 1) {
    hipLaunchKernelGGL((cc_gaussian_bwd_flat_kernel<T, 1, SAMPLE>), grid_for(batch * C, 1), dim3(kBlock), 0, st, a);
  } else {
    a.G = pick_lanes(P);
    hipLaunchKernelGGL((cc_gaussian_bwd_kernel<T, 1, SAMPLE>), grid_for(batch * C, a.G), dim3(kBlock), 0, st, a);
  }
  return launched();
}

template <typename T>
static int reduce_rows(const T* per_sample, const int32_t* idx, T* out, int64_t batch, int32_t C, int64_t R, void* stream) {
  if (batch < 0 || C < 1 || R < 1 || R > 65535) return VCNF_ERR_SHAPE;
  if (!per_sample || !idx || !out) return VCNF_ERR_NULL;
  if (!all_aligned({per_sample, out}, sizeof(T)) || !aligned(idx, 4)) return VCNF_ERR_ALIGN;
  ReduceArgs<T> a{per_sample, idx, out, batch, C};
  hipLaunchKernelGGL(cc_gaussian_reduce_rows_kernel<T>, dim3((unsigned)((C + 63) / 64), (unsigned)R),
                     dim3(64 * kReduceWaves), 0, (hipStream_t)stream, a);
  return launched();
}

}  // namespace vcnf_cc

using namespace vcnf_cc;

#define VCNF_CC_ENTRY_POINTS(T, SFX)                                                                                   \
  extern "C" int vcnf_cc_gaussian_log_prob_##SFX(const T* z, const T* loc_rows, const T* log_scale_rows,               \
                                                 const int32_t* row_index, T log_temperature, T* logp, int64_t batch,  \
                                                 int32_t channels, int32_t pixels, int64_t rows, int ld_mode,          \
                                                 T ld_sign, void* stream) {                                            \
    return forward<T>(z, loc_rows, log_scale_rows, row_index, log_temperature, nullptr, logp, batch, channels, pixels, \
                      rows, ld_mode, ld_sign, 0, stream);                                                              \
  }                                                                                                                    \
  extern "C" int vcnf_cc_gaussian_sample_##SFX(const T* eps, const T* loc_rows, const T* log_scale_rows,               \
                                               const int32_t* row_index, T log_temperature, T* z, T* logp,             \
                                               int64_t batch, int32_t channels, int32_t pixels, int64_t rows,          \
                                               void* stream) {                                                         \
    return forward<T>(eps, loc_rows, log_scale_rows, row_index, log_temperature, z, logp, batch, channels, pixels,     \
                      rows, VCNF_LD_STORE, T(1), 1, stream);                                                           \
  }                                                                                                                    \
  extern "C" int vcnf_cc_gaussian_log_prob_bwd_##SFX(const T* z, const T* loc_rows, const T* log_scale_rows,           \
                                                     const int32_t* row_index, T log_temperature, const T* g, T* dz,   \
                                                     T* d_loc, T* d_log_scale, int64_t batch, int32_t channels,        \
                                                     int32_t pixels, int64_t rows, void* stream) {                     \
    return backward<T, false>(z, nullptr, loc_rows, log_scale_rows, row_index, log_temperature, g, dz, d_loc,          \
                              d_log_scale, batch, channels, pixels, rows, stream);                                     \
  }                                                                                                                    \
  extern "C" int vcnf_cc_gaussian_sample_bwd_##SFX(const T* eps, const T* log_scale_rows, const int32_t* row_index,    \
                                                   T log_temperature, const T* g_z, const T* g_logp, T* d_eps,         \
                                                   T* d_loc, T* d_log_scale, int64_t batch, int32_t channels,          \
                                                   int32_t pixels, int64_t rows, void* stream) {                       \
    return backward<T, true>(eps, g_z, nullptr, log_scale_rows, row_index, log_temperature, g_logp, d_eps, d_loc,      \
                             d_log_scale, batch, channels, pixels, rows, stream);                                      \
  }                                                                                                                    \
  extern "C" int vcnf_cc_gaussian_reduce_rows_##SFX(const T* per_sample, const int32_t* row_index, T* out_rows,        \
                                                    int64_t batch, int32_t channels, int64_t rows, void* stream) {     \
    return reduce_rows<T>(per_sample, row_index, out_rows, batch, channels, rows, stream);                             \
  }

VCNF_CC_ENTRY_POINTS(float, f32)
VCNF_CC_ENTRY_POINTS(double, f64)
