// A run of Planar and Radial layers (normflow/flows/planar.py, radial.py) in ONE launch for MI355X (gfx950, wave64),
// fp32 and fp64 from one template.  Written in torch a layer is a dozen launches of a microsecond of work each, and
// 16 - 64 of them are stacked at 1024 - 2048 samples per call: the evaluation is launch-bound.
//
// The kernels take EFFECTIVE operands, one row per layer in the order the layers are applied (no parameter formula
// lives here: the caller builds them with a fixed number of batched torch ops and autograd carries the gradients of
// the operands on to the parameters):
//   kind [K]     0 planar tanh, 1 planar leaky_relu, 2 radial
//   va   [K, D]  planar: u_hat = u + (log(1 + exp(w.u)) - 1 - w.u) w / |w|^2      radial: z_0
//   vb   [K, D]  planar: w                                                         radial: not read
//   sc   [K, 2]  planar: (b, negative slope)                                       radial: (|alpha|, beta_eff)
// Forward, per layer and sample (sums over the D features):
//   planar   lin = w.z + b,  z' = z + u_hat h(lin),  log|det| = log|1 + (w.u_hat) h'(lin)|
//   radial   r = |z - z_0|,  h = beta / (|alpha| + r),  h' = -beta r / (|alpha| + r)^2,  z' = z + h (z - z_0),
//            log|det| = (D - 1) log(1 + h) + log(1 + h + h')
//   inverse (every kind 1):  lin = w.z + b,  a = 1 or the slope where lin < 0,  s = a (w.u_hat),
//            z' = z - a u_hat lin / (1 + s),  log|det| = -log|1 + s|
//
// Work split: a group of G <= 64 lanes (a power of two, a function of D alone) owns a sample and lane g the kLaneEl
// consecutive features from kLaneEl g of its row, moved in packs of up to 16 bytes.  The row is read once, stays in
// the lane's registers from the first layer to the last and is written once; the dot product and the norm are shuffle
// butterflies inside the group.  The operand rows are read through the caches one layer ahead of their use, so K has
// no limit and nothing depends on K (2 D + 2) values fitting anywhere.  The optional trace [K, B] holds lin (planar)
// or r (radial); the optional checkpoints hold the row as it enters the layers C, 2 C, ... with C = max(ceil(D / 8), 4),
// which is (K - 1) / C rows of D, at most 8 K elements, per sample: with the trace and the output that is all the VJP
// needs, O(B K + B D).
//
// VJP: one launch walks the layers from last to first and rebuilds each layer's input from its output and the trace:
// z = z' - u_hat h(lin) for a planar layer, and z = z_0 + r (z' - z_0) / |z' - z_0| for a radial one, which is
// z_0 + (z' - z_0) / (1 + h(r)) with the traced r as its length (so the rebuilt row is exact along the one direction
// the layer moves it in, whatever the rounding of z').  Across the direction a contracting radial layer still
// multiplies the error of z' by 1 / (1 + h) > 1, at every layer, and a run of leaky_relu layers whose rows grow
// carries the rounding of its large last rows back to its small first ones: both showed in the fp32 gradients of 33
// layers (radial at D <= 5, leaky_relu at D >= 64), so the walk takes the row from a checkpoint wherever one was
// stored and rebuilds at most C - 1 layers in a row.
// Workgroup k takes the sample tiles k, k + groups, ...; per layer the tile's parameter terms are summed over the lane
// groups of a wave (butterfly), over the waves through LDS in ascending order, and added to the workgroup's own block
// [K, 2 D + 2] of the workspace; a second launch (reduce_partials) adds the blocks in a fixed order.  No atomics: the
// same call twice gives the same bits.
#include "stream_common.hpp"

namespace vcnf_pr {

using namespace vcnf_stream;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kLaneEl = 4;                    // features of a row a lane owns
constexpr int kMaxD = 64 * kLaneEl;           // the row lives in the registers of one lane group: D <= 256
constexpr int kMaxFwdBlocks = 4096;
constexpr long long kMaxWsElems = 1LL << 22;  // elements of the VJP's workspace (while one block per K fits)
constexpr long long kMaxBwdGroups = 1024;

enum { kTanh = VCNF_PLANAR_TANH, kLeaky = VCNF_PLANAR_LEAKY, kRadial = VCNF_RADIAL };

__device__ __forceinline__ float tanh_(float v) { return tanhf(v); }
__device__ __forceinline__ double tanh_(double v) { return tanh(v); }
__device__ __forceinline__ float cosh_(float v) { return coshf(v); }
__device__ __forceinline__ double cosh_(double v) { return cosh(v); }

// ------------------------------------------------------------------ a lane's part of a row
template <typename T>
struct Row {
  T v[kLaneEl];
};

template <typename T>
__device__ __forceinline__ Row<T> zero_row() {
  Row<T> r;
#pragma unroll
  for (int j = 0; j < kLaneEl; ++j) r.v[j] = T(0);
  return r;
}

// the features e0 .. e0 + kLaneEl - 1 of the row at p; features >= D are zero (D % V == 0, e0 % kLaneEl == 0: a pack is
// inside the row or outside it)
template <typename T, int V>
__device__ __forceinline__ Row<T> load_row(const T* __restrict__ p, int e0, int D) {
  Row<T> r;
#pragma unroll
  for (int c = 0; c < kLaneEl; c += V) {
    if (e0 + c < D) {
      const Pack<T, V> x = *reinterpret_cast<const Pack<T, V>*>(p + e0 + c);
#pragma unroll
      for (int j = 0; j < V; ++j) r.v[c + j] = x.v[j];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) r.v[c + j] = T(0);
    }
  }
  return r;
}

template <typename T, int V>
__device__ __forceinline__ void store_row(T* __restrict__ p, int e0, int D, const Row<T>& r) {
#pragma unroll
  for (int c = 0; c < kLaneEl; c += V) {
    if (e0 + c < D) {
      Pack<T, V> x;
#pragma unroll
      for (int j = 0; j < V; ++j) x.v[j] = r.v[c + j];
      *reinterpret_cast<Pack<T, V>*>(p + e0 + c) = x;
    }
  }
}

template <typename T>
__device__ __forceinline__ T dot(const Row<T>& x, const Row<T>& y) {
  T s = T(0);
#pragma unroll
  for (int j = 0; j < kLaneEl; ++j) s += x.v[j] * y.v[j];
  return s;
}

// ------------------------------------------------------------------ layer operands
template <typename T>
struct Operands {
  const int* kind;
  const T *va, *vb, *sc;
};

template <typename T>
struct Layer {
  Row<T> a, w;             // u_hat | z_0, w
  T s0, s1;                // (b, slope) | (|alpha|, beta_eff)
  int kind;
};

template <typename T, int V>
__device__ __forceinline__ Layer<T> load_layer(const Operands<T>& o, int k, int e0, int D) {
  Layer<T> l;
  l.kind = o.kind[k];
  l.a = load_row<T, V>(o.va + (long long)k * D, e0, D);
  l.w = l.kind == kRadial ? zero_row<T>() : load_row<T, V>(o.vb + (long long)k * D, e0, D);
  l.s0 = o.sc[2LL * k];
  l.s1 = o.sc[2LL * k + 1];
  return l;
}

// h, h' and h'' of a planar layer at lin
template <typename T>
__device__ __forceinline__ void activation(int kind, T lin, T slope, T& h, T& hp, T& hpp) {
  if (kind == kTanh) {
    const T c = cosh_(lin);
    h = tanh_(lin);
    hp = T(1) / (c * c);
    hpp = T(-2) * h * hp;
  } else {
    hp = lin < T(0) ? slope : T(1);
    h = hp * lin;
    hpp = T(0);
  }
}

// ------------------------------------------------------------------ forward / inverse
template <typename T>
struct FwdArgs {
  Operands<T> o;
  const T* z;
  T *out, *logdet, *trace, *ckpt;
  long long B;
  int D, K, G, every, ld_mode;
  T sign;
};

template <typename T, int V, bool INV>
__global__ __launch_bounds__(kBlock) void pr_fwd_kernel(const FwdArgs<T> a) {
  const int D = a.D, K = a.K, G = a.G, g = threadIdx.x & (G - 1), e0 = g * kLaneEl, per_block = kBlock / G;
  for (long long b = (long long)blockIdx.x * per_block + threadIdx.x / G; b < a.B; b += (long long)gridDim.x * per_block) {
    Row<T> z = load_row<T, V>(a.z + b * D, e0, D);
    T ld = T(0);
    Layer<T> cur = load_layer<T, V>(a.o, 0, e0, D);
    for (int k = 0; k < K; ++k) {
      const Layer<T> nxt = load_layer<T, V>(a.o, k + 1 < K ? k + 1 : k, e0, D);      // one layer ahead of its use
      T tr;
      if (INV) {
        const T lin = lanes_sum(dot(cur.w, z), 1, G) + cur.s0;
        const T al = lin < T(0) ? cur.s1 : T(1);
        const T s = al * lanes_sum(dot(cur.w, cur.a), 1, G);
        const T f = al * lin / (T(1) + s);
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) z.v[j] -= cur.a.v[j] * f;
        ld -= log_(abs_(T(1) + s));
        tr = lin;
      } else if (cur.kind != kRadial) {
        const T lin = lanes_sum(dot(cur.w, z), 1, G) + cur.s0;
        const T s = lanes_sum(dot(cur.w, cur.a), 1, G);
        T h, hp, hpp;
        activation(cur.kind, lin, cur.s1, h, hp, hpp);
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) z.v[j] += cur.a.v[j] * h;
        ld += log_(abs_(T(1) + s * hp));
        tr = lin;
      } else {
        Row<T> dz;
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) dz.v[j] = z.v[j] - cur.a.v[j];
        const T r = sqrt_(lanes_sum(dot(dz, dz), 1, G));
        const T u = cur.s0 + r;
        const T h = cur.s1 / u;
        const T hp = -cur.s1 * r / (u * u);
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) z.v[j] += h * dz.v[j];
        ld += T(D - 1) * log_(T(1) + h) + log_(T(1) + h + hp);
        tr = r;
      }
      if (a.trace && g == 0) a.trace[(long long)k * a.B + b] = tr;
      if (a.ckpt && k + 1 < K && (k + 1) % a.every == 0)
        store_row<T, V>(a.ckpt + ((long long)((k + 1) / a.every - 1) * a.B + b) * D, e0, D, z);
      cur = nxt;
    }
    store_row<T, V>(a.out + b * D, e0, D, z);
    if (g == 0) put_ld(a.logdet, b, a.sign * ld, a.ld_mode);
  }
}

// ------------------------------------------------------------------ the VJP
template <typename T>
struct BwdArgs {
  Operands<T> o;
  const T *zout, *trace, *ckpt, *gout, *gld;
  T *gin, *partials;
  long long B, tiles;
  int D, K, G, every;
};

template <typename T, int V>
__global__ __launch_bounds__(kBlock) void pr_bwd_kernel(const BwdArgs<T> a) {
  __shared__ T red[2][kWaves][2 * kMaxD + 2];
  const int D = a.D, K = a.K, G = a.G, g = threadIdx.x & (G - 1), e0 = g * kLaneEl, per_block = kBlock / G;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = 2 * D + 2;
  T* const block = a.partials + (long long)blockIdx.x * K * n;
  int it = 0;                                          // layers visited: its parity picks the LDS buffer
  bool first = true;
  // every lane of the workgroup walks every tile (barriers inside); a lane group past the batch runs along on zeros
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x, first = false) {
    const long long b = tile * per_block + threadIdx.x / G;
    const bool live = b < a.B;
    Row<T> z = live ? load_row<T, V>(a.zout + b * D, e0, D) : zero_row<T>();
    Row<T> gz = (live && a.gout) ? load_row<T, V>(a.gout + b * D, e0, D) : zero_row<T>();
    const T gl = (live && a.gld) ? a.gld[b] : T(0);
    for (int k = K - 1; k >= 0; --k, ++it) {
      const Layer<T> l = load_layer<T, V>(a.o, k, e0, D);
      const T t = live ? a.trace[(long long)k * a.B + b] : T(0);
      const bool stored = a.ckpt && k > 0 && k % a.every == 0;       // the layer's input is a checkpoint
      Row<T> in = zero_row<T>();
      if (stored && live) in = load_row<T, V>(a.ckpt + ((long long)(k / a.every - 1) * a.B + b) * D, e0, D);
      Row<T> ga, gw;                                   // this sample's terms of d va[k], d vb[k]
      T gs0, gs1;                                      // and of d sc[k]
      if (l.kind != kRadial) {
        T h, hp, hpp;
        activation(l.kind, t, l.s1, h, hp, hpp);
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) z.v[j] = stored ? in.v[j] : z.v[j] - l.a.v[j] * h;          // the layer's input
        const T s = lanes_sum(dot(l.w, l.a), 1, G);
        const T gu = lanes_sum(dot(gz, l.a), 1, G);
        const T q = T(1) + s * hp;
        const T c = gl * hp / q;
        const T glin = gu * hp + gl * (s / q) * hpp;
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) {
          ga.v[j] = h * gz.v[j] + c * l.w.v[j];
          gw.v[j] = glin * z.v[j] + c * l.a.v[j];
          gz.v[j] += glin * l.w.v[j];
        }
        gs0 = glin;
        gs1 = T(0);
      } else {
        const T r = t, al = l.s0, be = l.s1, u = al + r;
        const T h = be / u, hp = -be * r / (u * u);
        const T m = T(1) + h + hp;                     // = 1 + beta |alpha| / u^2
        Row<T> dz;
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) dz.v[j] = (stored ? in.v[j] : z.v[j]) - l.a.v[j];
        if (!stored) {                                 // z' - z_0 to the length r
          const T len = sqrt_(lanes_sum(dot(dz, dz), 1, G));
          const T sc = len > T(0) ? r / len : T(0);
#pragma unroll
          for (int j = 0; j < kLaneEl; ++j) dz.v[j] *= sc;
        }
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) z.v[j] = l.a.v[j] + dz.v[j];     // the layer's input
        const T gh = lanes_sum(dot(gz, dz), 1, G) + gl * T(D - 1) / (T(1) + h);
        const T gm = gl / m;
        const T u2 = u * u, h_r = -be / u2, m_r = T(-2) * be * al / (u2 * u);
        const T gr = gh * h_r + gm * m_r;
        gs0 = gh * h_r + gm * (be / u2 + m_r);
        gs1 = gh / u + gm * al / u2;
        const T cf = r > T(0) ? gr / r : T(0);         // d r / d z = 0 at r == 0
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) {
          const T gd = h * gz.v[j] + cf * dz.v[j];
          ga.v[j] = -gd;
          gw.v[j] = T(0);
          gz.v[j] += gd;
        }
      }
      if (!live) {
        ga = zero_row<T>();
        gw = zero_row<T>();
        gs0 = gs1 = T(0);
      }
      // over the lane groups of the wave, then over the waves
#pragma unroll
      for (int j = 0; j < kLaneEl; ++j) {
        ga.v[j] = lanes_sum(ga.v[j], G, 64);
        gw.v[j] = lanes_sum(gw.v[j], G, 64);
      }
      gs0 = lanes_sum(gs0, G, 64);
      gs1 = lanes_sum(gs1, G, 64);
      T* const buf = red[it & 1][wave];
      if (lane < G) {
#pragma unroll
        for (int j = 0; j < kLaneEl; ++j) {
          if (e0 + j < D) {
            buf[e0 + j] = ga.v[j];
            buf[D + e0 + j] = gw.v[j];
          }
        }
        if (g == 0) {
          buf[2 * D] = gs0;
          buf[2 * D + 1] = gs1;
        }
      }
      __syncthreads();
      for (int e = threadIdx.x; e < n; e += kBlock) {
        T s = red[it & 1][0][e];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += red[it & 1][w][e];
        T* const dst = block + (long long)k * n + e;
        *dst = first ? s : *dst + s;
      }
    }
    if (live) store_row<T, V>(a.gin + b * D, e0, D, gz);
  }
}

// element e of the summed block [K, 2 D + 2] goes to g_va [K, D] | g_vb [K, D] | g_sc [K, 2]
template <typename T>
struct LayerDest {
  T *va, *vb, *sc;
  int D;
  __device__ T* operator()(long long e) const {
    const long long n = 2LL * D + 2, k = e / n;
    const int j = (int)(e - k * n);
    return j < D ? va + k * D + j : j < 2 * D ? vb + k * D + (j - D) : sc + 2 * k + (j - 2 * D);
  }
};

// ------------------------------------------------------------------ host side
static inline bool supported(int32_t D) { return D >= 1 && D <= kMaxD; }
static inline int lanes_for(int32_t D) { return pick_lanes((D + kLaneEl - 1) / kLaneEl); }
// a checkpoint of the row every so many layers: (K - 1) / every rows of D per sample, at most 8 K elements
static inline int checkpoint_every(int32_t D) { return D > 32 ? (D + 7) / 8 : 4; }

static int check_shape(int64_t batch, int32_t D, int32_t K) {
  return batch < 0 || !supported(D) || K < 1 ? VCNF_ERR_SHAPE : VCNF_OK;
}

// kinds known, and all leaky_relu for the inverse; *planar: some layer reads vb
static bool ok_kinds(const int32_t* kind, int32_t K, bool inverse, bool* planar) {
  *planar = false;
  for (int32_t k = 0; k < K; ++k) {
    if (kind[k] < kTanh || kind[k] > kRadial || (inverse && kind[k] != kLeaky)) return false;
    *planar |= kind[k] != kRadial;
  }
  return true;
}

static long long sample_tiles(int64_t batch, int32_t D) {
  const long long per_block = kBlock / lanes_for(D);
  return (batch + per_block - 1) / per_block;
}

// workgroups = partial blocks of the VJP: a pure function of the shape
static long long bwd_groups(int64_t batch, int32_t D, int32_t K) {
  long long cap = kMaxWsElems / ((long long)K * (2LL * D + 2));
  cap = cap < 1 ? 1 : cap > kMaxBwdGroups ? kMaxBwdGroups : cap;
  const long long n = sample_tiles(batch, D);
  return n < 1 ? 1 : n > cap ? cap : n;
}

template <typename T>
static int forward(const T* z, T* out, T* logdet, T* trace, T* ckpt, const int32_t* kind, const int32_t* kind_dev, const T* va,
                   const T* vb, const T* sc, int64_t batch, int32_t D, int32_t K, int inverse, int ld_mode, T sign,
                   void* stream) {
  if (const int st = check_shape(batch, D, K)) return st;
  if (!kind) return VCNF_ERR_NULL;
  bool planar;
  if (!ok_kinds(kind, K, inverse != 0, &planar) || !ok_ld(ld_mode)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!z || !out || !logdet || !kind_dev || !va || !sc || (planar && !vb)) return VCNF_ERR_NULL;
  if (!all_aligned({z, out, logdet, trace, ckpt, va, vb, sc}, sizeof(T)) || !aligned(kind_dev, sizeof(int32_t)))
    return VCNF_ERR_ALIGN;
  const FwdArgs<T> a{Operands<T>{kind_dev, va, vb, sc}, z, out, logdet, trace, ckpt, batch, D, K, lanes_for(D),
                     checkpoint_every(D), ld_mode, sign};
  const dim3 grid = grid_for(batch, a.G, kBlock, kMaxFwdBlocks);
  return with_pack<T>(D, {z, out, ckpt, va, vb}, [&](auto V) {
    return with_flags([&](auto INVERSE) {
      hipLaunchKernelGGL((pr_fwd_kernel<T, V(), INVERSE()>), grid, dim3(kBlock), 0, (hipStream_t)stream, a);
      return launched();
    }, inverse != 0);
  });
}

template <typename T>
static int backward(const T* zout, const T* trace, const T* ckpt, const T* gout, const T* gld, const int32_t* kind, const int32_t* kind_dev,
                    const T* va, const T* vb, const T* sc, T* gin, T* g_va, T* g_vb, T* g_sc, T* workspace, int64_t batch,
                    int32_t D, int32_t K, void* stream) {
  if (const int st = check_shape(batch, D, K)) return st;
  if (!kind) return VCNF_ERR_NULL;
  bool planar;
  if (!ok_kinds(kind, K, false, &planar)) return VCNF_ERR_UNSUPPORTED;
  if (batch == 0) return VCNF_OK;
  if (!zout || !trace || !kind_dev || !va || !sc || (planar && !vb) || !gin || !g_va || !g_vb || !g_sc || !workspace)
    return VCNF_ERR_NULL;
  if (!all_aligned({zout, trace, ckpt, gout, gld, va, vb, sc, gin, g_va, g_vb, g_sc, workspace}, sizeof(T)) ||
      !aligned(kind_dev, sizeof(int32_t)))
    return VCNF_ERR_ALIGN;
  const BwdArgs<T> a{Operands<T>{kind_dev, va, vb, sc}, zout, trace, ckpt, gout, gld, gin, workspace, batch,
                     sample_tiles(batch, D), D, K, lanes_for(D), checkpoint_every(D)};
  const dim3 grid((unsigned)bwd_groups(batch, D, K));
  const int rc = with_pack<T>(D, {zout, ckpt, gout, gin, va, vb}, [&](auto V) {
    hipLaunchKernelGGL((pr_bwd_kernel<T, V()>), grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    return launched();
  });
  if (rc) return rc;
  return launch_reduce_partials(workspace, bwd_groups(batch, D, K), (long long)K * (2LL * D + 2),
                                LayerDest<T>{g_va, g_vb, g_sc, D}, stream);
}

}  // namespace vcnf_pr

using namespace vcnf_pr;

extern "C" int vcnf_planar_radial_supported(int32_t features) { return supported(features) ? 1 : 0; }

extern "C" int32_t vcnf_planar_radial_checkpoint_every(int32_t features) {
  return supported(features) ? checkpoint_every(features) : 0;
}

extern "C" int64_t vcnf_planar_radial_bwd_groups(int64_t batch, int32_t features, int32_t n_layers) {
  if (check_shape(batch, features, n_layers) != VCNF_OK) return 0;
  return bwd_groups(batch, features, n_layers);
}

#define VCNF_PR_ENTRY_POINTS(T, SFX)                                                                                    \
  extern "C" int vcnf_planar_radial_stack_##SFX(const T* z, T* out, T* logdet, T* trace, T* checkpoints,               \
                                                const int32_t* kind, const int32_t* kind_dev, const T* va,             \
                                                const T* vb, const T* sc, int64_t batch, int32_t features,             \
                                                int32_t n_layers, int inverse, int ld_mode, T ld_sign, void* stream) { \
    return forward<T>(z, out, logdet, trace, checkpoints, kind, kind_dev, va, vb, sc, batch, features, n_layers,       \
                      inverse, ld_mode, ld_sign, stream);                                                              \
  }                                                                                                                    \
  extern "C" int vcnf_planar_radial_stack_bwd_##SFX(const T* z_out, const T* trace, const T* checkpoints,              \
                                                    const T* g_out, const T* g_logdet, const int32_t* kind,            \
                                                    const int32_t* kind_dev, const T* va, const T* vb, const T* sc,    \
                                                    T* g_in, T* g_va, T* g_vb, T* g_sc, T* workspace, int64_t batch,   \
                                                    int32_t features, int32_t n_layers, void* stream) {                \
    return backward<T>(z_out, trace, checkpoints, g_out, g_logdet, kind, kind_dev, va, vb, sc, g_in, g_va, g_vb, g_sc, \
                       workspace, batch, features, n_layers, stream);                                                  \
  }

VCNF_PR_ENTRY_POINTS(float, f32)
VCNF_PR_ENTRY_POINTS(double, f64)
