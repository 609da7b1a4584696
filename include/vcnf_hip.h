/*
 * vcnf_hip.h - C ABI of the MI355X (gfx950) coupling-flow transform engine.
 *
 * The reference (telegraphroad/VCNF, a fork of normflow 1.2) is pure Python: it
 * has no FFI.  Its hot path sits behind Python classes
 * (normflow/flows/base.py:6-21, Flow.forward / Flow.inverse).  This header is
 * the boundary a binding for that path attaches to: every entry point replaces
 * the arithmetic of the reference function cited above it, on device buffers
 * the caller owns.  Conventions shared by all entry points:
 *
 *   - plain pointers + sizes, fp32 row-major dense buffers in HBM, int32 index
 *     vectors on the device; no allocation, no host sync, no host callbacks;
 *   - `stream` is a hipStream_t (NULL = default stream); the call only enqueues;
 *   - return value: VCNF_OK or a VCNF_ERR_* code (vcnf_status_string());
 *     arguments are validated on the host BEFORE anything is launched;
 *   - `logdet` handling: ld_mode VCNF_LD_STORE writes sign*sum, VCNF_LD_ACCUM
 *     adds sign*sum to what is there (the `log_q += / -= log_det` of
 *     normflow/core.py:153-155, :179-181 folded into the kernel);
 *   - direction names follow the reference's nsf code: `inverse == 0` is the
 *     density direction of a spline (search x knots), `inverse != 0` the
 *     sampling direction (search y knots, quadratic root).
 *
 * See INTEGRATION.md for the ctypes binding that ships in vcnf_amd/_lib.py.
 */
#ifndef VCNF_HIP_H
#define VCNF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VCNF_ABI_VERSION 1

enum {
  VCNF_OK = 0,
  VCNF_ERR_NULL = 1,        /* a required pointer is NULL */
  VCNF_ERR_SHAPE = 2,       /* sizes inconsistent / out of the supported range */
  VCNF_ERR_ALIGN = 3,       /* a buffer is not 4-byte aligned */
  VCNF_ERR_VALUE = 4,       /* e.g. min_bin_width * K > 1 (splines.py:104-107) */
  VCNF_ERR_UNSUPPORTED = 5, /* unknown enum value (tails, scale map) */
  VCNF_ERR_LAUNCH = 6       /* hipGetLastError() after the launch */
};

enum { VCNF_LD_STORE = 0, VCNF_LD_ACCUM = 1 };
enum { VCNF_TAILS_NONE = 0, VCNF_TAILS_LINEAR = 1, VCNF_TAILS_CIRCULAR = 2 };
enum { VCNF_PREC_F32 = 0, VCNF_PREC_F16X3 = 1 };   /* matrix path of the fused layer kernel */
enum { VCNF_SCALE_EXP = 0, VCNF_SCALE_SIGMOID = 1, VCNF_SCALE_SIGMOID_INV = 2, VCNF_SCALE_NONE = 3 };

int vcnf_abi_version(void);
const char* vcnf_status_string(int status);

/* Spline constants.  Replaces the keyword arguments of
 * unconstrained_rational_quadratic_spline / rational_quadratic_spline
 * (normflow/utils/splines.py:20-29, :88-96). */
typedef struct vcnf_rqs_cfg {
  int32_t num_bins;        /* K */
  int32_t tails;           /* VCNF_TAILS_* ; LINEAR: K-1 derivative logits, identity outside;
                              CIRCULAR: K logits (last knot = first knot, splines.py:44-49), identity outside */
  float left, right;       /* x interval; LINEAR uses [-tail_bound, tail_bound] */
  float bottom, top;       /* y interval */
  float min_bin_width;     /* splines.py:6 */
  float min_bin_height;    /* splines.py:7 */
  float min_derivative;    /* splines.py:8 */
  float wh_scale;          /* multiplies width/height logits: 1/sqrt(hidden_features),
                              flows/neural_spline/coupling.py:314-316; 1 for none */
} vcnf_rqs_cfg;

/* Elementwise spline on n independent elements with per-element parameters.
 * Replaces splines.py:20-85 (tails=LINEAR) and :88-193 (tails=NONE).
 * uw/uh/ud: element i reads uw[i*ld_w + k], k<K; uh[i*ld_h + k]; ud[i*ld_d + k],
 * k < K-1 (LINEAR) or K+1 (NONE).  bad_disc (optional, device int32) counts
 * negative discriminants, the condition the reference asserts on (splines.py:164). */
int vcnf_rqs_elementwise_f32(const float* x, const float* uw, const float* uh, const float* ud,
                             int64_t ld_w, int64_t ld_h, int64_t ld_d,
                             float* y, float* logabsdet, int64_t n,
                             const vcnf_rqs_cfg* cfg, int inverse, int32_t* bad_disc, void* stream);

/* Same spline with general addressing of the logit rows (image-shaped couplings,
 * coupling.py:148-151, and rows shared by the whole batch, coupling.py:211-240):
 *   r = period > 0 ? i % period : i;  outer = r / inner;  s = r % inner;
 *   logit k of element i = u?[outer * row_? + s + k * k_stride].
 * Conditioner output [B, C*P, H, W] of a 4-D coupling: inner = H*W, k_stride = H*W,
 * row_* = P*H*W, uh = uw + K*H*W, ud = uw + 2*K*H*W.  Per-pixel logits [C,H,W,K] shared by
 * the batch: inner = 1, k_stride = 1, row_* = K (K-1 | K | K+1 for ud), period = C*H*W. */
int vcnf_rqs_elementwise_strided_f32(const float* x, const float* uw, const float* uh, const float* ud,
                                     int64_t row_w, int64_t row_h, int64_t row_d, int64_t inner,
                                     int64_t k_stride, int64_t period,
                                     float* y, float* logabsdet, int64_t n,
                                     const vcnf_rqs_cfg* cfg, int inverse, int32_t* bad_discriminant,
                                     void* stream);

/* Interval limits of the functional spline given per element (splines.py:99-102, tensor `left / right / bottom /
 * top`).  Limit j (0 left, 1 right, 2 bottom, 3 top) of element i is lim_j[(i / inner[j]) % period[j]]: a
 * full-shape tensor is period = n, inner = 1; a trailing-shape one ([D] against [B, D]) period = D, inner = 1; a
 * leading one ([B, 1] against [B, D]) period = B, inner = D; a 0-dim one period = inner = 1.  period, inner >= 1. */
typedef struct vcnf_rqs_limit_bcast {
  int64_t period[4];
  int64_t inner[4];
} vcnf_rqs_limit_bcast;

/* vcnf_rqs_elementwise_f32 with per-element limits: the knots of element i are lo + (hi - lo) * c_k with
 * hi - lo evaluated in the working precision (the reference's tensor branch).  cfg->tails must be
 * VCNF_TAILS_NONE (K + 1 derivative logits; the limits in cfg are ignored); inputs outside their interval are
 * evaluated in the nearest edge bin.  K <= 64. */
int vcnf_rqs_elementwise_limits_f32(const float* x, const float* uw, const float* uh, const float* ud,
                                    int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                    const float* left, const float* right, const float* bottom, const float* top,
                                    const vcnf_rqs_limit_bcast* bcast, float* y, float* logabsdet, int64_t n,
                                    const vcnf_rqs_cfg* cfg, int inverse, int32_t* bad_disc, void* stream);

/* VJP of vcnf_rqs_elementwise_limits_f32: the outputs of vcnf_rqs_elementwise_bwd_f32 (dense gradient rows) plus the
 * PER-ELEMENT gradients g_left[n], g_right[n], g_bottom[n], g_top[n] of the limits (the caller reduces them to the
 * limits' own shapes).  A NULL limit gradient is not computed.  K <= 64. */
int vcnf_rqs_elementwise_limits_bwd_f32(const float* x, const float* uw, const float* uh, const float* ud,
                                        int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                        const float* left, const float* right, const float* bottom, const float* top,
                                        const vcnf_rqs_limit_bcast* bcast,
                                        const float* g_y, const float* g_logabsdet,
                                        float* g_x, float* g_uw, float* g_uh, float* g_ud,
                                        float* g_left, float* g_right, float* g_bottom, float* g_top, int64_t n,
                                        const vcnf_rqs_cfg* cfg, int inverse, void* stream);

/* Whole AffineCouplingBlock on x[B, features] in one launch when the conditioner is an MLP with two
 * hidden layers of equal width: Linear(c_in, hidden), LeakyReLU, Linear(hidden, hidden), LeakyReLU,
 * Linear(hidden, n_out), n_out = 2*d_t (interleaved shift, scale) or d_t (scale map NONE).
 * Replaces flows/affine/coupling.py:247-258 with :113-168, reshape.py:25-29, :50-55 and
 * nets/mlp.py:30-58 for that case.  The conditioner reads x[:, cond_off : cond_off + c_in], the
 * features [t_off, t_off + d_t) are transformed, the rest is copied.  hidden in {32, 64, 128},
 * c_in <= 64, n_out <= 128.  wpack: vcnf_affine_layer_fused_pack_floats(...) floats in the
 * fragment order documented in vcnf_amd/fused_affine.py.  in_gather / out_gather (int32[features],
 * may be NULL) fold a neighbouring Permute (flows/mixing.py:32-54) into the layer: the block is
 * applied to x[:, in_gather] and the result returned as result[:, out_gather]. */
int vcnf_affine_layer_fused_supported(int32_t c_in, int32_t hidden, int32_t n_out, int32_t features);
int64_t vcnf_affine_layer_fused_pack_floats(int32_t c_in, int32_t hidden, int32_t n_out);
int vcnf_affine_layer_fused_f32(const float* x, float* y, float* logdet, int64_t batch, int32_t features,
                                int32_t cond_off, int32_t c_in, int32_t t_off, int32_t d_t,
                                int32_t hidden, float leaky_slope, int scale_map,
                                const float* wpack, int64_t wpack_floats,
                                const int32_t* in_gather, const int32_t* out_gather,
                                int inverse, int ld_mode, float ld_sign, void* stream);

/* Per-position splines whose logits are shared by the whole batch (coupling.py:211-240): x [n] with
 * position i % period, logits sw, sh [period, K], sd [period, K-1 | K | K+1].  `tables` is a caller
 * workspace of period * 3 * (K + 1) floats: the knots of every position are generated once into it,
 * the elements then search their row (no softmax per element). */
int vcnf_rqs_shared_f32(const float* x, const float* sw, const float* sh, const float* sd, int64_t period,
                        float* tables, float* y, float* logabsdet, int64_t n,
                        const vcnf_rqs_cfg* cfg, int inverse, int32_t* bad_discriminant, void* stream);

/* Vector-Jacobian product of vcnf_rqs_elementwise_f32 (training path; the reference
 * obtains it from autograd over utils/splines.py:88-193).  Inputs as the forward call
 * plus the upstream gradients g_y[n], g_logabsdet[n]; outputs g_x[n] and dense
 * g_uw[n,K], g_uh[n,K], g_ud[n, K-1 | K+1].  K <= 64. */
int vcnf_rqs_elementwise_bwd_f32(const float* x, const float* uw, const float* uh, const float* ud,
                                 int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                 const float* g_y, const float* g_logabsdet,
                                 float* g_x, float* g_uw, float* g_uh, float* g_ud, int64_t n,
                                 const vcnf_rqs_cfg* cfg, int inverse, void* stream);

/* VJP of the spline with the logits read from (and their gradient written in) the conditioner's
 * own output layout: params / g_params [rows, P, inner] with P = 2K + (K-1 | K | K+1), x [rows*inner]
 * (2-D coupling: inner = 1, rows = B*d_t; image coupling: inner = H*W, rows = B*C_t).  g_logabsdet
 * is read at i / lad_div (per-sample log-det: lad_div = elements per sample). */
int vcnf_rqs_packed_bwd_f32(const float* x, const float* params, int64_t inner, int64_t lad_div,
                            const float* g_y, const float* g_logabsdet,
                            float* g_x, float* g_params, int64_t n,
                            const vcnf_rqs_cfg* cfg, int inverse, void* stream);

/* VJP of the batch-shared spline (coupling.py:211-240): x [batch, period], logits sw, sh [period, K],
 * sd [period, nd].  Writes g_x and `groups` partial gradient rows per position,
 * partial [groups, period, 2K+nd] (sum over the first axis = gradient of the logits, row layout
 * w | h | d); groups must equal vcnf_rqs_shared_bwd_groups(batch, period).  K in {4, 8, 10, 16}. */
int64_t vcnf_rqs_shared_bwd_groups(int64_t batch, int64_t period);
int vcnf_rqs_shared_bwd_f32(const float* x, const float* sw, const float* sh, const float* sd,
                            int64_t batch, int64_t period, int64_t lad_div,
                            const float* g_y, const float* g_logabsdet,
                            float* g_x, float* partial, int64_t groups,
                            const vcnf_rqs_cfg* cfg, int inverse, void* stream);

/* Last conditioner layer + splines of an RQS coupling for any number of transformed features:
 * h [B, hidden] is the conditioner trunk's output (input of nets/resnet.py:105 final_layer), wpack the
 * final layer's weights and bias in matrix-core fragment order (vcnf_amd/fused_final.py).  Writes the
 * transformed columns y[:, transform_idx] (the caller has filled the identity columns) and the
 * per-group-block log|det| rows partial[vcnf_rqs_final_fused_partial_rows(d_t, K), B] whose sum over
 * rows is the transform half's log|det|.  Replaces nets/resnet.py:105, coupling.py:147-159 and
 * :309-343 without materialising the [B, d_t * (3K-1)] logits.  hidden = 128, linear tails, K in {8, 10, 16}. */
int vcnf_rqs_final_fused_supported(int32_t d_t, int32_t hidden, int32_t num_bins, int32_t tails);
int64_t vcnf_rqs_final_fused_pack_floats(int32_t d_t, int32_t hidden, int32_t num_bins);
int64_t vcnf_rqs_final_fused_partial_rows(int32_t d_t, int32_t num_bins);
int vcnf_rqs_final_fused_f32(const float* x, const float* h, float* y, float* partial,
                             int64_t batch, int32_t features, const int32_t* transform_idx, int32_t d_t,
                             int32_t hidden, const float* wpack, int64_t wpack_floats,
                             const vcnf_rqs_cfg* cfg, int inverse, int32_t* bad_discriminant, void* stream);

/* Trunk of a ResidualNet conditioner in one launch: h[B, 128] = everything in front of final_layer
 * (nets/resnet.py:92-105: initial_layer, then per block h += linear_1(relu(linear_0(relu(h)))), ReLU, no batch
 * norm, dropout 0, no context gate) for x[B, d_in] = the (identity | context) input, d_in a multiple of 16,
 * hidden 128, 1-3 blocks; exact fp32 matrix instructions.  Feeds vcnf_rqs_final_fused_f32 (config C5).
 * wpack: vcnf_resnet_trunk_pack_floats floats, every weight matrix as [row block of 16][k block of 16][lane][4]
 * fragments (k = 16 kb + 4 (lane >> 4) + c), biases in natural order (vcnf_amd/fused_final.py::pack_trunk). */
int vcnf_resnet_trunk_supported(int32_t d_in, int32_t hidden, int32_t num_blocks);
int64_t vcnf_resnet_trunk_pack_floats(int32_t d_in, int32_t hidden, int32_t num_blocks);
int vcnf_resnet_trunk_f32(const float* x, float* h, int64_t batch, int32_t d_in, int32_t hidden,
                          int32_t num_blocks, const float* wpack, int64_t wpack_floats, void* stream);

/* The pair with the trunk output handed over already split for the matrix path of the last-layer kernel: row b of
 * h_split (128 floats wide) holds 128 fp16 hi halves followed by 128 fp16 lo halves (h ~ hi + lo / 2048, values clamped
 * at +-65504 and counted in sat_count) - the split then happens once per sample instead of once per sample and
 * feature-group workgroup.  Same results as the fp32 hand-over, bit for bit. */
int vcnf_resnet_trunk_split_f32(const float* x, float* h_split, int64_t batch, int32_t d_in, int32_t hidden,
                                int32_t num_blocks, const float* wpack, int64_t wpack_floats, int32_t* sat_count,
                                void* stream);
int vcnf_rqs_final_fused_presplit_f32(const float* x, const float* h_split, float* y, float* partial,
                                      int64_t batch, int32_t features, const int32_t* transform_idx, int32_t d_t,
                                      int32_t hidden, const float* wpack, int64_t wpack_floats,
                                      const vcnf_rqs_cfg* cfg, int inverse, int32_t* bad_discriminant, void* stream);


/* One RQS coupling layer on x[B,D] -> y[B,D].
 * Replaces Coupling.forward / .inverse (flows/neural_spline/coupling.py:70-96 /
 * :98-125) minus the conditioner call, PiecewiseCoupling._coupling_transform
 * (:147-159), _piecewise_cdf (:309-343), the unconditional per-feature spline
 * (PiecewiseRationalQuadraticCDF._spline :211-240) and sum_except_batch
 * (utils/nn.py:131-134).
 *   params[B, d_t*P] dense, P = 3K-1 (LINEAR) or 3K+1 (NONE): conditioner output.
 *   transform_idx[d_t], identity_idx[d_id]: feature indices (buffers
 *     transform_features / identity_features, coupling.py:45-46), d_t+d_id == D.
 *   shared_w/h[d_id,K], shared_d[d_id, K-1 | K+1]: unconditional spline logits or
 *     all NULL when apply_unconditional_transform is off; never scaled by wh_scale.
 *   logdet[B]: per-sample sum over all D features, see ld_mode / sign above. */
int vcnf_rqs_coupling_f32(const float* x, const float* params,
                          const int32_t* transform_idx, int32_t d_t,
                          const int32_t* identity_idx, int32_t d_id,
                          const float* shared_w, const float* shared_h, const float* shared_d,
                          float* y, float* logdet, int64_t batch,
                          const vcnf_rqs_cfg* cfg, int inverse,
                          int ld_mode, float ld_sign, int32_t* bad_disc, void* stream);

/* Conditioner input for one RQS coupling layer: out[B, d_id + ctx_dim] =
 * cat(identity_split, context).  With apply_inverse_shared != 0 the identity
 * columns first go through the INVERSE unconditional spline, which is what the
 * sampling direction feeds its conditioner (coupling.py:110-114); otherwise the
 * raw gather of coupling.py:78 (and the concat of nets/resnet.py:100-102). */
int vcnf_rqs_conditioner_input_f32(const float* x, int64_t batch, int32_t features,
                                   const int32_t* identity_idx, int32_t d_id,
                                   const float* context, int32_t ctx_dim,
                                   const float* shared_w, const float* shared_h, const float* shared_d,
                                   const vcnf_rqs_cfg* cfg, int apply_inverse_shared,
                                   float* out, void* stream);

/* Per-pixel channel mixing of an image batch: y[b, o, p] = sum_c matrix[o, c] x[b, c, p] + shift[o] for x, y
 * [batch, channels, inner] (NCHW, inner = H W); matrix [channels, channels] row-major and shift [channels] on the device.
 * One launch for Glow's invertible 1x1 convolution (flows/mixing.py:57-128) composed with the neighbouring ActNorm
 * (flows/normalization.py:8-38, flows/affine/coupling.py:37-53); the caller composes matrix / shift from the layer
 * parameters and adds the constant log|det| (vcnf_amd/flows/affine/glow.py).  Exact fp32 products on
 * v_mfma_f32_16x16x4_f32.  channels: multiple of 4, 4..64 (vcnf_channel_mix_supported). */
int vcnf_channel_mix_supported(int32_t channels);
int vcnf_channel_mix_f32(const float* x, float* y, const float* matrix, const float* shift,
                         int64_t batch, int32_t channels, int64_t inner, void* stream);

/* 1x1 convolution of an NCHW batch with the bias adds and LeakyReLUs around it in one pass (nets/cnn.py:20-52, the
 * middle layer of the Glow conditioner flows/affine/glow.py:37-47):
 *   y[b, o, p] = act_out( sum_c W[o, c] * act_in(x[b, c, p] + in_bias[c]) + out_bias[o] ),  act(t) = t >= 0 ? t : slope t
 * x [batch, c_in, inner], y [batch, c_out, inner]; in_bias / out_bias may be NULL; in_act / out_act switch the
 * activations.  The caller runs the preceding convolution without its bias and passes that bias as in_bias.
 * Matrix path: fp16 split-half operands (hi + lo 2^-11, fp32 accumulation, 3 instructions per product); values beyond
 * +-65504 are clamped and counted in sat_count (device int32, may be NULL).  wpack: vcnf_conv1x1_pack_floats(c_in, c_out)
 * floats = W as A fragments of v_mfma_f32_32x32x16_f16, [8 row blocks][c_in / 16][hi | lo][64 lanes][8 halves]
 * (vcnf_amd/nets/cnn.py::pack_conv1x1).  c_in multiple of 16 up to 256, c_out up to 256. */
int vcnf_conv1x1_supported(int32_t c_in, int32_t c_out);
int64_t vcnf_conv1x1_pack_floats(int32_t c_in, int32_t c_out);
int vcnf_conv1x1_f16x3_f32(const float* x, float* y, const float* wpack, int64_t wpack_floats,
                           const float* in_bias, const float* out_bias, int64_t batch, int32_t c_in, int32_t c_out,
                           int64_t inner, int in_act, float in_slope, int out_act, float out_slope,
                           int32_t* sat_count, void* stream);

/* Weight and bias gradient of a dense conditioner layer y = x W^T + b for large batches (training path; the reference
 * gets them from autograd over nets/resnet.py:92-106):  dw[o, i] (+)= sum_b dy[b, o] x[b, i],  db[o] (+)= sum_b dy[b, o]
 * with x [batch, in_features], dy [batch, out_features] row-major; db may be NULL.  The reduction over the batch is
 * split into vcnf_linear_wgrad_slices(...) slices (exact fp32 matrix instructions), whose partial results go through
 * `workspace` (>= slices * (out * in + out) floats) and are added in a fixed order.  accumulate != 0 adds to dw / db.
 * in_features: multiple of 16 up to 128. */
int vcnf_linear_wgrad_supported(int32_t in_features, int32_t out_features);
int64_t vcnf_linear_wgrad_slices(int64_t batch, int32_t in_features, int32_t out_features);
int vcnf_linear_wgrad_f32(const float* x, const float* dy, float* dw, float* db, float* workspace,
                          int64_t workspace_floats, int64_t batch, int32_t in_features, int32_t out_features,
                          int accumulate, void* stream);
/* The same gradients with the partial products on the fp16 split-half matrix path (v_mfma_f32_32x32x16_f16, both
 * operands split in registers, fp32 accumulation; arithmetic of VCNF_PREC_F16X3): the exact-fp32 kernel is bound by
 * its matrix instructions, this one runs the 736-row last layer of config C3 in a third of the time.  Same workspace,
 * same deterministic slice order.  relu_input: the layer's input is relu(x) (applied on load).  dy_amax (may be NULL):
 * [out_features] device floats, the largest |dy[:, o]| of every column (col_amax of vcnf_abs_max_rows_cols_f32) -
 * column o of dy is then multiplied by the power of two that puts that value in [2^14, 2^15) as it is read and row o
 * of dW and db[o] by its inverse as they are written (both exact: 2^-k dy gives 2^-k dW bit for bit), so a cotangent
 * of any magnitude keeps full precision for 2^29 below the largest entry of its column and is not clamped; NULL, or 0
 * or a non-finite value for a column: no scaling (of that column).  Values beyond +-65504 (after the scaling) are
 * clamped and counted in sat_count (may be NULL). */
int vcnf_linear_wgrad_f16x3_f32(const float* x, const float* dy, float* dw, float* db, float* workspace,
                                int64_t workspace_floats, int64_t batch, int32_t in_features,
                                int32_t out_features, int accumulate, int relu_input, const float* dy_amax,
                                int32_t* sat_count, void* stream);
/* Largest |value| of every row (row_amax [rows]) and of every column (col_amax [cols]) of x [rows, cols], left on the
 * device for the x_amax / dy_amax arguments of the split-half training kernels (one launch, one read of x, no host
 * read; graph-capturable); a NaN in a row / column gives NaN there.  cols <= 8192.  scratch: at least
 * vcnf_abs_max_rows_cols_scratch_floats(rows, cols) floats (0: shape not supported), owned by one stream; its first word
 * is zero when first used and left zero by every launch. */
int64_t vcnf_abs_max_rows_cols_scratch_floats(int64_t rows, int32_t cols);
int vcnf_abs_max_rows_cols_f32(const float* x, int64_t rows, int32_t cols, float* row_amax, float* col_amax,
                               float* scratch, int64_t scratch_floats, void* stream);

/* First two layers of the Glow conditioner in one launch (nets/cnn.py:20-52): y = act2(W2 act1(conv3x3(x; W1, padding 1)
 * + b1) + b2) with x [batch, c_in, height, width], 256 hidden and 256 output channels, act = LeakyReLU(slope); the
 * hidden activation between the two layers stays on chip.  Matrix path and saturation counter as
 * vcnf_conv1x1_f16x3_f32.  w1pack: the [256, 9 c_in] patch matrix (k = ci * 9 + ky * 3 + kx, zero padded to a multiple of
 * 16) as A fragments, vcnf_conv3x3_1x1_pack_floats(c_in) floats; w2pack: vcnf_conv1x1_pack_floats(256, 256) floats
 * (vcnf_amd/nets/cnn.py::pack_conv1x1).  c_in <= 24. */
int vcnf_conv3x3_1x1_supported(int32_t c_in, int32_t hidden, int32_t c_out);
int64_t vcnf_conv3x3_1x1_pack_floats(int32_t c_in);
int vcnf_conv3x3_1x1_f16x3_f32(const float* x, float* y, const float* w1pack, int64_t w1pack_floats,
                               const float* w2pack, int64_t w2pack_floats, const float* b1, const float* b2,
                               int64_t batch, int32_t c_in, int32_t height, int32_t width, float slope1, float slope2,
                               int32_t* sat_count, void* stream);

/* The whole Glow conditioner Conv3x3(c_in -> 256), LeakyReLU, Conv1x1(256 -> 256), LeakyReLU, Conv3x3(256 -> c_out)
 * (nets/cnn.py:20-52, flows/affine/glow.py:37-47) in two launches, neither 256-channel activation ever in memory:
 *   vcnf_convnet3_taps_f16x3_f32: the first two layers as vcnf_conv3x3_1x1_f16x3_f32, then the last layer's nine taps as
 *       1x1 convolutions  z[b, t * c_out + o, p] = sum_c W3[o, c, tap t] y[b, c, p],  t = ky * 3 + kx  (no shift);
 *       w3pack: the tap matrix [9 c_out, 256] as A fragments, vcnf_convnet3_w3_pack_floats(c_out) floats
 *       (vcnf_amd/nets/cnn.py::pack_conv1x1 with ceil(9 c_out / 32) row blocks);
 *   vcnf_col2im3x3_f32: out[b, o, py, px] = bias[o] + sum over the taps inside the image of
 *       z[b, t * channels + o, py + dy - 1, px + dx - 1]  (the convolution's zero padding).
 * c_in <= 24, c_out <= 56.  Matrix path and saturation counter as vcnf_conv1x1_f16x3_f32. */
int vcnf_convnet3_supported(int32_t c_in, int32_t hidden, int32_t c_out);
int64_t vcnf_convnet3_w3_pack_floats(int32_t c_out);
int vcnf_convnet3_taps_f16x3_f32(const float* x, float* z, const float* w1pack, int64_t w1pack_floats,
                                 const float* w2pack, int64_t w2pack_floats, const float* w3pack, int64_t w3pack_floats,
                                 const float* b1, const float* b2, int64_t batch, int32_t c_in, int32_t c_out,
                                 int32_t height, int32_t width, float slope1, float slope2, int32_t* sat_count,
                                 void* stream);
int vcnf_col2im3x3_f32(const float* z, const float* bias, float* out, int64_t batch, int32_t channels,
                       int32_t height, int32_t width, void* stream);

/* Fused elementwise maps of a residual block of the conditioner and of its backward (training path;
 * nets/resnet.py:38-57 under autograd), n contiguous floats each:
 *   op 0: out0 = a + b * sigmoid(c)                          (block output: input + second Linear gated by the context)
 *   op 1: out0 = a * s, out1 = a * b * s * (1 - s), s = sigmoid(c)     (gradients of the gated product)
 *   op 2: out0 = a where b > 0, else 0                       (ReLU backward, b = the ReLU's output; c unused)
 *   op 3: out0 = c + (a where b > 0, else 0)                 (ReLU backward joined with the skip connection's gradient) */
int vcnf_resblock_elementwise_f32(int op, const float* a, const float* b, const float* c, float* out0, float* out1,
                                  int64_t n, void* stream);

/* Identity half of one RQS coupling layer in one launch (coupling.py:76-116): for f < d_id and v = x[b, identity_idx[f]]
 *   y = S_f(v) (inverse = 0) or S_f^-1(v) (inverse = 1) with the batch-shared unconditional spline of feature f
 *       (PiecewiseRationalQuadraticCDF, coupling.py:165-246), or y = v when shared_w/h/d are all NULL;
 *   out[b, identity_idx[f]] = y;   cond_in[b, f] = cond_sees_output ? y : v   (cond_in may be NULL): the conditioner
 *       sees the raw identity features in the density direction (:78-80) and S^-1 of them when sampling (:110-114);
 *   partial[c][b] = sum of log|dy/dv| over features 64 c .. 64 c + 63, c < vcnf_rqs_identity_half_partial_rows(d_id)
 *       (written only with shared logits; the caller adds the rows - deterministic, no atomics).
 * Bin counts 4, 8, 10, 16, 32; tails none / linear (vcnf_rqs_identity_half_supported).  Results are bitwise those of
 * vcnf_rqs_shared_f32 on the gathered columns. */
int vcnf_rqs_identity_half_supported(int32_t num_bins, int32_t tails);
int64_t vcnf_rqs_identity_half_partial_rows(int32_t d_id);
int vcnf_rqs_identity_half_f32(const float* x, float* y, float* cond_in, float* partial, int64_t batch,
                               int32_t features, const int32_t* identity_idx, int32_t d_id,
                               const float* shared_w, const float* shared_h, const float* shared_d,
                               const vcnf_rqs_cfg* cfg, int inverse, int cond_sees_output,
                               int32_t* bad_disc, void* stream);

/* Packed conditioner weights of one fused RQS coupling layer: ONE device buffer of
 * vcnf_rqs_layer_fused_pack_floats(d_id, d_t, ctx_dim, num_blocks) floats (0: shape not supported) holding the ResidualNet's nn.Linear
 * weights (nets/resnet.py:78-90) re-ordered into matrix-core fragments, in the order
 *   W0 | b0 | per block: WA | ba | WB | bb | (WC | bc if ctx_dim > 0) | WF | bf
 * (exact fragment order: vcnf_amd/fused.py::pack_layer, csrc/fused_common.hpp PackLayout / PackLayout6). */
int64_t vcnf_rqs_layer_fused_pack_floats(int32_t d_id, int32_t d_t, int32_t ctx_dim, int32_t num_blocks);

/* 1 if vcnf_rqs_layer_fused_f32 has a kernel for this layer shape, else 0. */
int vcnf_rqs_layer_fused_supported(int32_t d_id, int32_t d_t, int32_t ctx_dim, int32_t hidden,
                                   int32_t num_blocks, int32_t num_bins, int32_t tails);

/* One RQS coupling layer INCLUDING its ResidualNet conditioner in a single kernel:
 * Coupling.forward / .inverse (flows/neural_spline/coupling.py:70-96 / :98-125) with
 * transform_net = ResidualNet(ReLU, no batch norm, dropout 0; nets/resnet.py:92-106)
 * evaluated on the fp32 matrix cores.  Same results contract as
 * vcnf_rqs_conditioner_input_f32 + the dense layers + vcnf_rqs_coupling_f32; the
 * conditioner output never touches HBM.  context[B, ctx_dim] may be NULL when
 * ctx_dim = 0.  x, y, context must be 16-byte aligned.
 * precision: VCNF_PREC_F32 - every dense layer on v_mfma_f32_16x16x4_f32 (exact fp32
 * fma chains); VCNF_PREC_F16X3 - every dense layer on v_mfma_f32_32x32x16_f16 with both
 * operands split into hi + lo*2^-11 fp16 halves (3 instructions per product, 4 in the
 * 16- and 48-deep layers, fp32 accumulation; GEMM error at or below the F32 path's on
 * every layer shape, tests/test_gpu_gemm_error.py).  The halves cannot carry a value
 * beyond +-65504 or a non-finite input.  redo_tiles (device int32, one entry per
 * vcnf_rqs_layer_fused_tile_rows() = 32 consecutive samples, ceil(batch / 32) entries, may
 * be NULL) makes the pair of calls below range-safe WITHOUT a host round trip:
 *   F16X3 call: redo_tiles is OUTPUT - 1 for the rows of a tile that held such a value
 *     (the kernel's tile is 32 samples for small batches, 128 = four entries otherwise),
 *     and then no y row and no logdet entry of that tile is written; 0 otherwise.
 *   F32 call with the same arguments (and the F32 packing of the same weights):
 *     redo_tiles is INPUT - only the flagged rows are evaluated and written.
 * After both, every sample has fp32-range results (the reference is plain fp32,
 * nets/resnet.py:92-106).  With redo_tiles == NULL the F16X3 call clamps at +-65504 and
 * stores.  sat_count (device int32, may be NULL) is incremented once per out-of-range tile
 * in either case.  wpack must have been packed for the same precision; the F16X3 buffer
 * has the 1/sqrt(hidden) logit scale (coupling.py:314-316) and the log2(e) factors of the
 * softmax / softplus / sigmoid exponentials folded in (vcnf_amd/fused.py::pack_layer_h3),
 * cfg->wh_scale must be the folded value. */
int32_t vcnf_rqs_layer_fused_tile_rows(void);
/* F16X3 path: batches of up to `rows` samples run on 32-sample tiles (one workgroup per 32
 * samples: the batch sizes of the reference's drivers, /root/reference/run.py:45-47, fill the
 * chip), larger ones on 128-sample tiles.  Same results contract; y is bitwise the same on
 * both, logdet differs by the order of its per-sample sum.  Process-wide; rows < 0 only
 * queries.  Returns the previous value (default 16384). */
int64_t vcnf_rqs_layer_fused_small_batch_rows(int64_t rows);
int vcnf_rqs_layer_fused_f32(const float* x, const float* context, float* y, float* logdet,
                             int64_t batch, const int32_t* transform_idx, int32_t d_t,
                             const int32_t* identity_idx, int32_t d_id, int32_t ctx_dim,
                             int32_t hidden, int32_t num_blocks, int32_t precision,
                             const float* wpack, int64_t wpack_floats,
                             const float* shared_w, const float* shared_h, const float* shared_d,
                             const vcnf_rqs_cfg* cfg, int inverse,
                             int ld_mode, float ld_sign, int32_t* bad_disc, int32_t* sat_count,
                             int32_t* redo_tiles, void* stream);

/* A run of MaskedAffineFlow layers INCLUDING their MLP conditioners s, t = Linear(D, H) - LeakyReLU - Linear(H, D), and
 * of the per-feature affine layers (AffineConstFlow / ActNorm) between them, in one launch: the loop body of
 * NormalizingFlow.log_prob / sample (core.py:144-183) over the models of the reference's own drivers
 * (/root/reference/run.py:58-68: K x [MaskedAffineFlow(b, t, s), ActNorm], D = 2 .. 15, 1024 - 2048 samples, fp64).
 * Layer arithmetic: flows/affine/coupling.py:171-222 (non-finite s / t -> NaN), :22-61, nets/mlp.py:30-58.
 * z, out [batch, features], features <= 16, hidden <= 64; logdet receives / accumulates ld_sign * the summed log|det|
 * of the run (inverse: every layer inverted, in the order given).  table: DEVICE array of 12 int64 per layer in
 * application order - [0] kind (0 masked affine, 1 per-feature), [1] hidden width, [2] LeakyReLU slope (bits of a
 * double), [3] b [features]; [4..7] s: W1 [H, D], b1 [H], W2 [D, H], b2 [D] (0: no s); [8..11] t likewise;
 * per-feature kind: [4] s [features] or 0, [5] t [features] or 0.  All pointers of the scalar type of the call. */
int vcnf_masked_affine_stack_supported(int32_t features, int32_t hidden);
int vcnf_masked_affine_stack_f32(const float* z, float* out, float* logdet, const int64_t* table,
                                 int64_t batch, int32_t features, int32_t n_layers, int inverse,
                                 int ld_mode, float ld_sign, void* stream);
int vcnf_masked_affine_stack_f64(const double* z, double* out, double* logdet, const int64_t* table,
                                 int64_t batch, int32_t features, int32_t n_layers, int inverse,
                                 int ld_mode, double ld_sign, void* stream);

/* Vector-Jacobian product of vcnf_masked_affine_stack_* (training through these layers: core.py:30-141 over
 * coupling.py:171-222 / :22-61 / mlp.py:30-58).  z_out = the forward call's output (nothing else is kept: the
 * kernel walks the layers backwards and rebuilds every layer's input from its output), g_out / g_logdet = upstream
 * gradients of the output and of the run's summed log|det| (g_logdet may be NULL), g_in = gradient of the run's
 * input.  Parameter gradients are ADDED (hardware floating-point atomics, batch order not fixed) into the flat
 * buffer `grads`, zeroed by the caller; grad_offsets[l] = element offset of layer l's block - masked affine:
 * [W1s | b1s | W2s | b2s | W1t | b1t | W2t | b2t] (absent conditioners take no room), per-feature: [s | t]. */
int vcnf_masked_affine_stack_bwd_f32(const float* z_out, const float* g_out, const float* g_logdet, float* g_in,
                                     float* grads, const int64_t* table, const int64_t* grad_offsets,
                                     int64_t batch, int32_t features, int32_t n_layers, int inverse, void* stream);
int vcnf_masked_affine_stack_bwd_f64(const double* z_out, const double* g_out, const double* g_logdet, double* g_in,
                                     double* grads, const int64_t* table, const int64_t* grad_offsets,
                                     int64_t batch, int32_t features, int32_t n_layers, int inverse, void* stream);

/* Dense layer at training batch sizes on the fp16 split-half matrix path (csrc/linear_f16x3.hip):
 *   y[b, n] = sum_k x[b, k] * A[n, k] (+ bias[n]),  A[n, k] = w[n * ldn + k * ldk],  x [batch, k], y [batch, n]
 * = nn.Linear's forward (w = weight [n, k]: ldn = k, ldk = 1; nets/resnet.py:42-57, 92-106) and its input gradient
 * g_x = g_y W (w = weight [k, n]: ldn = 1, ldk = n), i.e. what autograd computes for the conditioner's dense layers
 * in NormalizingFlow.forward_kld (core.py:30-65).  The weights are read in their natural fp32 layout and split in
 * registers; arithmetic as VCNF_PREC_F16X3 of vcnf_rqs_layer_fused_f32 (lo*lo kept for k <= 48).  k % 16 == 0,
 * n % 4 == 0, and n <= 128 when k > 128.  x, y 16-byte aligned.  relu_input / relu_output: ReLU applied to x while it
 * is read / to y before it is stored (the residual block's activations, nets/resnet.py:42, :46, without their own
 * passes over memory); mask / addend [batch, n] (16-byte aligned, may be NULL): y = addend + y * (mask > 0) - a ReLU's
 * backward pass and the skip connection's gradient applied to an input gradient as it is stored (autograd of
 * nets/resnet.py:42-57).  x_amax (may be NULL; input-gradient form only: bias == NULL and ldk != 1, else
 * VCNF_ERR_UNSUPPORTED): [batch] device floats, the largest |x[b, :]| of every row (row_amax of
 * vcnf_abs_max_rows_cols_f32): the pre-scale of vcnf_linear_wgrad_f16x3_f32's dy_amax applied to the rows of x as they
 * are staged and taken out of the rows of y before mask and addend.  Values beyond +-65504 after that scaling
 * (or NaN inputs) are clamped and counted in sat_count (device int32, may be NULL) once per 64-sample tile. */
int vcnf_linear_f16x3_supported(int32_t k, int32_t n);
int vcnf_linear_f16x3_f32(const float* x, const float* w, const float* bias, float* y, int64_t batch,
                          int32_t k, int32_t n, int64_t ldn, int64_t ldk, int relu_input, int relu_output,
                          const float* mask, const float* addend, const float* x_amax, int32_t* sat_count,
                          void* stream);

/* A run of n_layers (<= vcnf_rqs_stack_fused_max_layers() = 16) RQS coupling layers of ONE shape and one spline
 * configuration in a single launch: the body of NormalizingFlow.log_prob / sample over consecutive
 * CoupledRationalQuadraticSpline layers (core.py:144-183 around coupling.py:70-125).  `layers` is a HOST array in
 * the order in which the layers are applied to x (its entries are copied into the launch); every entry carries the
 * layer's index vectors, its packed conditioner weights for `precision` and the unconditional spline's logits
 * (all layers with them, or none).  y = the last layer's output; logdet receives / accumulates ld_sign * the SUM of
 * the layers' log|det| (one rounding of the sum instead of one per layer).  Everything else as
 * vcnf_rqs_layer_fused_f32.  F16X3: every layer runs on 32-sample tiles that stay in LDS from the first layer to
 * the last (meant for the small batches at which one launch per layer is launch-bound: the reference's drivers use
 * 1024 - 2048 samples, /root/reference/run.py:45-47); a tile in which ANY layer met a value the fp16 halves cannot
 * carry is left unwritten and flagged in redo_tiles, and the same call with VCNF_PREC_F32 and the F32 packings
 * evaluates exactly the flagged rows through all layers on exact fp32 matrix instructions.  The one exception to
 * the 32-sample tiles: n_layers == 2 at a batch above vcnf_rqs_layer_fused_small_batch_rows() where
 * vcnf_rqs_pair_fused_supported() says 1 - the 128-sample-tile kernel then walks both layers per tile visit and adds
 * their log|det| one after the other: y AND logdet are bitwise those of two vcnf_rqs_layer_fused_f32 calls (the
 * fp32 re-evaluation of a flagged tile still adds the sum). */
typedef struct vcnf_rqs_stack_layer {
  const int32_t* transform_idx;
  const int32_t* identity_idx;
  const float* wpack;
  const float* shared_w;
  const float* shared_h;
  const float* shared_d;
} vcnf_rqs_stack_layer;
int32_t vcnf_rqs_stack_fused_max_layers(void);
/* 1 if a run of exactly TWO layers of this shape on the fp16 split-half path, at a batch above
 * vcnf_rqs_layer_fused_small_batch_rows(), is evaluated two layers per tile visit by the 128-sample-tile kernel (both
 * layers' tables fit its LDS), else 0.  y and logdet of such a run are bitwise those of two one-layer calls. */
int vcnf_rqs_pair_fused_supported(int32_t d_id, int32_t d_t, int32_t ctx_dim, int32_t hidden, int32_t num_blocks);
int vcnf_rqs_stack_fused_f32(const float* x, const float* context, float* y, float* logdet,
                             int64_t batch, const vcnf_rqs_stack_layer* layers, int32_t n_layers,
                             int32_t d_t, int32_t d_id, int32_t ctx_dim, int32_t hidden,
                             int32_t num_blocks, int32_t precision, int64_t wpack_floats,
                             const vcnf_rqs_cfg* cfg, int inverse, int ld_mode, float ld_sign,
                             int32_t* bad_disc, int32_t* sat_count, int32_t* redo_tiles, void* stream);

/* Affine coupling on z[B, C, inner] (inner = H*W, 1 for 2-D inputs).
 * Replaces AffineCoupling.forward / .inverse (flows/affine/coupling.py:113-142 /
 * :144-168) together with the channel Split / Merge around it
 * (flows/reshape.py:25-29, :50-55; AffineCouplingBlock :247-258): channels
 * [t_off, t_off+d_t) are transformed, all other channels are copied.
 * param[B, n_par*d_t, inner]: channel 2c = shift, 2c+1 = scale logit
 * (coupling.py:122-123); scale_map NONE: param[B, d_t, inner] is the shift. */
int vcnf_affine_coupling_f32(const float* z, const float* param, float* out, float* logdet,
                             int64_t batch, int32_t channels, int32_t inner,
                             int32_t t_off, int32_t d_t, int scale_map, int inverse,
                             int ld_mode, float ld_sign, void* stream);

/* A run of AffineCouplingBlocks with ONE conditioner shape (c_in, hidden, d_t as in
 * vcnf_affine_layer_fused_f32) and the column permutations between them in a single launch:
 * the reference's loop over [AffineCouplingBlock, Permute] pairs of NormalizingFlow.log_prob /
 * .sample (core.py:150-155, :176-183; flows/affine/coupling.py:225-258; flows/mixing.py:32-54)
 * for config C1 / C2 style stacks.  ``layers`` (HOST array, at most VCNF_AFFINE_STACK_MAX_LAYERS) is in EXECUTION
 * order of the requested direction; gather_before = row of ``gathers`` [n_gather_rows][features] (device int32) whose
 * permutation the layer's input columns go through (the layer sees z[:, row]), -1 for none;
 * gather_after likewise for the result.  wpack = the layers' vcnf_affine_layer_fused_pack_floats
 * buffers back to back, in the same order.  log|det| of all layers is added to / stored in logdet. */
enum { VCNF_AFFINE_STACK_MAX_LAYERS = 16 };
typedef struct {
  int32_t cond_off, t_off, d_t;
  int32_t gather_before;
} vcnf_affine_stack_layer;
/* 1 if vcnf_affine_stack_fused_f32 takes this layer shape at this feature count (the layer kernel's limits plus
 * the stack kernel's two LDS strips per wave: features <= 128), else 0 - then run the layers one launch each. */
int vcnf_affine_stack_fused_supported(int32_t c_in, int32_t hidden, int32_t n_out, int32_t features);
int vcnf_affine_stack_fused_f32(const float* x, float* y, float* logdet, int64_t batch, int32_t features,
                                int32_t n_layers, const vcnf_affine_stack_layer* layers, int32_t gather_after,
                                int32_t c_in, int32_t hidden, float leaky_slope, int scale_map,
                                const float* wpack, int64_t wpack_floats,
                                const int32_t* gathers, int32_t n_gather_rows,
                                int inverse, int ld_mode, float ld_sign, void* stream);

/* The same run with the two hidden-deep dense layers of every conditioner MLP (nets/mlp.py:30-35: hidden -> hidden,
 * hidden -> parameters) on the fp16 split-half matrix path (v_mfma_f32_16x16x32_f16, hi + lo halves of both operands,
 * fp32 accumulation; GEMM error at or below the fp32 chain's at depth >= 32, tests/test_gpu_gemm_error.py); the first
 * layer (raw inputs, c_in deep) stays on exact fp32 matrix instructions.  wpack as for vcnf_affine_stack_fused_f32
 * (first layer, biases; its second / third layer weights serve the range fallback), wpack_h3 =
 * vcnf_affine_layer_fused_h3_pack_floats floats per layer (vcnf_amd/fused_affine.py::pack_h3).  A wave whose hidden
 * activations leave the fp16 range (|h| > 65504) evaluates that layer with the exact fp32 body instead - nothing is
 * clamped - and bumps redo_count (device int32, may be NULL).  hidden in {32, 64, 128}. */
int64_t vcnf_affine_layer_fused_h3_pack_floats(int32_t c_in, int32_t hidden, int32_t n_out);
int vcnf_affine_stack_fused_f16x3_f32(const float* x, float* y, float* logdet, int64_t batch, int32_t features,
                                      int32_t n_layers, const vcnf_affine_stack_layer* layers,
                                      int32_t gather_after, int32_t c_in, int32_t hidden, float leaky_slope,
                                      int scale_map, const float* wpack, int64_t wpack_floats,
                                      const float* wpack_h3, int64_t wpack_h3_floats,
                                      const int32_t* gathers, int32_t n_gather_rows,
                                      int inverse, int ld_mode, float ld_sign, int32_t* redo_count, void* stream);

/* Elementwise map of the masked affine autoregressive flow (flows/affine/autoregressive.py:75-103): params
 * [batch, features, 2] = (unconstrained scale u, shift) per feature from one MADE pass (:96-103),
 * scale = sigmoid(u + 2) + 1e-3.  inverse = 0: y = scale x + shift, logdet = sum log scale (:75-81, the flow's
 * one-pass direction); inverse != 0: y = (x - shift) / scale, logdet = -sum log scale (:83-89, applied D times by the
 * sequential loop :29-36).  params must be 8-byte aligned. */
int vcnf_maf_affine_f32(const float* x, const float* params, float* out, float* logdet, int64_t batch,
                        int32_t features, int inverse, int ld_mode, float ld_sign, void* stream);

/* MaskedAffineFlow.forward / .inverse (flows/affine/coupling.py:202-211 /
 * :213-222) on z[B,D]; s,t [B,D] are the scale / shift net outputs (NULL =
 * zeros, coupling.py:192-200); b[D] the 0/1 float mask.  Non-finite s/t become
 * NaN (coupling.py:205-208). */
int vcnf_masked_affine_f32(const float* z, const float* s, const float* t, const float* b,
                           float* out, float* logdet, int64_t batch, int32_t features,
                           int inverse, int ld_mode, float ld_sign, void* stream);

/* AffineConstFlow / ActNorm arithmetic (flows/affine/coupling.py:37-53) on
 * z[B, C, inner] with per-channel s[C], t[C] (either may be NULL = zeros);
 * the parameter-only log_det (a scalar) is left to the host. */
int vcnf_affine_const_f32(const float* z, const float* s, const float* t, float* out,
                          int64_t batch, int32_t channels, int32_t inner, int inverse, void* stream);

/* Column gather out[b, j, :] = z[b, idx[j], :] for z[B, C, inner].
 * Replaces Permute.forward / .inverse (flows/mixing.py:32-54) and
 * _Permutation._permute (:219-228). */
int vcnf_permute_f32(const float* z, const int32_t* idx, float* out,
                     int64_t batch, int32_t channels, int32_t inner, void* stream);

/* The channel partition of a coupling as two tensors, and back (training path: the gather
 * inputs[:, identity_features] / inputs[:, transform_features] and the scatter outputs[:, ...] = ... of
 * flows/neural_spline/coupling.py:86-88, :122-124 - each the other's VJP).  z / out [B, C] row-major;
 * first_part [B, first], second_part [B, C - first].
 * split:  first_part[b, c] = z[b, idx[c]] (c < first), second_part[b, c - first] = z[b, idx[c]] (c >= first).
 * merge:  out[b, c] = p < first ? first_part[b, p] : second_part[b, p - first] with p = idx[c]
 *         (idx of merge = the inverse permutation of the idx of split). */
int vcnf_split_columns_f32(const float* z, const int32_t* idx, float* first_part, float* second_part,
                           int64_t batch, int32_t channels, int32_t first, void* stream);
int vcnf_merge_columns_f32(const float* first_part, const float* second_part, const int32_t* idx, float* out,
                           int64_t batch, int32_t channels, int32_t first, void* stream);

/* DiagGaussian.log_prob (normflow/distributions/base.py:644-652).
 * loc, log_scale [D]; log_temperature = log(T) or 0; logp[B] per ld_mode. */
int vcnf_diag_gaussian_log_prob_f32(const float* z, const float* loc, const float* log_scale,
                                    float log_temperature, float* logp, int64_t batch,
                                    int32_t features, int ld_mode, float ld_sign, void* stream);

/* DiagGaussian.forward (base.py:632-642) with the standard-normal draw eps[B,D]
 * supplied by the caller: z = loc + exp(log_scale) * eps, logp[B]. */
int vcnf_diag_gaussian_sample_f32(const float* eps, const float* loc, const float* log_scale,
                                  float log_temperature, float* z, float* logp, int64_t batch,
                                  int32_t features, void* stream);

/* ---- fp64 variants.  The reference's Flow contract is dtype-agnostic and its drivers convert
 * the model with .double() (/root/reference/run.py:114, rundiag.py:90, runadultvdeq.py:183 over MaskedAffineFlow,
 * ActNorm and Gaussian bases).  Same contracts as the _f32 entry points of the same name with every float buffer and
 * scalar a double; elementwise HBM-bound maps only - the fused / matrix-core kernels stay fp32. */
typedef struct vcnf_rqs_cfg_f64 {
  int32_t num_bins;
  int32_t tails;
  double left, right, bottom, top;
  double min_bin_width, min_bin_height, min_derivative, wh_scale;
} vcnf_rqs_cfg_f64;
int vcnf_rqs_elementwise_f64(const double* x, const double* uw, const double* uh, const double* ud,
                             int64_t ld_w, int64_t ld_h, int64_t ld_d,
                             double* y, double* logabsdet, int64_t n,
                             const vcnf_rqs_cfg_f64* cfg, int inverse, int32_t* bad_disc, void* stream);
/* VJP of vcnf_rqs_elementwise_f64: the contract of vcnf_rqs_elementwise_bwd_f32 in double (dense gradient rows). */
int vcnf_rqs_elementwise_bwd_f64(const double* x, const double* uw, const double* uh, const double* ud,
                                 int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                 const double* g_y, const double* g_logabsdet,
                                 double* g_x, double* g_uw, double* g_uh, double* g_ud, int64_t n,
                                 const vcnf_rqs_cfg_f64* cfg, int inverse, void* stream);
/* vcnf_rqs_elementwise_strided_f32 in double (image-shaped couplings: the conditioner output [B, C*P, H, W] read in
 * place).  Per element the same bin and the same arithmetic as vcnf_rqs_elementwise_f64. */
int vcnf_rqs_elementwise_strided_f64(const double* x, const double* uw, const double* uh, const double* ud,
                                     int64_t row_w, int64_t row_h, int64_t row_d, int64_t inner,
                                     int64_t k_stride, int64_t period,
                                     double* y, double* logabsdet, int64_t n,
                                     const vcnf_rqs_cfg_f64* cfg, int inverse, int32_t* bad_discriminant,
                                     void* stream);
/* VJP of vcnf_rqs_elementwise_strided_f64 on the conditioner layout: the contract of vcnf_rqs_packed_bwd_f32 in
 * double (g_params written in the layout of params). */
int vcnf_rqs_packed_bwd_f64(const double* x, const double* params, int64_t inner, int64_t lad_div,
                            const double* g_y, const double* g_logabsdet,
                            double* g_x, double* g_params, int64_t n,
                            const vcnf_rqs_cfg_f64* cfg, int inverse, void* stream);
/* vcnf_rqs_elementwise_limits_f32 / _bwd_f32 in double: per element the bin and the arithmetic of
 * vcnf_rqs_elementwise_f64 / vcnf_rqs_elementwise_bwd_f64 with that element's limits. */
int vcnf_rqs_elementwise_limits_f64(const double* x, const double* uw, const double* uh, const double* ud,
                                    int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                    const double* left, const double* right, const double* bottom, const double* top,
                                    const vcnf_rqs_limit_bcast* bcast, double* y, double* logabsdet, int64_t n,
                                    const vcnf_rqs_cfg_f64* cfg, int inverse, int32_t* bad_disc, void* stream);
int vcnf_rqs_elementwise_limits_bwd_f64(const double* x, const double* uw, const double* uh, const double* ud,
                                        int64_t ld_w, int64_t ld_h, int64_t ld_d,
                                        const double* left, const double* right, const double* bottom,
                                        const double* top, const vcnf_rqs_limit_bcast* bcast,
                                        const double* g_y, const double* g_logabsdet,
                                        double* g_x, double* g_uw, double* g_uh, double* g_ud,
                                        double* g_left, double* g_right, double* g_bottom, double* g_top, int64_t n,
                                        const vcnf_rqs_cfg_f64* cfg, int inverse, void* stream);
/* vcnf_maf_affine_f32 in double; params must be 16-byte aligned (one double2 load per feature). */
int vcnf_maf_affine_f64(const double* x, const double* params, double* out, double* logdet, int64_t batch,
                        int32_t features, int inverse, int ld_mode, double ld_sign, void* stream);
int vcnf_affine_coupling_f64(const double* z, const double* param, double* out, double* logdet,
                             int64_t batch, int32_t channels, int32_t inner,
                             int32_t t_off, int32_t d_t, int scale_map, int inverse,
                             int ld_mode, double ld_sign, void* stream);
int vcnf_masked_affine_f64(const double* z, const double* s, const double* t, const double* b,
                           double* out, double* logdet, int64_t batch, int32_t features,
                           int inverse, int ld_mode, double ld_sign, void* stream);
int vcnf_affine_const_f64(const double* z, const double* s, const double* t, double* out,
                          int64_t batch, int32_t channels, int32_t inner, int inverse, void* stream);
int vcnf_permute_f64(const double* z, const int32_t* idx, double* out,
                     int64_t batch, int32_t channels, int32_t inner, void* stream);
int vcnf_split_columns_f64(const double* z, const int32_t* idx, double* first_part, double* second_part,
                           int64_t batch, int32_t channels, int32_t first, void* stream);
int vcnf_merge_columns_f64(const double* first_part, const double* second_part, const int32_t* idx, double* out,
                           int64_t batch, int32_t channels, int32_t first, void* stream);
int vcnf_diag_gaussian_log_prob_f64(const double* z, const double* loc, const double* log_scale,
                                    double log_temperature, double* logp, int64_t batch,
                                    int32_t features, int ld_mode, double ld_sign, void* stream);
int vcnf_diag_gaussian_sample_f64(const double* eps, const double* loc, const double* log_scale,
                                  double log_temperature, double* z, double* logp, int64_t batch,
                                  int32_t features, void* stream);

/* ---- Class-conditional diagonal Gaussian end caps: GlowBase (normflow/distributions/base.py:778-869) and
 * ClassCondDiagGaussian (:715-775).  z / eps [B, C, P] contiguous (d = C * P elements per sample: C channels of
 * P = pixels elements); the parameters are tables loc_rows, log_scale_rows [rows, C].  Sample b uses table row
 * row_index[b] (int32 [B]); with row_index == NULL it uses row b (rows == B) or row 0 (rows == 1).  A row_index entry
 * outside [0, rows) reads nothing out of bounds: that sample's logp and its z / dz / d_eps row (and its d_loc / d_ls
 * rows) are written as NaN, with no host synchronisation.  With ls = log_scale_rows[row, c] + log_temperature:
 *   log_prob:  logp[b] = -0.5 d log(2 pi) - P sum_c ls - 0.5 sum_{c,p} ((z - loc) / exp(ls))^2   (per ld_mode / ld_sign)
 *   sample:    z = loc + exp(ls) eps,  logp[b] = -0.5 d log(2 pi) - P sum_c ls - 0.5 sum eps^2
 *   log_prob_bwd (g[B]):  dz = -g u / s,  d_loc[b, c] = sum_p g u / s,  d_log_scale[b, c] = sum_p g (u^2 - 1),
 *                         u = (z - loc) / s, s = exp(ls)
 *   sample_bwd (g_z[B, d], g_logp[B]):  d_eps = g_z s - g_logp eps,  d_loc[b, c] = sum_p g_z,
 *                         d_log_scale[b, c] = sum_p g_z s eps - P g_logp
 * d_loc / d_log_scale are [B, C] (per sample); vcnf_cc_gaussian_reduce_rows_* sums them onto the table rows:
 * out_rows[r, c] = sum over {b: row_index[b] == r} of per_sample[b, c], in a fixed order (rows <= 65535).
 * No atomics: every call is bitwise reproducible.  Status: channels < 1, pixels < 1, rows < 1 or (row_index == NULL
 * and rows not in {1, batch}) -> VCNF_ERR_SHAPE; batch == 0 -> VCNF_OK without a launch; NULL required pointer ->
 * VCNF_ERR_NULL; a pointer not aligned to its element size -> VCNF_ERR_ALIGN.  16-byte accesses are used when the
 * buffers are 16-byte aligned and pixels % V == 0, or pixels == 1 and channels % V == 0 (V = 4 floats / 2 doubles). */
int vcnf_cc_gaussian_log_prob_f32(const float* z, const float* loc_rows, const float* log_scale_rows,
                                  const int32_t* row_index, float log_temperature, float* logp, int64_t batch,
                                  int32_t channels, int32_t pixels, int64_t rows, int ld_mode, float ld_sign,
                                  void* stream);
int vcnf_cc_gaussian_sample_f32(const float* eps, const float* loc_rows, const float* log_scale_rows,
                                const int32_t* row_index, float log_temperature, float* z, float* logp,
                                int64_t batch, int32_t channels, int32_t pixels, int64_t rows, void* stream);
int vcnf_cc_gaussian_log_prob_bwd_f32(const float* z, const float* loc_rows, const float* log_scale_rows,
                                      const int32_t* row_index, float log_temperature, const float* g, float* dz,
                                      float* d_loc, float* d_log_scale, int64_t batch, int32_t channels,
                                      int32_t pixels, int64_t rows, void* stream);
int vcnf_cc_gaussian_sample_bwd_f32(const float* eps, const float* log_scale_rows, const int32_t* row_index,
                                    float log_temperature, const float* g_z, const float* g_logp, float* d_eps,
                                    float* d_loc, float* d_log_scale, int64_t batch, int32_t channels,
                                    int32_t pixels, int64_t rows, void* stream);
int vcnf_cc_gaussian_reduce_rows_f32(const float* per_sample, const int32_t* row_index, float* out_rows,
                                     int64_t batch, int32_t channels, int64_t rows, void* stream);
int vcnf_cc_gaussian_log_prob_f64(const double* z, const double* loc_rows, const double* log_scale_rows,
                                  const int32_t* row_index, double log_temperature, double* logp, int64_t batch,
                                  int32_t channels, int32_t pixels, int64_t rows, int ld_mode, double ld_sign,
                                  void* stream);
int vcnf_cc_gaussian_sample_f64(const double* eps, const double* loc_rows, const double* log_scale_rows,
                                const int32_t* row_index, double log_temperature, double* z, double* logp,
                                int64_t batch, int32_t channels, int32_t pixels, int64_t rows, void* stream);
int vcnf_cc_gaussian_log_prob_bwd_f64(const double* z, const double* loc_rows, const double* log_scale_rows,
                                      const int32_t* row_index, double log_temperature, const double* g, double* dz,
                                      double* d_loc, double* d_log_scale, int64_t batch, int32_t channels,
                                      int32_t pixels, int64_t rows, void* stream);
int vcnf_cc_gaussian_sample_bwd_f64(const double* eps, const double* log_scale_rows, const int32_t* row_index,
                                    double log_temperature, const double* g_z, const double* g_logp, double* d_eps,
                                    double* d_loc, double* d_log_scale, int64_t batch, int32_t channels,
                                    int32_t pixels, int64_t rows, void* stream);
int vcnf_cc_gaussian_reduce_rows_f64(const double* per_sample, const int32_t* row_index, double* out_rows,
                                     int64_t batch, int32_t channels, int64_t rows, void* stream);

/* ---- Gaussian mixture base distribution (normflow 1.2 distributions/base.py GaussianMixture).  z / eps [B, D]
 * contiguous; the parameters are tables loc, log_scale [M, D] and the log mixture weights log_w [M]
 * (log softmax of the module's weight_scores).  With u = (z - loc[m]) / exp(log_scale[m]):
 *   a[b, m]  = log_w[m] - sum_d log_scale[m, d] - 0.5 D log(2 pi) - 0.5 sum_d u^2
 *   log_prob:  logp[b] = sign * logsumexp_m a[b, m]   (ld_mode VCNF_LD_STORE writes it, VCNF_LD_ACCUM adds it to logp);
 *              a running maximum keeps it finite wherever the exact value is
 *   sample:    z[b] = eps[b] * exp(log_scale[mode[b]]) + loc[mode[b]], logp[b] = the mixture log density of that z.
 *              mode is int32 [B]; an entry outside [0, M) reads row 0 and that sample's z row and logp are written as
 *              NaN: no out-of-bounds access, nothing for the host to check
 *   log_prob_bwd (lse[B] = the forward's logp, cotangent g[B], gz_in[B, D] or NULL): with r = exp(a - lse)
 *              dz = gz_in - g sum_m r u / s,  and per workgroup k one block partials[k] [M, 2 D + 1] holding the
 *              workgroup's share of  d_loc[m] = sum_b g r u / s | d_log_scale[m] = sum_b g r (u^2 - 1) | d_log_w[m] =
 *              sum_b g r,  added in a fixed order.  partials has vcnf_gmm_bwd_groups(batch, D, M) blocks; every block
 *              is written in full.  partials == NULL: only dz is computed (no table needs a gradient)
 *   reduce_partials: d_loc, d_log_scale [M, D] and d_log_w [M] = the sum of `groups` blocks in a fixed order
 * vcnf_gmm_bwd_groups is a pure function of its arguments (no device query; 0 for an unsupported shape).
 * Supported: features >= 1, modes >= 1, features * modes <= VCNF_GMM_MAX_TABLE, else VCNF_ERR_SHAPE (groups < 1 as
 * well); unknown ld_mode -> VCNF_ERR_UNSUPPORTED; batch == 0 -> VCNF_OK without a launch; NULL required pointer ->
 * VCNF_ERR_NULL; a pointer not aligned to its element size -> VCNF_ERR_ALIGN.  The tables are staged in LDS once per
 * workgroup;
 * 16-byte (8-byte) accesses are used when features % V == 0 and the row buffers are aligned to them.  No atomics,
 * no allocation, no host synchronisation: every call is bitwise reproducible and capturable. */
enum { VCNF_GMM_MAX_TABLE = 8192 };
int64_t vcnf_gmm_bwd_groups(int64_t batch, int32_t features, int32_t modes);
int vcnf_gmm_log_prob_f32(const float* z, const float* loc, const float* log_scale, const float* log_w, float* logp,
                          int64_t batch, int32_t features, int32_t modes, int ld_mode, float sign, void* stream);
int vcnf_gmm_sample_f32(const float* eps, const int32_t* mode, const float* loc, const float* log_scale,
                        const float* log_w, float* z, float* logp, int64_t batch, int32_t features, int32_t modes,
                        void* stream);
int vcnf_gmm_log_prob_bwd_f32(const float* z, const float* loc, const float* log_scale, const float* log_w,
                              const float* lse, const float* g, const float* gz_in, float* dz, float* partials,
                              int64_t batch, int32_t features, int32_t modes, void* stream);
int vcnf_gmm_reduce_partials_f32(const float* partials, int64_t groups, int32_t modes, int32_t features, float* d_loc,
                                 float* d_log_scale, float* d_log_w, void* stream);
int vcnf_gmm_log_prob_f64(const double* z, const double* loc, const double* log_scale, const double* log_w,
                          double* logp, int64_t batch, int32_t features, int32_t modes, int ld_mode, double sign,
                          void* stream);
int vcnf_gmm_sample_f64(const double* eps, const int32_t* mode, const double* loc, const double* log_scale,
                        const double* log_w, double* z, double* logp, int64_t batch, int32_t features, int32_t modes,
                        void* stream);
int vcnf_gmm_log_prob_bwd_f64(const double* z, const double* loc, const double* log_scale, const double* log_w,
                              const double* lse, const double* g, const double* gz_in, double* dz, double* partials,
                              int64_t batch, int32_t features, int32_t modes, void* stream);
int vcnf_gmm_reduce_partials_f64(const double* partials, int64_t groups, int32_t modes, int32_t features,
                                 double* d_loc, double* d_log_scale, double* d_log_w, void* stream);

/* ---- Heavy-tailed product base distributions: Student-t and the generalised Gaussian, one tail parameter per
 * feature.  z / eps / gamma [B, D] contiguous; the parameters are the rows loc, log_scale, shape (nu or beta) and cst
 * (the normalisers) [D].  The caller computes cst - for Student-t lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2, for
 * the generalised Gaussian log(beta) - log 2 - lgamma(1/beta) - and draws the random numbers: no kernel evaluates a
 * special function or draws.  With u = (z - loc) / exp(log_scale):
 *   f(u; nu)   = -(nu + 1)/2 log1p(u^2 / nu)                         VCNF_TAIL_STUDENT_T
 *   f(u; beta) = -|u|^beta = -exp(beta log|u|), 0 at u == 0          VCNF_TAIL_GEN_GAUSSIAN
 *   log_prob:  logp[b] = sign * sum_d (cst[d] - log_scale[d] + f(u; shape[d]))   (ld_mode as for vcnf_gmm_log_prob_*)
 *   sample:    u = eps sqrt(nu / (2 gamma)) with eps ~ N(0, 1), gamma ~ Gamma(nu/2, 1), or
 *              u = sign(eps) gamma^(1/beta) with gamma ~ Gamma(1/beta, 1), where |u|^beta = gamma is used as is;
 *              z[b] = loc + exp(log_scale) u and logp[b] = the log density of that z
 *   log_prob_bwd (cotangent g[B], gz_in[B, D] or NULL): dz = gz_in + g df/du / s, and per workgroup k one block
 *              partials[k] [3, D] with the workgroup's share of  d_loc = -sum_b g df/du / s | d_log_scale =
 *              sum_b g (-1 - u df/du) | sum_b g df/dshape (the part of d_shape that does not go through cst), added in a
 *              fixed order.  Student-t: df/du = -(nu+1) u / (nu + u^2), df/dnu = -log1p(u^2/nu)/2 + (nu+1) u^2 /
 *              (2 nu (nu + u^2)).  Generalised Gaussian: df/du = -beta |u|^beta / u, df/dbeta = -|u|^beta log|u|, and
 *              both 0 at u == 0 for every beta (for beta < 1, where df/du is unbounded there, a convention).
 *              partials has vcnf_tail_bwd_groups(batch, D) blocks, every block is written in full; partials == NULL:
 *              only dz is computed
 *   sample_bwd (cotangents g_z[B, D] and g_lp[B], either may be NULL = zero): deps (may be NULL) and dgamma [B, D], and
 *              blocks as above for the three rows.  du/deps = sqrt(nu / (2 gamma)), du/dgamma = -u / (2 gamma),
 *              du/dnu = u / (2 nu);  du/deps = 0, du/dgamma = u / (beta gamma), du/dbeta = -u log(gamma) / beta^2
 *   reduce_partials: d_loc, d_log_scale, d_shape [D] = the sum of `groups` blocks in a fixed order
 * vcnf_tail_bwd_groups is a pure function of its arguments (no device query; 0 for an unsupported shape).
 * features >= 1 (no upper limit) and batch >= 0, else VCNF_ERR_SHAPE (groups < 1 as well); unknown family or ld_mode ->
 * VCNF_ERR_UNSUPPORTED; batch == 0 -> VCNF_OK without a launch; NULL required pointer -> VCNF_ERR_NULL; a pointer not
 * aligned to its element size -> VCNF_ERR_ALIGN.  16-byte (8-byte) accesses are used when features % V == 0 and the
 * [B, D] buffers are aligned to them.  No atomics, no allocation, no host synchronisation: every call is bitwise
 * reproducible and capturable. */
enum { VCNF_TAIL_STUDENT_T = 0, VCNF_TAIL_GEN_GAUSSIAN = 1 };
int64_t vcnf_tail_bwd_groups(int64_t batch, int32_t features);
int vcnf_tail_log_prob_f32(const float* z, const float* loc, const float* log_scale, const float* shape,
                           const float* cst, float* logp, int64_t batch, int32_t features, int family, int ld_mode,
                           float sign, void* stream);
int vcnf_tail_sample_f32(const float* eps, const float* gamma, const float* loc, const float* log_scale,
                         const float* shape, const float* cst, float* z, float* logp, int64_t batch, int32_t features,
                         int family, void* stream);
int vcnf_tail_log_prob_bwd_f32(const float* z, const float* loc, const float* log_scale, const float* shape,
                               const float* g, const float* gz_in, float* dz, float* partials, int64_t batch,
                               int32_t features, int family, void* stream);
int vcnf_tail_sample_bwd_f32(const float* eps, const float* gamma, const float* loc, const float* log_scale,
                             const float* shape, const float* g_z, const float* g_lp, float* deps, float* dgamma,
                             float* partials, int64_t batch, int32_t features, int family, void* stream);
int vcnf_tail_reduce_partials_f32(const float* partials, int64_t groups, int32_t features, float* d_loc,
                                  float* d_log_scale, float* d_shape, void* stream);
int vcnf_tail_log_prob_f64(const double* z, const double* loc, const double* log_scale, const double* shape,
                           const double* cst, double* logp, int64_t batch, int32_t features, int family, int ld_mode,
                           double sign, void* stream);
int vcnf_tail_sample_f64(const double* eps, const double* gamma, const double* loc, const double* log_scale,
                         const double* shape, const double* cst, double* z, double* logp, int64_t batch, int32_t features,
                         int family, void* stream);
int vcnf_tail_log_prob_bwd_f64(const double* z, const double* loc, const double* log_scale, const double* shape,
                               const double* g, const double* gz_in, double* dz, double* partials, int64_t batch,
                               int32_t features, int family, void* stream);
int vcnf_tail_sample_bwd_f64(const double* eps, const double* gamma, const double* loc, const double* log_scale,
                             const double* shape, const double* g_z, const double* g_lp, double* deps, double* dgamma,
                             double* partials, int64_t batch, int32_t features, int family, void* stream);
int vcnf_tail_reduce_partials_f64(const double* partials, int64_t groups, int32_t features, double* d_loc,
                                  double* d_log_scale, double* d_shape, void* stream);

/* ---- End caps of the flow VAE (NormalizingFlowVAE): the amortised diagonal Gaussian encoder and the Gaussian /
 * Bernoulli decoders.  rows = batch * samples rows of `features` = D columns, all buffers contiguous; row n belongs to
 * data item n / samples.  A parameter row is h = [mean (D) | lv (D)], 2 D contiguous values with lv the log variance
 * (for a net output [., 2 C, H, W] that is the contiguous row, D = C H W).  An operand that the rows of an item share
 * is read through its divisor (row n reads its row n / div) and never repeated in memory.
 *   encode (h [batch, 2 D], eps [rows, D]):  z = mean + exp(lv / 2) eps [rows, D],
 *              logq[n] = -D/2 log 2 pi - sum_j (lv / 2 + eps^2 / 2)       (log std is lv / 2 as it stands)
 *   encode_bwd (cotangents g_z [rows, D] and g_lq [rows], either may be NULL = zero, not both): d_h [batch, 2 D] with
 *              d_mean[b, j] = sum_s g_z[n, j],  d_lv[b, j] = sum_s (exp(lv / 2) eps g_z / 2 - g_lq[n] / 2); eps gets no
 *              gradient
 *   gauss_log_prob (v [rows / v_div, D], h [rows / h_div, 2 D]):
 *              logp[n] = -D/2 log 2 pi - 1/2 sum_j (lv + (v - mean)^2 exp(-lv))
 *              the encoder's log_prob(z, x) is v_div = 1, h_div = samples; the Gaussian decoder v_div = samples,
 *              h_div = 1.  Both divisors >= 1, min(v_div, h_div) == 1 and rows divisible by both, else VCNF_ERR_SHAPE
 *   gauss_log_prob_bwd (cotangent g_lp [rows]; d_v and d_h shaped like v and h, either may be NULL, not both): with
 *              r = (v - mean) exp(-lv):  d_v = -g r,  d_mean = g r,  d_lv = g (r (v - mean) / 2 - 1 / 2); the operand
 *              with divisor 1 is written row by row, the other is summed over its rows
 *   bernoulli_log_prob (x [rows / x_div, D] with values in [0, 1], score [rows, D]):
 *              logp[n] = sum_j (x ls(a) + (1 - x) ls(-a)),  ls(a) = -max(-a, 0) - log1p(exp(-|a|))
 *   bernoulli_log_prob_bwd: d_score [rows, D] = g (x - sigmoid(a)), the sigmoid in the form that never exponentiates a
 *              positive number; x gets no gradient
 * Forward: a lane group per row, the row in chunks of 16 bytes' worth of columns strided over the group; 16-byte
 * (8-byte) accesses when features % V == 0 and the [., D] / [., 2 D] buffers are aligned to them, scalar otherwise,
 * with the same bits either way.  VJPs: a lane per (item, column) walks the item's rows in ascending order, the shared
 * operand's gradient in a register: a fixed-order sum, no atomics, no workspace, no allocation, no host
 * synchronisation - every call is bitwise reproducible and capturable.  No kernel loops over the grid: a shape that
 * needs more than 2^31 - 1 workgroups -> VCNF_ERR_SHAPE.
 * Checked in this order: NULL required pointer -> VCNF_ERR_NULL; features < 1, samples < 1, a negative count or the
 * divisor rules -> VCNF_ERR_SHAPE; batch == 0 / rows == 0 -> VCNF_OK without a launch; a pointer not aligned to its
 * element size -> VCNF_ERR_ALIGN; in the _bwd entry points samples (the divisor) > VCNF_VAE_MAX_SAMPLES ->
 * VCNF_ERR_UNSUPPORTED (one lane walks them: a mistaken argument must not become a launch that runs for minutes).  The
 * forward entry points take any divisor. */
enum { VCNF_VAE_MAX_SAMPLES = 4096 };
int vcnf_vae_encode_f32(const float* h, const float* eps, float* z, float* logq, int64_t batch, int32_t samples,
                        int32_t features, void* stream);
int vcnf_vae_encode_bwd_f32(const float* h, const float* eps, const float* g_z, const float* g_lq, float* d_h,
                            int64_t batch, int32_t samples, int32_t features, void* stream);
int vcnf_vae_gauss_log_prob_f32(const float* v, const float* h, float* logp, int64_t rows, int32_t v_div, int32_t h_div,
                                int32_t features, void* stream);
int vcnf_vae_gauss_log_prob_bwd_f32(const float* v, const float* h, const float* g_lp, float* d_v, float* d_h,
                                    int64_t rows, int32_t v_div, int32_t h_div, int32_t features, void* stream);
int vcnf_vae_bernoulli_log_prob_f32(const float* x, const float* score, float* logp, int64_t rows, int32_t x_div,
                                    int32_t features, void* stream);
int vcnf_vae_bernoulli_log_prob_bwd_f32(const float* x, const float* score, const float* g_lp, float* d_score,
                                        int64_t rows, int32_t x_div, int32_t features, void* stream);
int vcnf_vae_encode_f64(const double* h, const double* eps, double* z, double* logq, int64_t batch, int32_t samples,
                        int32_t features, void* stream);
int vcnf_vae_encode_bwd_f64(const double* h, const double* eps, const double* g_z, const double* g_lq, double* d_h,
                            int64_t batch, int32_t samples, int32_t features, void* stream);
int vcnf_vae_gauss_log_prob_f64(const double* v, const double* h, double* logp, int64_t rows, int32_t v_div,
                                int32_t h_div, int32_t features, void* stream);
int vcnf_vae_gauss_log_prob_bwd_f64(const double* v, const double* h, const double* g_lp, double* d_v, double* d_h,
                                    int64_t rows, int32_t v_div, int32_t h_div, int32_t features, void* stream);
int vcnf_vae_bernoulli_log_prob_f64(const double* x, const double* score, double* logp, int64_t rows, int32_t x_div,
                                    int32_t features, void* stream);
int vcnf_vae_bernoulli_log_prob_bwd_f64(const double* x, const double* score, const double* g_lp, double* d_score,
                                        int64_t rows, int32_t x_div, int32_t features, void* stream);

/* ---- Circular flows: the periodic maps of normflow 1.2's flows/periodic.py (PeriodicWrap, PeriodicShift) and the
 * UniformGaussian base of its distributions/base.py (csrc/periodic.hip).  Rows of `features` = D contiguous columns.
 *   periodic (z, out [n_rows, D]; half [D]; shift [D] or NULL = no shift): a column with half[j] == 0 is copied; on
 *              the others, with bound = half[j] > 0 and s = sign * shift[j], in the element type and in this order
 *                a = (z + s) + bound;  r = fmod(a, 2 * bound);  if (r != 0 && r < 0) r += 2 * bound;  out = r - bound
 *              No step is contracted or reordered, so out has the bits of torch.remainder(z + s + bound, 2 * bound) -
 *              bound.  sign is +1 for PeriodicShift.forward and -1 for its inverse.  out == z is allowed (in place).
 *              Both maps have derivative 1 and log-det 0: there is nothing else to compute.
 *   uniform_gaussian_log_prob (z [batch, D], inv_scale_g [D]):
 *              logp[b] = const_term - 0.5 * sum_j (z[b, j] * inv_scale_g[j])^2
 *              inv_scale_g is 1 / scale on a Gaussian column and 0 on a uniform one (the uniform part does not test
 *              its range); const_term = -sum_j log scale_j - 0.5 * (number of Gaussian columns) * log(2 pi), which the
 *              caller evaluates in fp64.  ld_mode: VCNF_LD_STORE or VCNF_LD_ACCUM (logp[b] += ...)
 *   uniform_gaussian_sample (eps [batch, D] in the order drawn, src [D] int32, offset, scale, inv_scale_g [D]):
 *              z[b, j] = scale[j] * (eps[b, src[j]] - offset[j])  (offset 0.5 where src[j] is a uniform draw, else 0)
 *              and logp[b] of that z as above, in the same launch.  A src[j] outside [0, D) gives NaN, never a read
 *              outside the row
 *   uniform_gaussian_log_prob_bwd (cotangent g [batch]):  d_z[b, j] = -g[b] * z[b, j] * inv_scale_g[j]^2
 * A lane group per row, the row in chunks of 16 bytes' worth of columns strided over the group, a lane's columns added
 * in ascending order and the group by the ascending butterfly; 16-byte (8-byte) accesses when features % V == 0 and
 * the row buffers and tables are aligned to them, scalar otherwise, with the same bits either way.  Any number of
 * features.  No kernel loops over the grid: a shape that needs more than 2^31 - 1 workgroups -> VCNF_ERR_SHAPE.
 * Checked in this order: NULL required pointer -> VCNF_ERR_NULL; features < 1, a negative count, or work beyond a grid
 * -> VCNF_ERR_SHAPE; unknown ld_mode -> VCNF_ERR_UNSUPPORTED; n_rows == 0 / batch == 0 -> VCNF_OK without a launch; a
 * pointer not aligned to its element size -> VCNF_ERR_ALIGN.  No atomics, no allocation, no host synchronisation:
 * every call is bitwise reproducible and capturable. */
int vcnf_periodic_f32(const float* z, const float* half, const float* shift, float* out, int64_t n_rows,
                      int32_t features, float sign, void* stream);
int vcnf_uniform_gaussian_log_prob_f32(const float* z, const float* inv_scale_g, float const_term, float* logp,
                                       int64_t batch, int32_t features, int ld_mode, void* stream);
int vcnf_uniform_gaussian_sample_f32(const float* eps, const int32_t* src, const float* offset, const float* scale,
                                     float const_term, const float* inv_scale_g, float* z, float* logp, int64_t batch,
                                     int32_t features, void* stream);
int vcnf_uniform_gaussian_log_prob_bwd_f32(const float* z, const float* inv_scale_g, const float* g, float* d_z,
                                           int64_t batch, int32_t features, void* stream);
int vcnf_periodic_f64(const double* z, const double* half, const double* shift, double* out, int64_t n_rows,
                      int32_t features, double sign, void* stream);
int vcnf_uniform_gaussian_log_prob_f64(const double* z, const double* inv_scale_g, double const_term, double* logp,
                                       int64_t batch, int32_t features, int ld_mode, void* stream);
int vcnf_uniform_gaussian_sample_f64(const double* eps, const int32_t* src, const double* offset, const double* scale,
                                     double const_term, const double* inv_scale_g, double* z, double* logp,
                                     int64_t batch, int32_t features, void* stream);
int vcnf_uniform_gaussian_log_prob_bwd_f64(const double* z, const double* inv_scale_g, const double* g, double* d_z,
                                           int64_t batch, int32_t features, void* stream);

/* ---- Image data end caps: the Logit transform of normflow 1.2's transforms.py and the byte ingest in front of it
 * (csrc/logit.hip).  Rows of `features` = D contiguous elements (all axes of an item but the first); alpha in [0, 0.5)
 * and beta = 1 - 2 alpha are passed / formed in fp64 and rounded to the element type once, as torch rounds a Python
 * scalar operand; every step below is rounded once in the element type and none is contracted into an fma.
 *   logit_inverse (x, z [batch, D]; the density direction):
 *              u = alpha + beta * x (a multiply, then an add);  z = log(u) - log(1 - u)
 *              ld[b] = D log(beta) - sum_j log(u) - sum_j log(1 - u)
 *              With alpha = 0, x = 0 gives z = -inf, x = 1 gives z = +inf and either gives ld = +inf, never NaN.
 *   logit_forward (z, y [batch, D]; the sampling direction):  with s = sigmoid(z)
 *              y = (s - alpha) / beta;  ld[b] = -D log(beta) + sum_j (-|z| - 2 log1p(exp(-|z|)))
 *              the sum's term is logsigmoid(z) + logsigmoid(-z): finite for every finite z, -inf at +-inf
 *   logit_inverse_u8 (bytes [batch, D] uint8, noise [batch, D] uniform on [0, 1) drawn by the caller):
 *              x = ((T(byte) / 255) + noise * jitter) * scale, one rounded operation at a time, then logit_inverse of
 *              that x in the same launch: one byte and one noise value are read per element, x is never stored
 *   logdet[b] = ld_sign * ld[b] (VCNF_LD_STORE) or logdet[b] + ld_sign * ld[b] (VCNF_LD_ACCUM).  z == x / y == z is
 *              allowed (in place).
 *   logit_inverse_bwd (cotangents g_z [batch, D], g_ld [batch]; either may be NULL = zero), recomputing u from x:
 *              d_x = beta / (u (1 - u)) * (g_z - g_ld[b] * (1 - 2 u))
 *   logit_forward_bwd (cotangents g_y [batch, D], g_ld [batch]; either may be NULL = zero), recomputing s from z:
 *              d_z = g_y * (s (1 - s) / beta) + g_ld[b] * (1 - 2 s)
 * A lane group per row, the row in chunks of 16 bytes' worth of elements strided over the group (at features = 3072 a
 * row is 12 trips of a 64-lane group, at features = 1 a lane owns a row), a lane's elements added in ascending order and
 * the group by the ascending butterfly; 16-byte (8-byte) accesses when features % V == 0 and the row buffers are aligned
 * to them, scalar otherwise, with the same bits either way.  Any number of features.  The grid is NOT capped and no
 * kernel loops over it, as in csrc/periodic.hip (the row-sum kernels of csrc/affine_kernels.hip cap theirs and loop): a
 * shape that needs more than 2^31 - 1 workgroups -> VCNF_ERR_SHAPE.
 * Checked in this order: NULL required pointer -> VCNF_ERR_NULL; features < 1, a negative count, or work beyond a grid
 * -> VCNF_ERR_SHAPE; unknown ld_mode -> VCNF_ERR_UNSUPPORTED; batch == 0 -> VCNF_OK without a launch; a pointer not
 * aligned to its element size -> VCNF_ERR_ALIGN.  No atomics, no allocation, no host synchronisation: every call is
 * bitwise reproducible and capturable. */
int vcnf_logit_inverse_f32(const float* x, double alpha, float* z, float* logdet, int64_t batch, int32_t features,
                           int ld_mode, float ld_sign, void* stream);
int vcnf_logit_forward_f32(const float* z, double alpha, float* y, float* logdet, int64_t batch, int32_t features,
                           int ld_mode, float ld_sign, void* stream);
int vcnf_logit_inverse_bwd_f32(const float* x, double alpha, const float* g_z, const float* g_ld, float* d_x,
                               int64_t batch, int32_t features, void* stream);
int vcnf_logit_forward_bwd_f32(const float* z, double alpha, const float* g_y, const float* g_ld, float* d_z,
                               int64_t batch, int32_t features, void* stream);
int vcnf_logit_inverse_u8_f32(const uint8_t* bytes, const float* noise, double jitter, double scale, double alpha,
                              float* z, float* logdet, int64_t batch, int32_t features, int ld_mode, float ld_sign,
                              void* stream);
int vcnf_logit_inverse_f64(const double* x, double alpha, double* z, double* logdet, int64_t batch, int32_t features,
                           int ld_mode, double ld_sign, void* stream);
int vcnf_logit_forward_f64(const double* z, double alpha, double* y, double* logdet, int64_t batch, int32_t features,
                           int ld_mode, double ld_sign, void* stream);
int vcnf_logit_inverse_bwd_f64(const double* x, double alpha, const double* g_z, const double* g_ld, double* d_x,
                               int64_t batch, int32_t features, void* stream);
int vcnf_logit_forward_bwd_f64(const double* z, double alpha, const double* g_y, const double* g_ld, double* d_z,
                               int64_t batch, int32_t features, void* stream);
int vcnf_logit_inverse_u8_f64(const uint8_t* bytes, const double* noise, double jitter, double scale, double alpha,
                              double* z, double* logdet, int64_t batch, int32_t features, int ld_mode, double ld_sign,
                              void* stream);

/* ---- Categorical columns: uniform and variational dequantisation (Ho et al. 2019) per column and the reverse map to
 * integer codes (csrc/dequant.hip).  Rows x / z / out [batch, D] contiguous, D = features; C = n_cat <= D of the columns
 * are categorical.  slot [D] int32 (device) holds -1 for a continuous column and otherwise the column's index c into the
 * [batch, C] operands (u, v, ctx, w, d_w); levels [C] int32 (device) holds K_c >= 1.  A categorical column holds the
 * integer codes 0 .. K_c - 1 as floating values k.  a = alpha in [0, 1) crosses in fp64; a/2, 1 - a and log(1 - a) are
 * formed in fp64 and rounded to the element type once, as torch rounds a Python scalar operand; K = K_c converted to the
 * element type; every step below is rounded once in the element type and none is contracted into an fma.
 *   dequant_prepare (u [batch, C] uniform on [0, 1) drawn by the caller -> v, ctx [batch, C]):
 *              s = a/2 + (1 - a) u;  v = log(s) - log(1 - s);  ctx = 2 k / (K - 1) - 1, and 0 where K = 1
 *              ld[b] = sum_c ((log(1 - a) - log(s)) - log(1 - s))
 *   dequant_merge (w [batch, C] -> out [batch, D]; the density direction):
 *              noise_is_logit != 0:  n = 1 / (1 + exp(-w)),  ld_n = sum_c (-|w| - 2 log1p(exp(-|w|)))
 *                                    (the term is logsigmoid(w) + logsigmoid(-w))
 *              noise_is_logit == 0:  n = w,  ld_n = 0
 *              y = (k + n) / K;  s = a/2 + (1 - a) y;  out[:, col_c] = log(s) - log(1 - s);  a continuous column of out is
 *              that column of x, bit for bit
 *              ld[b] = ld_n + sum_c (((log(1 - a) - log(K)) - log(s)) - log(1 - s))
 *   dequant_merge_bwd (cotangents g_out [batch, D], g_ld [batch]; either may be NULL = zero), recomputing n and s from x
 *              and w:  d_n = ((1 - a) / K) / (s (1 - s)) * (g_out[:, col_c] - g_ld[b] (1 - 2 s))
 *              noise_is_logit != 0:  d_w = d_n (n (1 - n)) + g_ld[b] (1 - 2 n);   else d_w = d_n
 *              d_x [batch, D] (may be NULL: not written) = g_out on a continuous column, 0 on a categorical one
 *   quantize (z -> out [batch, D]; the sampling direction):  t = z[:, col_c],  sg = 1 / (1 + exp(-t))
 *              y = (sg - a/2) / (1 - a);  out[:, col_c] = min(max(floor(y K), 0), K - 1);  other columns copied
 *              ld[b] = sum_c (((-|t| - 2 log1p(exp(-|t|))) - log(1 - a)) + log(K)),  the log-det of t -> y K
 *   logdet[b] = ld_sign * ld[b] (VCNF_LD_STORE) or logdet[b] + ld_sign * ld[b] (VCNF_LD_ACCUM).  out must not overlap x / z.
 * The kernels do not test that a code is integral or in range: an out-of-range or fractional code gives the formula's
 * value.  A level < 1 cannot be seen on the host and is the caller's business, as is a slot outside -1 .. C - 1.
 * A lane group per row, the row in chunks of 16 bytes' worth of columns strided over the group (at features = 14 in fp32
 * four lanes share a row, at features <= 4 a lane owns one), a lane's terms added in ascending column order and the
 * group by the ascending butterfly: two calls give the same bits.  The [batch, D] buffers move in 16-byte (8-byte)
 * accesses when features % V == 0 and they are aligned to them, scalar otherwise, with the same bits either way; the
 * [batch, C] operands move one element at a time.  At most 4096 workgroups; a lane group walks further rows one grid
 * of rows apart.  Any number of features, any n_cat <= features.
 * Checked in this order: NULL required pointer -> VCNF_ERR_NULL; features < 1, n_cat < 0, n_cat > features, a negative
 * batch or batch * features beyond int64 -> VCNF_ERR_SHAPE; a pointer not aligned to its element size ->
 * VCNF_ERR_ALIGN; unknown ld_mode -> VCNF_ERR_UNSUPPORTED; batch == 0 -> VCNF_OK without a launch.  No atomics, no
 * random numbers, no allocation, no host synchronisation: every call is bitwise reproducible and capturable. */
int vcnf_dequant_prepare_f32(const float* x, const int32_t* slot, const int32_t* levels, const float* u, double alpha,
                             float* v, float* ctx, float* logdet, int64_t batch, int32_t features, int32_t n_cat,
                             int ld_mode, float ld_sign, void* stream);
int vcnf_dequant_merge_f32(const float* x, const int32_t* slot, const int32_t* levels, const float* w,
                           int noise_is_logit, double alpha, float* out, float* logdet, int64_t batch, int32_t features,
                           int32_t n_cat, int ld_mode, float ld_sign, void* stream);
int vcnf_dequant_merge_bwd_f32(const float* x, const int32_t* slot, const int32_t* levels, const float* w,
                               int noise_is_logit, double alpha, const float* g_out, const float* g_ld, float* d_w,
                               float* d_x, int64_t batch, int32_t features, int32_t n_cat, void* stream);
int vcnf_quantize_f32(const float* z, const int32_t* slot, const int32_t* levels, double alpha, float* out,
                      float* logdet, int64_t batch, int32_t features, int32_t n_cat, int ld_mode, float ld_sign,
                      void* stream);
int vcnf_dequant_prepare_f64(const double* x, const int32_t* slot, const int32_t* levels, const double* u, double alpha,
                             double* v, double* ctx, double* logdet, int64_t batch, int32_t features, int32_t n_cat,
                             int ld_mode, double ld_sign, void* stream);
int vcnf_dequant_merge_f64(const double* x, const int32_t* slot, const int32_t* levels, const double* w,
                           int noise_is_logit, double alpha, double* out, double* logdet, int64_t batch,
                           int32_t features, int32_t n_cat, int ld_mode, double ld_sign, void* stream);
int vcnf_dequant_merge_bwd_f64(const double* x, const int32_t* slot, const int32_t* levels, const double* w,
                               int noise_is_logit, double alpha, const double* g_out, const double* g_ld, double* d_w,
                               double* d_x, int64_t batch, int32_t features, int32_t n_cat, void* stream);
int vcnf_quantize_f64(const double* z, const int32_t* slot, const int32_t* levels, double alpha, double* out,
                      double* logdet, int64_t batch, int32_t features, int32_t n_cat, int ld_mode, double ld_sign,
                      void* stream);

/* ---- Full-covariance base distributions: the multivariate Gaussian and the multivariate Student-t over D = features
 * <= 128.  z / eps [B, D] contiguous, gamma [B], loc [D]; tri [D, D] row-major is a lower-triangular matrix of which
 * only the lower triangle including the diagonal is ever read: the scale L for sampling, its inverse M = L^-1 for the
 * density.  consts [2] = (cst, nu) on the device, cst = the normaliser - sum log diag L (Gaussian: -D/2 log 2 pi;
 * Student-t: lgamma((nu+D)/2) - lgamma(nu/2) - D/2 log(nu pi)); nu is ignored by the Gaussian.  The caller inverts L
 * and evaluates cst: no kernel solves or calls lgamma, and the caller draws the random numbers.  With x = z - loc,
 * y = M x, q = |y|^2:
 *   f(q) = -q / 2                        VCNF_MVN_GAUSSIAN
 *   f(q) = -(nu + D)/2 log1p(q / nu)     VCNF_MVN_STUDENT_T
 *   log_prob:  logp[b] = sign * (cst + f(q))   (ld_mode as for vcnf_tail_log_prob_*)
 *   sample:    z[b] = loc + s L eps with s = 1, or s = sqrt(nu / (2 gamma[b])) with gamma ~ Gamma(nu/2, 1) (gamma is
 *              required for the Student-t and ignored, possibly NULL, for the Gaussian); logp[b] = cst + f(s^2 |eps|^2),
 *              the log density of that z without a solve
 *   log_prob_bwd (cotangent g[B], gz_in[B, D] or NULL): with c = g 2 df/dq (df/dq = -1/2, or -(nu+D)/(2(nu+q))),
 *              dz = gz_in + c M^T y, and per workgroup k one block partials[k] [D D + D + 1] with the workgroup's share
 *              of  Y = tril(sum_b c y y^T) as a full square with zeros above the diagonal | d_loc = -sum_b c M^T y
 *              | sum_b g (-log1p(q/nu)/2 + (nu+D) q / (2 nu (nu+q))), the part of d_nu that does not go through cst (0
 *              for the Gaussian).  d_cst = sum_b g is the caller's, and so is the step from the symmetric sum to the
 *              gradient of L: d_L = -tril(M^T (Y + strict(Y)^T)).  (The gradient of M itself, sum_b c y x^T = Y L^T, is
 *              not what is summed: the way from it to d_L undoes the factor L^T and multiplies the sum's rounding by
 *              cond(L).)  partials has vcnf_mvn_bwd_groups(batch, D) blocks,
 *              every block is written in full; partials == NULL: only dz is computed
 *   sample_bwd (cotangents g_z[B, D] and g_lp[B], either may be NULL = zero): with w = L^T g_z and k = g_lp 2 df/dq,
 *              deps = s w + k s^2 eps (deps may be NULL), ds = w.eps + k s |eps|^2, dgamma[b] = -ds s / (2 gamma)
 *              (Student-t only; the Gaussian writes none and takes NULL), and blocks as above with  d_tri =
 *              tril(sum_b s g_z eps^T) | d_loc = sum_b g_z | d_nu = sum_b (ds s / (2 nu) + g_lp df/dnu at fixed q)
 *   reduce_partials: d_loc [D], d_tri [D, D], d_nu [1] = the sum of `groups` blocks in a fixed order
 * vcnf_mvn_bwd_groups is a pure function of its arguments (no device query; 0 for an unsupported shape): one workgroup
 * per 64 samples, at most 256, and at most 2^22 elements of partial blocks in all (16 MiB in fp32, 32 MiB in fp64).
 * Workgroup k takes the sample tiles k, k + groups, ...: every sum's order is fixed by the shape alone.
 * 1 <= features <= VCNF_MVN_MAX_DIM and batch >= 0, else VCNF_ERR_SHAPE (groups < 1 as well); unknown family or
 * ld_mode -> VCNF_ERR_UNSUPPORTED; batch == 0 -> VCNF_OK without a launch; NULL required pointer -> VCNF_ERR_NULL; a
 * pointer not aligned to its element size -> VCNF_ERR_ALIGN.
 * 16-byte (8-byte) accesses are used when features % V == 0 and the
 * [B, D] buffers are aligned to them.  No atomics, no allocation, no host synchronisation: every call is bitwise
 * reproducible and capturable. */
enum { VCNF_MVN_GAUSSIAN = 0, VCNF_MVN_STUDENT_T = 1 };
enum { VCNF_MVN_MAX_DIM = 128 };
int64_t vcnf_mvn_bwd_groups(int64_t batch, int32_t features);
int vcnf_mvn_log_prob_f32(const float* z, const float* loc, const float* tri_inv, const float* consts, float* logp,
                          int64_t batch, int32_t features, int family, int ld_mode, float sign, void* stream);
int vcnf_mvn_sample_f32(const float* eps, const float* gamma, const float* loc, const float* tri, const float* consts,
                        float* z, float* logp, int64_t batch, int32_t features, int family, void* stream);
int vcnf_mvn_log_prob_bwd_f32(const float* z, const float* loc, const float* tri_inv, const float* consts,
                              const float* g, const float* gz_in, float* dz, float* partials, int64_t batch,
                              int32_t features, int family, void* stream);
int vcnf_mvn_sample_bwd_f32(const float* eps, const float* gamma, const float* tri, const float* consts,
                            const float* g_z, const float* g_lp, float* deps, float* dgamma, float* partials,
                            int64_t batch, int32_t features, int family, void* stream);
int vcnf_mvn_reduce_partials_f32(const float* partials, int64_t groups, int32_t features, float* d_loc, float* d_tri,
                                 float* d_nu, void* stream);
int vcnf_mvn_log_prob_f64(const double* z, const double* loc, const double* tri_inv, const double* consts, double* logp,
                          int64_t batch, int32_t features, int family, int ld_mode, double sign, void* stream);
int vcnf_mvn_sample_f64(const double* eps, const double* gamma, const double* loc, const double* tri,
                        const double* consts, double* z, double* logp, int64_t batch, int32_t features, int family,
                        void* stream);
int vcnf_mvn_log_prob_bwd_f64(const double* z, const double* loc, const double* tri_inv, const double* consts,
                              const double* g, const double* gz_in, double* dz, double* partials, int64_t batch,
                              int32_t features, int family, void* stream);
int vcnf_mvn_sample_bwd_f64(const double* eps, const double* gamma, const double* tri, const double* consts,
                            const double* g_z, const double* g_lp, double* deps, double* dgamma, double* partials,
                            int64_t batch, int32_t features, int family, void* stream);
int vcnf_mvn_reduce_partials_f64(const double* partials, int64_t groups, int32_t features, double* d_loc, double* d_tri,
                                 double* d_nu, void* stream);

/* ---- A run of Planar and Radial layers (normflow/flows/planar.py, radial.py) in one launch, with its VJP
 * (csrc/planar_radial.hip).  z / out [B, D] contiguous, D = features <= 256 (vcnf_planar_radial_supported), K =
 * n_layers >= 1 without an upper limit.  The layers arrive in the order they are applied, as EFFECTIVE operands the
 * caller computes (no parameter formula lives in a kernel):
 *   kind [K] int32   VCNF_PLANAR_TANH, VCNF_PLANAR_LEAKY (leaky_relu) or VCNF_RADIAL.  Given twice: `kind` in HOST
 *                    memory, validated before anything is launched, and `kind_dev`, the same values on the device,
 *                    read by the kernel.
 *                    That the two agree is the CALLER'S contract and is not checked (checking would read device
 *                    memory back): with differing copies the validation passes for layers other than those the kernel
 *                    runs, e.g. the inverse on a kind it does not have, or a read of a NULL vb
 *   va [K, D]        planar: u_hat = u + (log(1 + exp(w.u)) - 1 - w.u) w / |w|^2;  radial: z_0
 *   vb [K, D]        planar: w;  radial rows are not read (NULL is accepted when every kind is 2)
 *   sc [K, 2]        planar: (b, negative slope);  radial: (|alpha|, beta_eff = log(1 + exp(beta)) - |alpha|)
 *   forward  planar: lin = w.z + b, z' = z + u_hat h(lin), ld = log|1 + (w.u_hat) h'(lin)|  (h = tanh, or leaky_relu)
 *            radial: r = |z - z_0|, h = beta_eff / (|alpha| + r), h' = -beta_eff r / (|alpha| + r)^2,
 *                    z' = z + h (z - z_0), ld = (D - 1) log(1 + h) + log(1 + h + h')
 *   inverse != 0 (every kind must be 1): lin = w.z + b, a = 1 or the slope where lin < 0, s = a (w.u_hat),
 *            z' = z - a u_hat lin / (1 + s), ld = -log|1 + s|
 *   logdet[b] = ld_sign * (sum of the layers' ld), stored or accumulated (ld_mode).  trace [K, B] (may be NULL)
 *   receives lin of a planar layer and r of a radial layer.  checkpoints [(K - 1) / C, B, D] with C =
 *   vcnf_planar_radial_checkpoint_every(D) = max(ceil(D / 8), 4) (may be NULL) receives the row as it enters the layers C,
 *   2 C, ...: at most 8 K elements per sample.
 *   stack_bwd: VJP of the forward run from its output z_out, its trace and the cotangents g_out [B, D] and g_logdet
 *            [B] of (out, sum of ld) - either may be NULL = zero; checkpoints as the forward run wrote them, or NULL
 *            (then every layer's input is rebuilt, and the rounding of z_out grows across the moving direction of
 *            contracting radial layers: by 1 / (1 + h) per layer): g_in [B, D], g_va [K, D], g_vb [K, D] (zero rows for
 *            radial layers) and g_sc [K, 2] (the slope's entry is zero).  One launch walks the layers from last to
 *            first, rebuilding each layer's input from its output and the trace; every workgroup adds its samples'
 *            parameter terms into its own block of `workspace` (vcnf_planar_radial_bwd_groups(batch, D, K) blocks of
 *            K (2 D + 2) elements, uninitialised on entry) and a second launch adds the blocks in a fixed order.
 * vcnf_planar_radial_bwd_groups is a pure function of its arguments (no device query; 0 for an unsupported shape):
 * at most 1024, and at most 2^22 workspace elements while one block fits in that.
 * NULL required pointer -> VCNF_ERR_NULL; batch < 0, features outside 1 .. 256 or n_layers < 1 -> VCNF_ERR_SHAPE; a
 * pointer not aligned to its element size -> VCNF_ERR_ALIGN; unknown kind or ld_mode, or inverse with a kind other than
 * 1 -> VCNF_ERR_UNSUPPORTED; batch == 0 -> VCNF_OK without a launch.  16-byte (8-byte) accesses are used when
 * features % V == 0 and the [., D] buffers are aligned to them.  No atomics, no allocation, no host synchronisation:
 * every call is bitwise reproducible and capturable. */
enum { VCNF_PLANAR_TANH = 0, VCNF_PLANAR_LEAKY = 1, VCNF_RADIAL = 2 };
int vcnf_planar_radial_supported(int32_t features);
int32_t vcnf_planar_radial_checkpoint_every(int32_t features);
int64_t vcnf_planar_radial_bwd_groups(int64_t batch, int32_t features, int32_t n_layers);
int vcnf_planar_radial_stack_f32(const float* z, float* out, float* logdet, float* trace, float* checkpoints,
                                 const int32_t* kind, const int32_t* kind_dev, const float* va, const float* vb,
                                 const float* sc, int64_t batch, int32_t features, int32_t n_layers, int inverse,
                                 int ld_mode, float ld_sign, void* stream);
int vcnf_planar_radial_stack_bwd_f32(const float* z_out, const float* trace, const float* checkpoints,
                                     const float* g_out, const float* g_logdet, const int32_t* kind,
                                     const int32_t* kind_dev, const float* va, const float* vb, const float* sc,
                                     float* g_in, float* g_va, float* g_vb, float* g_sc, float* workspace,
                                     int64_t batch, int32_t features, int32_t n_layers, void* stream);
int vcnf_planar_radial_stack_f64(const double* z, double* out, double* logdet, double* trace, double* checkpoints,
                                 const int32_t* kind, const int32_t* kind_dev, const double* va, const double* vb,
                                 const double* sc, int64_t batch, int32_t features, int32_t n_layers, int inverse,
                                 int ld_mode, double ld_sign, void* stream);
int vcnf_planar_radial_stack_bwd_f64(const double* z_out, const double* trace, const double* checkpoints,
                                     const double* g_out, const double* g_logdet, const int32_t* kind,
                                     const int32_t* kind_dev, const double* va, const double* vb, const double* sc,
                                     double* g_in, double* g_va, double* g_vb, double* g_sc, double* workspace,
                                     int64_t batch, int32_t features, int32_t n_layers, void* stream);

/* ---- Target densities: the 2-D targets of normflow 1.2 (distributions/target.py) with their score, one launch
 * (csrc/target_density.hip).  z [B, 2] contiguous, logp [B], score [B, 2] = d logp / d z or NULL (then none of the
 * score's arithmetic runs).  With r = sqrt(z0^2 + z1^2) and a = |z0|:
 *   VCNF_TARGET_TWO_MOONS     logp = -((r - 2) / 0.2)^2 / 2 - ((a - 2) / 0.3)^2 / 2 + log1p(e),  e = exp(-4 a / 0.09)
 *                             score0 = -(r - 2) / 0.04 z0 / r + sign(z0) ((2 - a) / 0.09 - (4 / 0.09) e / (1 + e))
 *                             score1 = -(r - 2) / 0.04 z1 / r
 *                             table, n_comp and scale are ignored (table may be NULL)
 *   VCNF_TARGET_CIRCULAR_GMM  table [n_comp, 2] the centres c_i (upstream: 2 (sin, cos)(2 pi i / n)),
 *                             d_i = |z - c_i|^2 / (2 scale^2),  logp = -log(2 pi scale^2 n_comp) + logsumexp_i(-d_i)
 *                             score = sum_i softmax_i(-d) (c_i - z) / scale^2
 *   VCNF_TARGET_RING_MIXTURE  table [n_comp] the radii t_i (upstream: 2 (i + 1) / n),
 *                             d_i = (r - t_i)^2 / (2 scale^2),  logp = logsumexp_i(-d_i)
 *                             score = sum_i softmax_i(-d) (t_i - r) / scale^2 z / r
 * The energy densities of normflow 1.2's distributions/prior.py (the test energies of Rezende & Mohamed) are families
 * of the same entry points.  `scale` is the density's scale s and `table` holds its other constants, device memory of
 * the call's type read at fixed indices.  With q = (20 s)^4, om = 2 pi / period, w1 = sin(om z0), w1' = om cos(om z0),
 * d = z1 - w1 and u(z) = z / r:
 *   VCNF_TARGET_TWO_MODES     table {loc} (n_comp >= 1); eps = |loc|, c1 = 2 s, c2 = 3 s, e = exp(-2 a eps / c2^2)
 *                             logp = -((r - loc) / c1)^2 / 2 - ((a - eps) / c2)^2 / 2 + log1p(e)
 *                             score0 = -(r - loc) / c1^2 u(z0) + sign(z0) ((eps - a) / c2^2 - (2 eps / c2^2) e / (1 + e))
 *                             score1 = -(r - loc) / c1^2 u(z1)
 *   VCNF_TARGET_SINUSOIDAL    table {period} (n_comp >= 1)
 *                             logp = -(d / s)^2 / 2 - (z0^4 + z1^4) / (2 q)
 *                             score0 = d w1' / s^2 - 2 z0^3 / q,   score1 = -d / s^2 - 2 z1^3 / q
 *   VCNF_TARGET_SINUSOIDAL_GAP    table {period, amp, mu, width} (n_comp >= 4; upstream: amp 3, mu 1, width 0.6)
 *                             w = amp exp(-((z0 - mu) / width)^2 / 2),  w' = -w (z0 - mu) / width^2
 *                             a = -(d / s)^2 / 2,  b = -((d + w) / s)^2 / 2,  pb = sigmoid(b - a),  pa = 1 - pb
 *                             logp = logaddexp(a, b) - (z0^4 + z1^4) / (2 q)
 *                             score0 = (pa d w1' + pb (d + w) (w1' - w')) / s^2 - 2 z0^3 / q
 *                             score1 = -(pa d + pb (d + w)) / s^2 - 2 z1^3 / q
 *   VCNF_TARGET_SINUSOIDAL_SPLIT  the same with w = amp sigmoid((z0 - mu) / width),  w' = w (1 - w / amp) / width
 *                             (upstream: amp 3, mu 1, width 0.3)
 *   VCNF_TARGET_SMILEY        c = 2 s,  t = |z1 + 0.8|;  table and n_comp are ignored (table may be NULL)
 *                             logp = -((r - 2) / c)^2 / 2 - ((t - 1.2) / c)^2 / 2
 *                             score0 = -(r - 2) / c^2 u(z0),   score1 = -(r - 2) / c^2 u(z1) - sign(z1 + 0.8) (t - 1.2) / c^2
 * The logaddexp subtracts its larger branch and pb comes from the same exp(-|b - a|): finite wherever a and b are,
 * where log(exp a + exp b) is -inf in fp32 a few |d| / s out.  scale == 0 and period == 0 are the caller's business.
 * The caller computes the table.  Every z / r is 0 at r == 0 (torch's gradient of norm there) and sign(0) = 0; a
 * non-finite z gives NaN logp and score.  The logsumexp subtracts its maximum in two passes over the components; no
 * buffer of size [B, n_comp] exists and n_comp has no upper limit.  One sample per lane; a row moves as one 8-byte
 * (16-byte) access when z and score are aligned to it, as two elements otherwise, with the same bits either way.
 * logp does not depend on whether score is given, bit for bit.
 * batch < 0, or n_comp below what the family reads (1 for a mixture) -> VCNF_ERR_SHAPE; unknown family ->
 * VCNF_ERR_UNSUPPORTED; batch == 0 -> VCNF_OK without a launch; NULL z or logp, or NULL table for a family that reads
 * one -> VCNF_ERR_NULL; a pointer not aligned to its element size -> VCNF_ERR_ALIGN.  No atomics, no allocation, no
 * host synchronisation: every call is bitwise reproducible and capturable. */
enum {
  VCNF_TARGET_TWO_MOONS = 0, VCNF_TARGET_CIRCULAR_GMM = 1, VCNF_TARGET_RING_MIXTURE = 2,
  VCNF_TARGET_TWO_MODES = 16, VCNF_TARGET_SINUSOIDAL = 17, VCNF_TARGET_SINUSOIDAL_GAP = 18,
  VCNF_TARGET_SINUSOIDAL_SPLIT = 19, VCNF_TARGET_SMILEY = 20
};
int vcnf_target_log_prob_f32(const float* z, const float* table, float* logp, float* score, int64_t batch,
                             int32_t n_comp, int family, float scale, void* stream);
int vcnf_target_log_prob_f64(const double* z, const double* table, double* logp, double* score, int64_t batch,
                             int32_t n_comp, int family, double scale, void* stream);

/* ---- Stochastic layers of normflow 1.2 (flows/stochastic.py) against the targets above (csrc/stochastic.hip): a run
 * of HamiltonianMonteCarlo layers in one launch with its VJP, and the walk of a MetropolisHastings layer with a diagonal
 * Gaussian proposal.  z / z_out [B, 2] contiguous; family, table, n_comp and scale as for vcnf_target_log_prob_*, with
 * its logp, score and its rule for a non-finite row.  Nothing random is drawn in a kernel: the draws are inputs.
 *   hmc_stack: K = n_layers >= 1 layers of `steps` >= 0 leapfrog steps each, applied in order.  step, mass, sqrt_mass
 *     [K, 2] are exp(log_step_size), exp(log_mass), exp(0.5 log_mass) of the layers (the caller computes them), noise
 *     [K, B, 2] standard-normal and unif [K, B] uniform draws.  Per layer and sample:
 *       p = noise sqrt_mass,  z_new = z,  p_new = p
 *       steps times:  p_half = p_new - (step / 2) (-score(z_new)),  z_new = z_new + step (p_half / mass),
 *                     p_new = p_half - (step / 2) (-score(z_new))
 *       prob = exp(logp(z_new) - logp(z) - sum(p_new^2 / mass) / 2 + sum(p^2 / mass) / 2)
 *       accept = unif < prob (a NaN prob rejects),  z_out = accept ? z_new : z (a rejected row keeps its bits)
 *       log_det += logp(z) - logp(z_out)      (0 on a rejected finite row, NaN on a non-finite one)
 *     K steps + 1 evaluations of (logp, score) per sample.  log_det [B] is stored.  trace [K, B, 2] (may be NULL)
 *     receives the row as it enters each layer and accept [K, B] (bytes 0 / 1, may be NULL) each layer's decision:
 *     what the VJP reads.
 *   hmc_stack_bwd: VJP of the run for the cotangents g_out [B, 2] of z_out and g_logdet [B] of log_det (either may be
 *     NULL = zero), with the score and the decision treated as constants, as the reference's detach does.  Per layer,
 *     last to first, with a the decision, gz the running cotangent and gl = g_logdet:
 *       G = a (gz - gl score(z_new)),  g_z = (1 - a) gz + G + a gl score(z)
 *       g_step      = G sum_i [p_half_i / mass + (step / mass) ((steps - i) s_i + (steps - 1 - i) s_{i+1}) / 2]
 *       g_mass      = -G step sum_i p_half_i / mass^2,      g_sqrt_mass = steps G (step / mass) noise
 *     (s_i the score before step i) from the trajectory recomputed out of trace, accept and noise.  a enters as a
 *     select on g_z and on each of the six terms: a rejected row hands gz on unchanged and adds exact zeros to the sums,
 *     also where its row is non-finite or its trajectory ran off to inf / NaN (the reference's autograd gives NaN
 *     parameter gradients for the whole batch there).  g_in
 *     [B, 2]; g_step, g_mass, g_sqrt_mass [K, 2] summed over the batch: every workgroup adds its samples' terms into
 *     its own block of `workspace` (`groups` blocks of 6 K elements, uninitialised on entry; 1 <= groups <=
 *     min(VCNF_HMC_MAX_BWD_GROUPS, ceil(B / VCNF_HMC_BLOCK)), the number of workgroups) and a second launch adds the
 *     blocks in a fixed order.
 *   hmc_annealed_stack, hmc_annealed_stack_bwd: the same run and its VJP for the layers of Hamiltonian annealed
 *     importance sampling (normflow's sampling/hais.py): layer k's density is the LinearInterpolation of the target and a
 *     2-D diagonal Gaussian prior with the weight beta[k].  beta [K], prior_loc [2] and prior_log_scale [2] are device
 *     memory of the run's type, all required.  At a point x, with (lt, st) the target's logp and score there:
 *       sig_j = exp(ls_j),  u_j = (x_j - loc_j) / sig_j
 *       l0 = -log(2 pi) - (ls_0 + ls_1) - 0.5 (u_0^2 + u_1^2),   s0_j = -u_j / sig_j
 *       logp_k = beta_k lt + (1 - beta_k) l0,   score_k = beta_k st + (1 - beta_k) s0
 *     and the leapfrog, the decision, log_det, trace, accept and the VJP's closed form are hmc_stack's with logp_k and
 *     score_k in place of logp and score (a non-finite row: NaN logp_k and score_k).  Only (lt, st) is carried from layer
 *     to layer and the prior's part recomputed, so the run costs K steps + 1 target evaluations per sample as the plain
 *     one does.  logp_target [B] (may be NULL) receives lt at z_out, the last term of the sampler's log weights.  beta and
 *     the prior's parameters are constants of the VJP; workspace, groups and the reduction are hmc_stack_bwd's.  With
 *     beta = 1 in every layer the run has the bits of hmc_stack on finite rows.
 *   mh_walk: `steps` >= 0 random-walk steps with eps [steps, B, 2] standard-normal and w [steps, B] uniform draws and
 *     prop_scale [2] the proposal's standard deviations (device memory):  z_ = eps prop_scale + z,
 *     accept = w <= min(exp(logp(z_) - logp(z)), 1) (NaN rejects),  z = accept ? z_ : z;  logp(z) is carried from step
 *     to step.  accept [steps, B] (bytes, may be NULL) receives the decisions.  The layer's log_det is zero and it is
 *     the identity under differentiation, so the caller provides both.
 * batch < 0, n_layers < 1, steps < 0, n_comp below what the family reads, or groups outside its range ->
 * VCNF_ERR_SHAPE; unknown family, or n_layers (steps + 1) > VCNF_STOCH_MAX_POINTS (a mistaken argument must not become
 * a launch that runs for minutes) -> VCNF_ERR_UNSUPPORTED; batch == 0 -> VCNF_OK without a launch; NULL required pointer -> VCNF_ERR_NULL; a
 * pointer not aligned to its element size -> VCNF_ERR_ALIGN, checked in this order.
 * One sample per lane; rows move as one 8-byte
 * (16-byte) access when the [., 2] buffers are aligned to it, as two elements otherwise, with the same bits either way.
 * Every loop is bounded by n_layers, steps or n_comp.  No atomics, no allocation, no host synchronisation: every call is
 * bitwise reproducible and capturable. */
/* samples per workgroup, the cap on the workgroups of the HMC VJP, and the limit on n_layers (steps + 1) */
enum { VCNF_HMC_BLOCK = 256, VCNF_HMC_MAX_BWD_GROUPS = 1024, VCNF_STOCH_MAX_POINTS = 65536 };
int vcnf_hmc_stack_f32(const float* z, const float* noise, const float* unif, const float* step, const float* mass,
                       const float* sqrt_mass, const float* table, float* z_out, float* log_det, float* trace,
                       uint8_t* accept, int64_t batch, int32_t n_layers, int32_t steps, int32_t n_comp, int family,
                       float scale, void* stream);
int vcnf_hmc_stack_bwd_f32(const float* trace, const uint8_t* accept, const float* noise, const float* step,
                           const float* mass, const float* sqrt_mass, const float* table, const float* g_out,
                           const float* g_logdet, float* g_in, float* g_step, float* g_mass, float* g_sqrt_mass,
                           float* workspace, int64_t batch, int32_t n_layers, int32_t steps, int32_t groups,
                           int32_t n_comp, int family, float scale, void* stream);
int vcnf_hmc_annealed_stack_f32(const float* z, const float* noise, const float* unif, const float* step, const float* mass,
                                const float* sqrt_mass, const float* beta, const float* prior_loc,
                                const float* prior_log_scale, const float* table, float* z_out, float* log_det,
                                float* logp_target, float* trace, uint8_t* accept, int64_t batch, int32_t n_layers,
                                int32_t steps, int32_t n_comp, int family, float scale, void* stream);
int vcnf_hmc_annealed_stack_bwd_f32(const float* trace, const uint8_t* accept, const float* noise, const float* step,
                                    const float* mass, const float* sqrt_mass, const float* beta, const float* prior_loc,
                                    const float* prior_log_scale, const float* table, const float* g_out,
                                    const float* g_logdet, float* g_in, float* g_step, float* g_mass, float* g_sqrt_mass,
                                    float* workspace, int64_t batch, int32_t n_layers, int32_t steps, int32_t groups,
                                    int32_t n_comp, int family, float scale, void* stream);
int vcnf_mh_walk_f32(const float* z, const float* eps, const float* w, const float* prop_scale, const float* table,
                     float* z_out, uint8_t* accept, int64_t batch, int32_t steps, int32_t n_comp, int family,
                     float scale, void* stream);
int vcnf_hmc_stack_f64(const double* z, const double* noise, const double* unif, const double* step, const double* mass,
                       const double* sqrt_mass, const double* table, double* z_out, double* log_det, double* trace,
                       uint8_t* accept, int64_t batch, int32_t n_layers, int32_t steps, int32_t n_comp, int family,
                       double scale, void* stream);
int vcnf_hmc_stack_bwd_f64(const double* trace, const uint8_t* accept, const double* noise, const double* step,
                           const double* mass, const double* sqrt_mass, const double* table, const double* g_out,
                           const double* g_logdet, double* g_in, double* g_step, double* g_mass, double* g_sqrt_mass,
                           double* workspace, int64_t batch, int32_t n_layers, int32_t steps, int32_t groups,
                           int32_t n_comp, int family, double scale, void* stream);
int vcnf_hmc_annealed_stack_f64(const double* z, const double* noise, const double* unif, const double* step, const double* mass,
                                const double* sqrt_mass, const double* beta, const double* prior_loc,
                                const double* prior_log_scale, const double* table, double* z_out, double* log_det,
                                double* logp_target, double* trace, uint8_t* accept, int64_t batch, int32_t n_layers,
                                int32_t steps, int32_t n_comp, int family, double scale, void* stream);
int vcnf_hmc_annealed_stack_bwd_f64(const double* trace, const uint8_t* accept, const double* noise, const double* step,
                                    const double* mass, const double* sqrt_mass, const double* beta, const double* prior_loc,
                                    const double* prior_log_scale, const double* table, const double* g_out,
                                    const double* g_logdet, double* g_in, double* g_step, double* g_mass, double* g_sqrt_mass,
                                    double* workspace, int64_t batch, int32_t n_layers, int32_t steps, int32_t groups,
                                    int32_t n_comp, int family, double scale, void* stream);
int vcnf_mh_walk_f64(const double* z, const double* eps, const double* w, const double* prop_scale, const double* table,
                     double* z_out, uint8_t* accept, int64_t batch, int32_t steps, int32_t n_comp, int family,
                     double scale, void* stream);

/* ---- The sampling direction of the autoregressive flows in one launch (csrc/made_sample.hip):
 * MaskedAffineAutoregressive.inverse and MaskedPiecewiseRationalQuadraticAutoregressive.inverse
 * (normflow/flows/affine/autoregressive.py:29-36, the loop of D = features MADE passes, over nets/made.py:215-300 with
 * residual blocks and ReLU).  With the reference's sequential degrees a hidden unit of degree m depends on inputs and
 * hidden units of degree <= m only, so once the variable of degree m is known every unit of degree m in every layer is
 * final: the loop is one masked MADE pass ordered by degree with one inversion between stages.
 *   x / y [B, D] contiguous, D = features, H = hidden, nb = num_blocks >= 0, P = params_per_feature.
 *   tables int32 [2 D] on the device: order[i] = the column holding the variable of degree i + 1; count[i] = the number
 *     of hidden units of degree <= i.  Hidden units are stored in ascending degree, in the same order in every layer.
 *     The kernel clamps order to 0 .. D - 1 and count to a non-decreasing sequence in 0 .. H: a wrong table gives wrong
 *     values, never an access out of bounds.
 *   wpack, vcnf_made_sample_pack_elems(D, H, nb, P) elements, the masked weights W * mask one after the other:
 *     Wi [H, D] (columns in the order of `order`), bi [H];  per block  W0 [H, H], b0 [H], W1 [H, H], b1 [H];
 *     Wf [D P, H] (the P rows of the variable of degree i + 1 at rows i P ..), bf [D P].
 *   ctx_add [B, H]: the MADE's context_layer(context);  ctx_gate [nb, B, H]: the blocks' context_layer(context) before
 *     the sigmoid; units in the stored order.  Both NULL without context; with nb = 0 ctx_gate is NULL.
 * Per sample, for i = 0 .. D - 1 (count[-1] = 0):
 *   1. for the units u in [count[i - 1], count[i]), layer by layer:
 *        h_0[u]     = bi[u] + sum_{j < i} Wi[u, j] y[j] + ctx_add[u]
 *        t_k[u]     = b0_k[u] + sum_{v < count[i]} W0_k[u, v] relu(h_k[v])
 *        h_{k+1}[u] = h_k[u] + (b1_k[u] + sum_{v < count[i]} W1_k[u, v] relu(t_k[v])) gate_k[u]
 *        gate_k[u]  = sigmoid(ctx_gate[k, b, u]), or 1
 *   2. q[p] = bf[i P + p] + sum_{v < count[i]} Wf[i P + p, v] h_nb[v],  p < P
 *   3. cfg == NULL (P = 2, the MAF): scale = sigmoid(q[0] + 2) + 1e-3, y[i] = (x[order[i]] - q[1]) / scale,
 *        ld -= log(scale)  (vcnf_maf_affine, inverse);
 *      cfg != NULL (P = 2 K + the derivative logits of cfg->tails): (y[i], lad) = the inverse spline of
 *        vcnf_rqs_elementwise (wh_scale included) at x[order[i]] with the logits q = [K widths | K heights | derivatives],
 *        ld += lad; bad_disc (may be NULL) as there
 *   4. out[b, order[i]] = y[i]
 * and logdet[b] = ld_sign ld, stored or accumulated (ld_mode).  features = 1 has count[0] = H and no input term; a
 * degree that owns no unit has an empty range in step 1.
 * Arithmetic: buffers and the activations kept between stages are float (_f32) or double (_f64); sums, the logits q
 * and step 3 are evaluated in double in both (the _f32 entry point inverts with the spline of vcnf_rqs_elementwise_f64
 * on cfg's values), and each activation, y and the log-det are rounded to the buffer's type once.
 * vcnf_made_sample_supported answers from the kernel's budget: a sample keeps (1 + 2 nb) H + D values and P doubles in
 * LDS and shares vcnf_made_sample_lanes(...) = 8 .. 64 lanes (the smallest group with which a workgroup of 256 threads
 * stays under 48 KiB of LDS, at most the 64 KiB a launch gets without raising the limit; 0: unsupported); D <= 1024,
 * H <= 4096, nb <= 16; splines have K in {8, 10, 16} (any other count would index the knot arrays in scratch).  A
 * workgroup takes 256 / lanes samples per trip.
 * batch < 0, an unsupported shape, wpack_elems or P not matching -> VCNF_ERR_SHAPE; unknown ld_mode or tails, or a
 * bin count without an instance -> VCNF_ERR_UNSUPPORTED; an invalid cfg as for vcnf_rqs_elementwise; batch == 0 ->
 * VCNF_OK without a launch; NULL required pointer, or one of ctx_add / ctx_gate without the other (nb > 0) ->
 * VCNF_ERR_NULL; a pointer not aligned to its element size -> VCNF_ERR_ALIGN.  Dot products are summed in a fixed order
 * (lane g of a group takes the terms g, g + lanes, ..., then the ascending butterfly): every call gives the same bits
 * and a row's bits do not depend on the batch (of this entry point: a caller that chooses between it and another path
 * by batch size, as vcnf_amd/made_sample.py does at 65 536 rows, changes the bits where it changes the path).  No scratch, no atomics besides bad_disc, no allocation, no host
 * synchronisation: capturable. */
int vcnf_made_sample_supported(int32_t features, int32_t hidden, int32_t num_blocks, int32_t params_per_feature,
                               int32_t elem_size);
int32_t vcnf_made_sample_lanes(int32_t features, int32_t hidden, int32_t num_blocks, int32_t params_per_feature,
                               int32_t elem_size);
int64_t vcnf_made_sample_pack_elems(int32_t features, int32_t hidden, int32_t num_blocks, int32_t params_per_feature);
int vcnf_made_sample_f32(const float* x, float* y, float* logdet, const float* ctx_add, const float* ctx_gate,
                         const float* wpack, int64_t wpack_elems, const int32_t* tables, int64_t batch,
                         int32_t features, int32_t hidden, int32_t num_blocks, int32_t params_per_feature,
                         const vcnf_rqs_cfg* cfg, int ld_mode, float ld_sign, int32_t* bad_disc, void* stream);
int vcnf_made_sample_f64(const double* x, double* y, double* logdet, const double* ctx_add, const double* ctx_gate,
                         const double* wpack, int64_t wpack_elems, const int32_t* tables, int64_t batch,
                         int32_t features, int32_t hidden, int32_t num_blocks, int32_t params_per_feature,
                         const vcnf_rqs_cfg_f64* cfg, int ld_mode, double ld_sign, int32_t* bad_disc, void* stream);

/* Diagnostic, not on any product path: ONE dense layer y[B, N] = x[B, K] W[N, K]^T + b (nn.Linear,
 * nets/resnet.py:78-106) evaluated with the arithmetic of one of the fused RQS layer kernels' matrix paths, so that
 * the GEMM-level error of each path can be measured against an fp64 product (tests/test_gpu_gemm_error.py):
 * VCNF_PROBE_F32 - v_mfma_f32_16x16x4_f32 chain as in vcnf_rqs_layer_fused_f32(VCNF_PREC_F32);
 * VCNF_PROBE_F16X3 - split-half operands, hi*hi + (hi*lo + lo*hi) 2^-11 (hidden / last layers of VCNF_PREC_F16X3);
 * VCNF_PROBE_F16X3_LL - the same plus the lo*lo term (its first layer).  relu_input != 0 applies max(x, 0) to the
 * input first (the hidden layers see relu(h), resnet.py:42-46).  K % 16 == 0, N % 32 == 0.  sat_count as in
 * vcnf_rqs_layer_fused_f32 (may be NULL). */
enum { VCNF_PROBE_F32 = 0, VCNF_PROBE_F16X3 = 1, VCNF_PROBE_F16X3_LL = 2 };
int vcnf_linear_probe_f32(const float* x, const float* weight, const float* bias, float* y, int64_t batch,
                          int32_t in_features, int32_t out_features, int mode, int relu_input,
                          int32_t* sat_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VCNF_HIP_H */
