"""Differentiable spline op: forward = vcnf_rqs_elementwise_f32 / _f64, backward =
vcnf_rqs_elementwise_bwd_f32 (csrc/rqs_backward.hip) / _f64 (csrc/rqs_f64.hip).  This is the training path of the
RQS couplings: when gradients are required the coupling layer composes
gather / conditioner / scatter in PyTorch (all differentiable) around this op, exactly the
structure of the reference (flows/neural_spline/coupling.py:70-125), with the spline
arithmetic and its gradient on the HIP kernels."""

import torch
from torch.nn import functional as F

from . import _lib


class RqsSplineFn(torch.autograd.Function):
    """(y, logabsdet) = spline(x; uw, uh, ud), elementwise.  ``wh_scale`` is already folded
    into ``cfg`` (it multiplies the width / height logits inside the kernels)."""

    @staticmethod
    def forward(ctx, x, uw, uh, ud, cfg, inverse):
        with torch.no_grad():
            y, lad = _lib.rqs_elementwise(x, uw, uh, ud, cfg, inverse, allow_grad=True)
        ctx.save_for_backward(x, uw, uh, ud)
        ctx.cfg, ctx.inverse = cfg, inverse
        return y, lad

    @staticmethod
    def backward(ctx, gy, glad):
        x, uw, uh, ud = ctx.saved_tensors
        gx, gw, gh, gd = _lib.rqs_elementwise_bwd(x, uw, uh, ud, gy.contiguous(), glad.contiguous(),
                                                  ctx.cfg, ctx.inverse)
        return gx, gw, gh, gd, None, None


def rqs_spline(x, uw, uh, ud, cfg, inverse=False):
    return RqsSplineFn.apply(x, uw.expand(x.shape + uw.shape[-1:]), uh.expand(x.shape + uh.shape[-1:]),
                             ud.expand(x.shape + ud.shape[-1:]), cfg, inverse)


class RqsLimitsFn(torch.autograd.Function):
    """(y, logabsdet) = spline(x; uw, uh, ud) on per-element intervals [left, right] -> [bottom, top] (tensor limits,
    splines.py:99-102), elementwise: forward vcnf_rqs_elementwise_limits_*, backward vcnf_rqs_elementwise_limits_bwd_*,
    which also returns the gradients of the four limit tensors (None for a limit that does not require grad)."""

    @staticmethod
    def forward(ctx, x, uw, uh, ud, left, right, bottom, top, cfg, inverse):
        with torch.no_grad():
            y, lad = _lib.rqs_elementwise_limits(x, uw, uh, ud, (left, right, bottom, top), cfg, inverse,
                                                 allow_grad=True)
        ctx.save_for_backward(x, uw, uh, ud, left, right, bottom, top)
        ctx.cfg, ctx.inverse = cfg, inverse
        return y, lad

    @staticmethod
    def backward(ctx, gy, glad):
        x, uw, uh, ud, *limits = ctx.saved_tensors
        gx, gw, gh, gd, glim = _lib.rqs_elementwise_limits_bwd(x, uw, uh, ud, limits, gy.contiguous(),
                                                               glad.contiguous(), ctx.cfg, ctx.inverse,
                                                               want=ctx.needs_input_grad[4:8])
        return (gx, gw, gh, gd, *glim, None, None)


def rqs_spline_limits(x, uw, uh, ud, left, right, bottom, top, cfg, inverse=False):
    return RqsLimitsFn.apply(x, uw.expand(x.shape + uw.shape[-1:]), uh.expand(x.shape + uh.shape[-1:]),
                             ud.expand(x.shape + ud.shape[-1:]), left, right, bottom, top, cfg, inverse)


_ARANGE32 = {}


def _arange32(n, device):
    key = (n, str(device))
    hit = _ARANGE32.get(key)
    if hit is None:
        hit = torch.arange(n, dtype=torch.int32, device=device)
        _ARANGE32[key] = hit
    return hit


class RqsPackedFn(torch.autograd.Function):
    """Transform half of a coupling: (y, logabsdet[B]) = spline(x; params) with x [B, C, *inner]
    and the conditioner output params [B, C*P, *inner] used in place, forward and backward: the
    gradient comes back in the conditioner's own output layout (no slicing, no permute, no
    per-tensor copies)."""

    @staticmethod
    def forward(ctx, x, params, cfg, inverse):
        ctx.save_for_backward(x, params)
        ctx.cfg, ctx.inverse = cfg, inverse
        with torch.no_grad():
            if x.dim() == 2 and params.dim() == 2 and cfg.tails == _lib.TAILS_LINEAR and x.dtype == torch.float32:
                # [B, C] inputs: the coupling kernel of the inference path with all C features transformed and no
                # identity half - rows staged through LDS with 16-byte transfers (88 us at 131 072 x 32 against 186 us for
                # the generally-addressed elementwise kernel); it returns the per-sample sum of the log-derivatives.
                # fp32 only: fp64 takes the strided elementwise kernel below (csrc/rqs_f64.hip)
                idx = _arange32(x.shape[1], x.device)
                return _lib.rqs_coupling(x.detach(), params.detach(), idx, idx[:0], None, cfg, inverse)
            y, lad = _lib.rqs_elementwise_image(x, params, cfg, inverse, allow_grad=True)
        return y, lad.reshape(lad.shape[0], -1).sum(1)

    @staticmethod
    def backward(ctx, gy, glad):
        x, params = ctx.saved_tensors
        gx, gp = _lib.rqs_packed_bwd(x, params, gy, glad, ctx.cfg, ctx.inverse)
        return gx, gp, None, None


class RqsSharedFn(torch.autograd.Function):
    """Identity half of a coupling: per-position spline whose logits are shared by the batch.
    Backward reduces the logit gradient over the batch inside the kernel (per-thread knot
    adjoints, one Jacobian application per thread) instead of materialising [B, ..., 3K-1]."""

    @staticmethod
    def forward(ctx, x, uw, uh, ud, cfg, inverse):
        with torch.no_grad():
            y, lad = _lib.rqs_elementwise_shared(x, uw, uh, ud, cfg, inverse, allow_grad=True)
        ctx.save_for_backward(x, uw, uh, ud)
        ctx.cfg, ctx.inverse = cfg, inverse
        return y, lad.reshape(lad.shape[0], -1).sum(1)

    @staticmethod
    def backward(ctx, gy, glad):
        x, uw, uh, ud = ctx.saved_tensors
        gx, gw, gh, gd = _lib.rqs_shared_bwd(x, uw, uh, ud, gy, glad, ctx.cfg, ctx.inverse)
        return gx, gw, gh, gd, None, None


def rqs_shared(x, uw, uh, ud, cfg, inverse=False):
    """(y, logabsdet[B]) of the batch-shared spline, differentiable.  fp64 takes the dense path (there is no fp64
    batch-shared reduction kernel; autograd of the expansion sums the logit gradient over the batch)."""
    if cfg.num_bins in _lib.SHARED_BWD_BINS and x.dtype != torch.float64:
        return RqsSharedFn.apply(x, uw, uh, ud, cfg, inverse)
    y, lad = rqs_spline(x, uw, uh, ud, cfg, inverse)           # any K: dense expansion
    return y, lad.reshape(lad.shape[0], -1).sum(1)


def rqs_packed(x, params, cfg, inverse=False):
    """(y, logabsdet[B]) of the conditional spline on packed conditioner output, differentiable."""
    if cfg.num_bins <= 64:
        return RqsPackedFn.apply(x, params, cfg, inverse)
    raise NotImplementedError("spline VJP kernel covers up to 64 bins")


def needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _bc(g, like):
    """[B] upstream log-det gradient broadcast over the feature dims of ``like``."""
    return g.reshape((-1,) + (1,) * (like.dim() - 1))


def _sum_to_channels(t):
    """Sum over batch and inner dims -> [C] (per-channel parameters)."""
    return t.transpose(0, 1).reshape(t.shape[1], -1).sum(1)


# The remaining layers are one or two elementwise ops; their forward values come from the HIP
# kernels and their VJPs are the closed forms below, evaluated with device tensor ops.

class AffineCouplingFn(torch.autograd.Function):
    """vcnf_affine_coupling_f32.  With m the multiplier (exp(s) | 1/sigmoid(s+2) | sigmoid(s+2))
    and q = d log m / ds:  forward  out = z m + shift, ld = sum log m;  inverse
    out = (z - shift) / m, ld = -sum log m.  Channels outside [t_off, t_off + d_t) pass through."""

    @staticmethod
    def forward(ctx, z, param, t_off, d_t, code, inverse):
        with torch.no_grad():
            out, ld = _lib.affine_coupling(z, param, t_off, d_t, code, inverse)
        ctx.save_for_backward(z if not inverse else out, param)
        ctx.cfg = (t_off, d_t, code, inverse)
        if ld is None:
            ld = torch.zeros(z.shape[0], dtype=z.dtype, device=z.device)
        return out, ld

    @staticmethod
    def backward(ctx, g_out, g_ld):
        keep, param = ctx.saved_tensors
        t_off, d_t, code, inverse = ctx.cfg
        sl = slice(t_off, t_off + d_t)
        g_t = g_out[:, sl]
        g_z = g_out.clone()
        if code == _lib.SCALE_NONE:
            g_param = -g_t if inverse else g_t
            return g_z, g_param.contiguous(), None, None, None, None
        s = param[:, 1::2]
        if code == _lib.SCALE_EXP:
            m, q = torch.exp(s), None
        else:
            sig = torch.sigmoid(s + 2)
            m, q = (1 / sig, sig - 1) if code == _lib.SCALE_SIGMOID else (sig, 1 - sig)
        gl = _bc(g_ld, g_t)
        if not inverse:
            g_z[:, sl] = g_t * m
            g_shift = g_t
            g_s = g_t * keep[:, sl] * m + gl            # keep = z
        else:
            g_z[:, sl] = g_t / m
            g_shift = -g_z[:, sl]
            g_s = -(g_t * keep[:, sl]) - gl             # keep = out
        if q is not None:
            g_s = g_s * q
        g_param = torch.empty_like(param)
        g_param[:, 0::2] = g_shift
        g_param[:, 1::2] = g_s
        return g_z, g_param, None, None, None, None


class MaskedAffineFn(torch.autograd.Function):
    """vcnf_masked_affine_f32: out = b z + (1-b)(z e^s + t) | b z + (1-b)(z - t) e^-s, [B, D]."""

    @staticmethod
    def forward(ctx, z, s, t, bmask, inverse):
        with torch.no_grad():
            out, ld = _lib.masked_affine(z, s, t, bmask, inverse)
        ctx.save_for_backward(z, s, t, bmask, out)
        ctx.inverse = inverse
        return out, ld

    @staticmethod
    def backward(ctx, g_out, g_ld):
        z, s, t, b, out = ctx.saved_tensors
        nb = 1 - b
        gl = g_ld[:, None]
        e = torch.exp(s if not ctx.inverse else -s) if s is not None else None
        if not ctx.inverse:
            g_z = g_out * (b + nb * e) if s is not None else g_out
            g_s = nb * (g_out * z * e + gl) if s is not None else None
            g_t = nb * g_out if t is not None else None
        else:
            g_z = g_out * (b + nb * e) if s is not None else g_out
            # (1-b) out = (1-b)(z - t) e^-s
            g_s = nb * (-(g_out * out) - gl) if s is not None else None
            g_t = (-(nb * g_out * e) if s is not None else -(nb * g_out)) if t is not None else None
        return g_z, g_s, g_t, None, None


class AffineConstFn(torch.autograd.Function):
    """vcnf_affine_const_f32: out = z e^s + t | (z - t) e^-s with per-channel s, t [C]."""

    @staticmethod
    def forward(ctx, z, s, t, inverse):
        with torch.no_grad():
            out = _lib.affine_const(z, s, t, inverse)
        ctx.save_for_backward(z if not inverse else out, s)
        ctx.inverse = inverse
        return out

    @staticmethod
    def backward(ctx, g):
        keep, s = ctx.saved_tensors
        shape = (1, -1) + (1,) * (g.dim() - 2)
        if not ctx.inverse:
            e = torch.exp(s).reshape(shape)
            return g * e, _sum_to_channels(g * keep * e), _sum_to_channels(g), None
        e = torch.exp(-s).reshape(shape)
        g_z = g * e
        return g_z, -_sum_to_channels(g * keep), -_sum_to_channels(g_z), None


class PermuteFn(torch.autograd.Function):
    """vcnf_permute_f32; the VJP is the same kernel with the opposite index vector."""

    @staticmethod
    def forward(ctx, z, idx32, back32):
        ctx.back = back32
        with torch.no_grad():
            return _lib.permute(z, idx32)

    @staticmethod
    def backward(ctx, g):
        return _lib.permute(g.contiguous(), ctx.back), None, None


class SplitColumnsFn(torch.autograd.Function):
    """(z[:, gather[:first]], z[:, gather[first:]]) as two contiguous tensors in one pass (vcnf_split_columns); the VJP
    is MergeColumnsFn's forward.  Replaces a full column permutation, two slice copies and, in the backward pass, two
    zero fills, two slice writes and an add."""

    @staticmethod
    def forward(ctx, z, gather32, scatter32, first):
        ctx.scatter = scatter32
        with torch.no_grad():
            return _lib.split_columns(z, gather32, first)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ga, gb):
        return _lib.merge_columns(ga, gb, ctx.scatter), None, None, None


class MergeColumnsFn(torch.autograd.Function):
    """cat([a, b], 1)[:, scatter] in one pass (vcnf_merge_columns); the VJP is SplitColumnsFn's forward."""

    @staticmethod
    def forward(ctx, a, b, gather32, scatter32):
        ctx.gather, ctx.first = gather32, a.shape[1]
        with torch.no_grad():
            return _lib.merge_columns(a, b, scatter32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ga, gb = _lib.split_columns(g, ctx.gather, ctx.first)
        return ga, gb, None, None


class DiagGaussianLogProbFn(torch.autograd.Function):
    """vcnf_diag_gaussian_log_prob_f32: lp = const - sum(ls + ((z - loc) / e^ls)^2 / 2)."""

    @staticmethod
    def forward(ctx, z, loc, ls, temperature):
        with torch.no_grad():
            lp = _lib.diag_gaussian_log_prob(z, loc, ls, temperature)
        ctx.save_for_backward(z, loc, ls)
        ctx.lt = _lib._log_t(temperature)
        return lp

    @staticmethod
    def backward(ctx, g):
        z, loc, ls = ctx.saved_tensors
        v = z.reshape(len(z), -1)
        inv = torch.exp(-(ls + ctx.lt))
        u = (v - loc) * inv
        gu = g[:, None] * u
        return (-(gu * inv)).reshape(z.shape), (gu * inv).sum(0), (gu * u - g[:, None]).sum(0), None


class DiagGaussianSampleFn(torch.autograd.Function):
    """vcnf_diag_gaussian_sample_f32: z = loc + e^ls eps, lp = const - sum(ls + eps^2 / 2)."""

    @staticmethod
    def forward(ctx, eps, loc, ls, temperature):
        with torch.no_grad():
            z, lp = _lib.diag_gaussian_sample(eps, loc, ls, temperature)
        ctx.save_for_backward(eps, ls)
        ctx.lt = _lib._log_t(temperature)
        return z, lp

    @staticmethod
    def backward(ctx, g_z, g_lp):
        eps, ls = ctx.saved_tensors
        e = eps.reshape(len(eps), -1)
        gz = g_z.reshape(len(eps), -1)
        sig = torch.exp(ls + ctx.lt)
        g_eps = gz * sig - g_lp[:, None] * e
        return g_eps.reshape(eps.shape), gz.sum(0), (gz * sig * e - g_lp[:, None]).sum(0), None

def _onto_rows(per_sample, row_index, rows):
    """Per-sample gradients [B, C] summed onto the [rows, C] parameter table they were read from: the fixed-order
    segmented sum kernel under a row index, a column sum for one shared row, nothing for one row per sample."""
    if row_index is not None:
        return _lib.cc_gaussian_reduce_rows(per_sample, row_index, rows)
    return per_sample.sum(0, keepdim=True) if rows == 1 and per_sample.shape[0] != 1 else per_sample


class ClassCondGaussianLogProbFn(torch.autograd.Function):
    """vcnf_cc_gaussian_log_prob_*: log density of z [B, C, P...] under the Gaussians of the table rows
    loc_rows / ls_rows [R, C] picked by row_index (int32 [B], or None with R in {1, B}); backward on
    vcnf_cc_gaussian_log_prob_bwd_* and vcnf_cc_gaussian_reduce_rows_*."""

    @staticmethod
    def forward(ctx, z, loc_rows, ls_rows, row_index, pixels, temperature):
        with torch.no_grad():
            lp = _lib.cc_gaussian_log_prob(z, loc_rows, ls_rows, row_index, pixels, temperature)
        ctx.save_for_backward(z, loc_rows, ls_rows, row_index)
        ctx.pixels, ctx.temperature = pixels, temperature
        return lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, loc_rows, ls_rows, row_index = ctx.saved_tensors
        dz, d_loc, d_ls = _lib.cc_gaussian_log_prob_bwd(z, loc_rows, ls_rows, row_index, ctx.pixels, ctx.temperature, g)
        rows = ls_rows.shape[0]
        return (dz, _onto_rows(d_loc, row_index, rows) if ctx.needs_input_grad[1] else None,
                _onto_rows(d_ls, row_index, rows) if ctx.needs_input_grad[2] else None, None, None, None)


class ClassCondGaussianSampleFn(torch.autograd.Function):
    """vcnf_cc_gaussian_sample_*: (z, log p(z)) = (loc + e^ls eps, ...) for the draw eps [B, C, P...]; backward on
    vcnf_cc_gaussian_sample_bwd_* and vcnf_cc_gaussian_reduce_rows_*."""

    @staticmethod
    def forward(ctx, eps, loc_rows, ls_rows, row_index, pixels, temperature):
        with torch.no_grad():
            z, lp = _lib.cc_gaussian_sample(eps, loc_rows, ls_rows, row_index, pixels, temperature)
        ctx.save_for_backward(eps, ls_rows, row_index)
        ctx.pixels, ctx.temperature = pixels, temperature
        return z, lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_z, g_lp):
        eps, ls_rows, row_index = ctx.saved_tensors
        d_eps, d_loc, d_ls = _lib.cc_gaussian_sample_bwd(eps, ls_rows, row_index, ctx.pixels, ctx.temperature, g_z, g_lp)
        rows = ls_rows.shape[0]
        return (d_eps, _onto_rows(d_loc, row_index, rows) if ctx.needs_input_grad[1] else None,
                _onto_rows(d_ls, row_index, rows) if ctx.needs_input_grad[2] else None, None, None, None)


class GaussianMixtureLogProbFn(torch.autograd.Function):
    """vcnf_gmm_log_prob_*: mixture log density of z [B, D] under the modes loc / ls [M, D] with log weights log_w [M];
    backward on vcnf_gmm_log_prob_bwd_* (the saved result is its lse) and vcnf_gmm_reduce_partials_*."""

    @staticmethod
    def forward(ctx, z, loc, ls, log_w):
        with torch.no_grad():
            lp = _lib.gmm_log_prob(z, loc, ls, log_w)
        ctx.save_for_backward(z, loc, ls, log_w, lp)
        return lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, loc, ls, log_w, lp = ctx.saved_tensors
        need = ctx.needs_input_grad
        dz, d_loc, d_ls, d_w = _lib.gmm_log_prob_bwd(z, loc, ls, log_w, lp, g, tables=any(need[1:4]))
        return dz, d_loc if need[1] else None, d_ls if need[2] else None, d_w if need[3] else None


class GaussianMixtureSampleFn(torch.autograd.Function):
    """vcnf_gmm_sample_*: (z, log p(z)) with z = loc[mode] + e^ls[mode] eps for the drawn modes (int32 [B], no
    gradient).  Backward: the density's VJP kernel gives dz_total = g_z + g_lp dlogp/dz and the parameters' share through
    the density; the reparametrisation's share is d_eps = dz_total e^ls[mode] and the rows dz_total / dz_total eps
    e^ls[mode] summed onto their mode's table row by vcnf_cc_gaussian_reduce_rows_* (fixed order)."""

    @staticmethod
    def forward(ctx, eps, loc, ls, log_w, mode):
        with torch.no_grad():
            z, lp = _lib.gmm_sample(eps, mode, loc, ls, log_w)
        ctx.save_for_backward(eps, loc, ls, log_w, mode, z, lp)
        return z, lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_z, g_lp):
        eps, loc, ls, log_w, mode, z, lp = ctx.saved_tensors
        need = ctx.needs_input_grad
        dz, d_loc, d_ls, d_w = _lib.gmm_log_prob_bwd(z, loc, ls, log_w, lp, g_lp, gz_in=g_z, tables=any(need[1:4]))
        m = ls.shape[0]
        # a mode outside the table never indexes a tensor: its z row is NaN already
        scale = torch.exp(ls).index_select(0, mode.clamp(0, m - 1).long())
        if need[1]:
            d_loc = d_loc + _lib.cc_gaussian_reduce_rows(dz, mode, m)
        if need[2]:
            d_ls = d_ls + _lib.cc_gaussian_reduce_rows(dz * eps * scale, mode, m)
        return dz * scale, d_loc if need[1] else None, d_ls if need[2] else None, d_w if need[3] else None, None


class HeavyTailLogProbFn(torch.autograd.Function):
    """vcnf_tail_log_prob_*: log density of z [B, ...] under the product of Student-t / generalised Gaussian factors with
    the rows loc, ls, shape (nu or beta) and cst (the normalisers) [D]; backward on vcnf_tail_log_prob_bwd_* and
    vcnf_tail_reduce_partials_*.  d_shape is the density's own share; cst gets sum_b g per feature and the caller's
    autograd carries it on to the tail parameter."""

    @staticmethod
    def forward(ctx, z, loc, ls, shape, cst, family):
        with torch.no_grad():
            lp = _lib.tail_log_prob(z, loc, ls, shape, cst, family)
        ctx.save_for_backward(z, loc, ls, shape)
        ctx.family = family
        return lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, loc, ls, shape = ctx.saved_tensors
        need = ctx.needs_input_grad
        dz, d_loc, d_ls, d_sh = _lib.tail_log_prob_bwd(z, loc, ls, shape, ctx.family, g, rows=any(need[1:4]))
        return (dz, d_loc if need[1] else None, d_ls if need[2] else None, d_sh if need[3] else None,
                g.sum().expand(shape.shape) if need[4] else None, None)


class HeavyTailSampleFn(torch.autograd.Function):
    """vcnf_tail_sample_*: (z, log p(z)) from the standard-normal draw eps and the gamma draw; backward on
    vcnf_tail_sample_bwd_* and vcnf_tail_reduce_partials_*, with respect to both draws and the four rows (the gradient
    of gamma is what carries the tail parameter's pathwise share through torch's gamma sampler)."""

    @staticmethod
    def forward(ctx, eps, gamma, loc, ls, shape, cst, family):
        with torch.no_grad():
            z, lp = _lib.tail_sample(eps, gamma, loc, ls, shape, cst, family)
        ctx.save_for_backward(eps, gamma, loc, ls, shape)
        ctx.family = family
        return z, lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_z, g_lp):
        eps, gamma, loc, ls, shape = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_eps, d_gamma, d_loc, d_ls, d_sh = _lib.tail_sample_bwd(eps, gamma, loc, ls, shape, ctx.family, g_z, g_lp,
                                                                 rows=any(need[2:5]), want_eps=need[0])
        return (d_eps, d_gamma if need[1] else None, d_loc if need[2] else None, d_ls if need[3] else None,
                d_sh if need[4] else None, g_lp.sum().expand(shape.shape) if need[5] else None, None)


class VaeEncodeFn(torch.autograd.Function):
    """vcnf_vae_encode_*: (z like eps, log q [B, S]) of the draw eps [B, S, ...] under the Gaussian of the parameter rows
    h [B, ...] = [mean | log variance] as ONE node that saves only its inputs; backward is vcnf_vae_encode_bwd_*.  eps
    gets no gradient (a caller whose eps requires grad takes the torch composition).  Not double-differentiable."""

    @staticmethod
    def forward(ctx, h, eps):
        with torch.no_grad():
            z, lq = _lib.vae_encode(h, eps)
        ctx.save_for_backward(h, eps)
        ctx.set_materialize_grads(False)
        return z, lq

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_z, g_lq):
        h, eps = ctx.saved_tensors
        if g_z is None and g_lq is None:
            return None, None
        return _lib.vae_encode_bwd(h, eps, g_z, g_lq), None


class VaeGaussLogProbFn(torch.autograd.Function):
    """vcnf_vae_gauss_log_prob_*: log density [N] of v [N / v_div, ...] under the Gaussians of the parameter rows
    h [N / h_div, ...] as ONE node that saves only its inputs; backward is vcnf_vae_gauss_log_prob_bwd_*, for whichever
    of v and h needs a gradient.  Not double-differentiable."""

    @staticmethod
    def forward(ctx, v, h, v_div, h_div):
        with torch.no_grad():
            lp = _lib.vae_gauss_log_prob(v, h, v_div, h_div)
        ctx.save_for_backward(v, h)
        ctx.divs = (v_div, h_div)
        return lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        v, h = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_v, d_h = _lib.vae_gauss_log_prob_bwd(v, h, g, *ctx.divs, want_v=need[0], want_h=need[1])
        return d_v, d_h, None, None


class VaeBernoulliLogProbFn(torch.autograd.Function):
    """vcnf_vae_bernoulli_log_prob_*: log likelihood [N] of the data x [N / x_div, ...] under the scores [N, ...] as ONE
    node that saves only its inputs; backward is vcnf_vae_bernoulli_log_prob_bwd_*.  x gets no gradient (a caller whose
    x requires grad takes the torch composition).  Not double-differentiable."""

    @staticmethod
    def forward(ctx, x, score, x_div):
        with torch.no_grad():
            lp = _lib.vae_bernoulli_log_prob(x, score, x_div)
        ctx.save_for_backward(x, score)
        ctx.x_div = x_div
        return lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, score = ctx.saved_tensors
        return None, _lib.vae_bernoulli_log_prob_bwd(x, score, g, ctx.x_div), None


class PeriodicFn(torch.autograd.Function):
    """vcnf_periodic_*: a PeriodicWrap / PeriodicShift direction as ONE node.  The map is a translation by a multiple of
    the period on every column, so its derivative is 1: backward hands the incoming gradient on, without a launch."""

    @staticmethod
    def forward(ctx, z, half, shift, sign):
        with torch.no_grad():
            return _lib.periodic(z, half, shift, sign)

    @staticmethod
    def backward(ctx, g):
        return g, None, None, None


class UniformGaussianLogProbFn(torch.autograd.Function):
    """vcnf_uniform_gaussian_log_prob_*: log density [B] of z [B, D] under UniformGaussian as ONE node that saves only
    its inputs; backward is vcnf_uniform_gaussian_log_prob_bwd_*, one launch.  The scale is a buffer and gets no
    gradient.  Not double-differentiable."""

    @staticmethod
    def forward(ctx, z, inv_scale_g, const_term):
        with torch.no_grad():
            lp = _lib.uniform_gaussian_log_prob(z, inv_scale_g, const_term)
        ctx.save_for_backward(z, inv_scale_g)
        return lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, inv_scale_g = ctx.saved_tensors
        return _lib.uniform_gaussian_log_prob_bwd(z, inv_scale_g, g), None, None


class LogitFn(torch.autograd.Function):
    """vcnf_logit_inverse_* / vcnf_logit_forward_*: (out, log-det [B]) of a Logit direction as ONE node that saves only
    its input; backward is vcnf_logit_*_bwd_*, one launch that recomputes from it.  Not double-differentiable."""

    @staticmethod
    def forward(ctx, x, alpha, inverse):
        with torch.no_grad():
            out, ld = _lib.logit(x, alpha, inverse)
        ctx.save_for_backward(x)
        ctx.args = (alpha, inverse)
        ctx.set_materialize_grads(False)
        return out, ld

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_ld):
        x, = ctx.saved_tensors
        if g_out is None and g_ld is None:
            return None, None, None
        return _lib.logit_bwd(x, *ctx.args, g_out=g_out, g_ld=g_ld), None, None


class DequantMergeFn(torch.autograd.Function):
    """vcnf_dequant_merge_*: (out, log-det [B]) of the noise w [B, C] merged into the categorical columns of the rows x as
    ONE node that saves x and w; backward is vcnf_dequant_merge_bwd_*, one launch that recomputes from them.  The rows
    get a gradient only where they ask for one (continuous columns hand the cotangent through, categorical ones are
    constants).  Not double-differentiable."""

    @staticmethod
    def forward(ctx, x, w, slot, levels, noise_is_logit, alpha):
        with torch.no_grad():
            out, ld = _lib.dequant_merge(x, slot, levels, w, noise_is_logit, alpha)
        ctx.save_for_backward(x, w, slot, levels)
        ctx.args = (noise_is_logit, alpha)
        ctx.set_materialize_grads(False)
        return out, ld

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_ld):
        x, w, slot, levels = ctx.saved_tensors
        if g_out is None and g_ld is None:
            return None, None, None, None, None, None
        d_w, d_x = _lib.dequant_merge_bwd(x, slot, levels, w, *ctx.args, g_out=g_out, g_ld=g_ld,
                                          want_x=ctx.needs_input_grad[0])
        return d_x, (d_w if ctx.needs_input_grad[1] else None), None, None, None, None


class PlanarRadialStackFn(torch.autograd.Function):
    """vcnf_planar_radial_stack_*: (out, log|det| [B]) of a run of Planar / Radial layers from its effective operands va,
    vb [K, D] and sc [K, 2] (vcnf_amd.fused_planar.operands) as ONE node.  Forward launches the kernel with the trace
    [K, B] and the row checkpoints; backward is vcnf_planar_radial_stack_bwd_*, which rebuilds the layers' inputs from
    the run's output, the trace and the checkpoints: the saved state is O(B K + B D)."""

    @staticmethod
    def forward(ctx, z, va, vb, sc, kinds):
        with torch.no_grad():
            out, ld, trace, ckpt = _lib.planar_radial_stack(z, kinds, va, vb, sc, want_trace=True)
        ctx.save_for_backward(out, trace, ckpt, va, vb, sc)
        ctx.kinds = kinds
        ctx.set_materialize_grads(False)
        return out, ld

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_ld):
        out, trace, ckpt, va, vb, sc = ctx.saved_tensors
        g_in, g_va, g_vb, g_sc = _lib.planar_radial_stack_bwd(out, trace, ckpt, ctx.kinds, va.detach(), vb.detach(),
                                                               sc.detach(), g_out, g_ld)
        return g_in, g_va, g_vb, g_sc, None


class TargetLogProbFn(torch.autograd.Function):
    """vcnf_target_log_prob_*: log density of z [B, 2] under one of the 2-D targets as ONE node.  The forward launch also
    writes the score d logp / d z, the only thing saved; backward is one multiply.  The targets have no parameters."""

    @staticmethod
    def forward(ctx, z, table, family, scale):
        lp, score = _lib.target_log_prob(z, family, table, scale, want_score=True)
        ctx.save_for_backward(score)
        return lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        score, = ctx.saved_tensors
        return g[:, None] * score, None, None, None


class HmcStackFn(torch.autograd.Function):
    """vcnf_hmc_stack_*: (z_out, log_det [B]) of a run of HamiltonianMonteCarlo layers from its operands step, mass,
    sqrt_mass [K, 2] (vcnf_amd.fused_stochastic.operands) and the draws noise [K, B, 2], unif [K, B] as ONE node.  Forward
    launches the kernel with the trace (each layer's entrance row) and the decisions; backward is
    vcnf_hmc_stack_bwd_*, which recomputes each layer's trajectory: the saved state is O(B K).  The score and the
    decisions are constants under differentiation, as the reference's detach makes them; the draws get no gradient."""

    @staticmethod
    def forward(ctx, z, step, mass, sqrt_mass, noise, unif, steps, family, table, scale):
        with torch.no_grad():
            out, ld, trace, accept = _lib.hmc_stack(z, noise, unif, step, mass, sqrt_mass, steps, family, table, scale,
                                                    want_trace=True)
        ctx.save_for_backward(trace, accept, noise, step, mass, sqrt_mass, table)
        ctx.target = (steps, family, scale)
        ctx.set_materialize_grads(False)
        return out, ld

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_ld):
        trace, accept, noise, step, mass, sqrt_mass, table = ctx.saved_tensors
        steps, family, scale = ctx.target
        g_in, g_step, g_mass, g_sqm = _lib.hmc_stack_bwd(trace, accept, noise, step.detach(), mass.detach(),
                                                         sqrt_mass.detach(), steps, family, table, scale, g_out, g_ld)
        return g_in, g_step, g_mass, g_sqm, None, None, None, None, None, None


class HmcAnnealedStackFn(torch.autograd.Function):
    """vcnf_hmc_annealed_stack_*: HmcStackFn for a run of annealed layers, whose densities are the LinearInterpolation
    of the target and a 2-D diagonal Gaussian prior (prior_loc, prior_log_scale [2]) with the weights beta [K].  beta and
    the prior's parameters are constants of the run: they get no gradient, and the caller sends a prior that trains to
    the torch composition.  Backward is vcnf_hmc_annealed_stack_bwd_*."""

    @staticmethod
    def forward(ctx, z, step, mass, sqrt_mass, noise, unif, beta, prior_loc, prior_log_scale, steps, family, table, scale):
        with torch.no_grad():
            out, ld, trace, accept = _lib.hmc_annealed_stack(z, noise, unif, step, mass, sqrt_mass, beta, prior_loc,
                                                             prior_log_scale, steps, family, table, scale, want_trace=True)
        ctx.save_for_backward(trace, accept, noise, step, mass, sqrt_mass, beta, prior_loc, prior_log_scale, table)
        ctx.target = (steps, family, scale)
        ctx.set_materialize_grads(False)
        return out, ld

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_ld):
        trace, accept, noise, step, mass, sqrt_mass, beta, prior_loc, prior_log_scale, table = ctx.saved_tensors
        steps, family, scale = ctx.target
        g_in, g_step, g_mass, g_sqm = _lib.hmc_annealed_stack_bwd(trace, accept, noise, step.detach(), mass.detach(),
                                                                  sqrt_mass.detach(), beta, prior_loc, prior_log_scale,
                                                                  steps, family, table, scale, g_out, g_ld)
        return (g_in, g_step, g_mass, g_sqm) + (None,) * 9


class MhWalkFn(torch.autograd.Function):
    """vcnf_mh_walk_*: the Metropolis-Hastings walk of z [B, 2] as a node.  Every step is z or z + eps scale, chosen by a
    decision that has no derivative: the walk is the identity under differentiation and backward hands gz through."""

    @staticmethod
    def forward(ctx, z, eps, w, prop_scale, family, table, scale):
        return _lib.mh_walk(z, eps, w, prop_scale, family, table, scale)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return g, None, None, None, None, None, None


def _mvn_d_consts(g, d_nu):
    """Gradient of consts = (cst, nu): cst enters every sample's log density once."""
    return torch.cat([g.sum().reshape(1), d_nu])


class MultivariateLogProbFn(torch.autograd.Function):
    """vcnf_mvn_log_prob_*: log density of z [B, D] under the multivariate Gaussian / Student-t with location loc [D],
    scale factor tri = L [D, D], its inverse tri_inv (a constant here: the gradient goes to L) and consts = (cst, nu);
    backward on vcnf_mvn_log_prob_bwd_* and vcnf_mvn_reduce_partials_*.  The kernels sum Y = tril(sum_b c_b y_b y_b^T);
    the gradient of L is -tril(L^-T Y_sym), a [D, D] product in fp64 like the inverse itself.  The caller's autograd
    carries it on to lower and log_diag, and d_consts to log_diag and log_df."""

    @staticmethod
    def forward(ctx, z, loc, tri, tri_inv, consts, family):
        with torch.no_grad():
            lp = _lib.mvn_log_prob(z, loc, tri_inv, consts, family)
        ctx.save_for_backward(z, loc, tri_inv, consts)
        ctx.family = family
        return lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, loc, tri_inv, consts = ctx.saved_tensors
        need = ctx.needs_input_grad
        dz, d_loc, yy, d_nu = _lib.mvn_log_prob_bwd(z, loc, tri_inv, consts, ctx.family, g, sums=any(need[1:5]))
        d_tri = None
        if need[2]:
            yy = yy.double()
            d_tri = -torch.tril(tri_inv.double().t() @ (yy + yy.tril(-1).t())).to(z.dtype)
        return (dz, d_loc if need[1] else None, d_tri, None, _mvn_d_consts(g, d_nu) if need[4] else None, None)


class MultivariateSampleFn(torch.autograd.Function):
    """vcnf_mvn_sample_*: (z, log p(z)) from the standard-normal draw eps [B, D] and, for the Student-t, the gamma draw
    [B]; backward on vcnf_mvn_sample_bwd_* and vcnf_mvn_reduce_partials_*, with respect to both draws, loc, the scale
    factor tri and consts (the gradient of gamma is what carries the pathwise share of log_df through torch's gamma
    sampler)."""

    @staticmethod
    def forward(ctx, eps, gamma, loc, tri, consts, family):
        with torch.no_grad():
            z, lp = _lib.mvn_sample(eps, gamma, loc, tri, consts, family)
        ctx.save_for_backward(eps, gamma, tri, consts)
        ctx.family = family
        return z, lp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_z, g_lp):
        eps, gamma, tri, consts = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_eps, d_gamma, d_loc, d_tri, d_nu = _lib.mvn_sample_bwd(eps, gamma, tri, consts, ctx.family, g_z, g_lp,
                                                                 sums=any(need[2:5]), want_eps=need[0])
        return (d_eps, d_gamma if need[1] else None, d_loc if need[2] else None, d_tri if need[3] else None,
                _mvn_d_consts(g_lp, d_nu) if need[4] else None, None)

# Matrix path of the conditioner's dense layers on the training path at large batches: 'fp16x3' - forward products, the
# 128 -> 128 layers' input gradients (csrc/linear_f16x3.hip) and the weight gradients (csrc/linear_wgrad.hip, split-half
# form) on fp16 split-half operands with fp32 accumulation - or 'fp32': the library's fp32 GEMMs and the exact-fp32
# weight-gradient kernel.  What holds on 'fp16x3' (tests/test_gpu_gemm_error.py, tests/test_gpu_grad_range.py): every
# entry within 4 * 2^-24 * sum |a b| of the fp64 product and mean / p99.9 error not above the library's fp32 GEMM, for
# activations and weights of unit scale and for cotangents of ANY scale - a cotangent (1/B under a mean loss: 2^-17 at
# the benchmark's batch, below fp16's smallest normal) travels times a power of two taken from its largest
# |value| (_cot_amax; split_half.hpp::pre_scale) - per row of the cotangent in an input gradient, per column in a weight
# gradient -, exact on the way in and out, so it is never clamped and keeps full precision for 2^29 below the largest
# entry of its row / column.  Activations and weights are NOT scaled: beyond +-65504 they are clamped
# and counted (nf.check_saturation()), and below 2^-14 they lose bits as a bare fp16 split does.
TRAIN_MATRIX_PATH = 'fp16x3'


def _cot_amax(g, n_in, wgrad=True, dgrad=True):
    """Largest |g| per row and per column for the split-half kernels that take the cotangent ``g`` [B, n_out] of a layer
    with ``n_in`` inputs (one reduction shared by its weight-gradient and input-gradient launches), or None when neither
    launch will run: off the 'fp16x3' path, below WGRAD_MIN_BATCH, or a shape that goes to the library in both
    (``wgrad`` / ``dgrad``: whether the caller wants that product at all)."""
    if not (TRAIN_MATRIX_PATH == 'fp16x3' and g.is_cuda and g.dtype == torch.float32 and g.dim() == 2
            and g.is_contiguous() and g.shape[0] >= WGRAD_MIN_BATCH):
        return None
    n_out = g.shape[1]
    takes_w = wgrad and bool(_lib.lib().vcnf_linear_wgrad_supported(n_in, n_out))
    takes_d = dgrad and n_in == n_out and bool(_lib.lib().vcnf_linear_f16x3_supported(n_out, n_in))
    if not (takes_w or takes_d) or not _lib.lib().vcnf_abs_max_rows_cols_scratch_floats(g.shape[0], n_out):
        return None
    return _lib.abs_max(g)


def _f16x3_ok(x, n_in, n_out):
    return (TRAIN_MATRIX_PATH == 'fp16x3' and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
            and x.shape[0] >= WGRAD_MIN_BATCH and bool(_lib.lib().vcnf_linear_f16x3_supported(n_in, n_out)))


def _fwd(x, weight, bias):
    """x W^T + b: split-half kernel where it wins (every forward shape of the conditioner), library otherwise."""
    if _f16x3_ok(x, weight.shape[1], weight.shape[0]):
        return _lib.linear_f16x3(x, weight, bias)
    return torch.addmm(bias, x, weight.t()) if bias is not None else x @ weight.t()


def _dgrad(gy, weight, amax=None):
    """gy W: split-half kernel for the square hidden layers (40 against 52 us at 131 072 x 128 x 128), library for the
    narrow / very deep ones, where its tiling is as fast."""
    if weight.shape[0] == weight.shape[1] and _f16x3_ok(gy, weight.shape[0], weight.shape[1]):
        return _lib.linear_f16x3(gy, weight, None, input_grad=True, amax=amax)
    return gy @ weight


class LinearFn(torch.autograd.Function):
    """y = x W^T + b whose weight / bias gradients come from csrc/linear_wgrad.hip (batch reduction split over the
    chip) instead of the library's output-tiled GEMM + column-sum kernel; forward and input gradient stay library GEMMs.
    Used by the conditioner's dense layers at training batch sizes (nets/resnet.py)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return _fwd(x, weight, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx = gw = gb = None
        gy = gy.contiguous()
        want_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        amax = _cot_amax(gy, weight.shape[1], wgrad=want_w, dgrad=ctx.needs_input_grad[0])
        if ctx.needs_input_grad[0]:
            gx = _dgrad(gy, weight, amax)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw, gb = _lib.linear_wgrad(x, gy, want_bias=ctx.has_bias and ctx.needs_input_grad[2],
                                       f16x3=TRAIN_MATRIX_PATH == 'fp16x3', amax=amax)
            if not ctx.needs_input_grad[1]:
                gw = None
        return gx, gw, gb


WGRAD_MIN_BATCH = 32768          # below this the library's output-tiled GEMM is as fast (16 384: 18.1 vs 19.4 ms per C3 step)


def linear(mod, x):
    """``mod(x)`` for an nn.Linear: through LinearFn when a weight gradient will be needed, the batch is large and the
    layer shape is one the weight-gradient kernel covers; the plain module call otherwise."""
    if (torch.is_grad_enabled() and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and mod.weight.requires_grad
            and x.shape[0] >= WGRAD_MIN_BATCH and type(mod) is torch.nn.Linear
            and _lib.lib().vcnf_linear_wgrad_supported(mod.in_features, mod.out_features)):
        return LinearFn.apply(x, mod.weight, mod.bias)
    return mod(x)

def _wgrad_or_torch(x, gy, want_bias=True, amax=None):
    if x.shape[0] >= WGRAD_MIN_BATCH and _lib.lib().vcnf_linear_wgrad_supported(x.shape[1], gy.shape[1]):
        return _lib.linear_wgrad(x, gy, want_bias=want_bias, f16x3=TRAIN_MATRIX_PATH == 'fp16x3', amax=amax)
    return gy.t() @ x, (gy.sum(0) if want_bias else None)


class ResBlockFn(torch.autograd.Function):
    """One residual block of the conditioner, out = h + W1 relu(W0 relu(h) + b0) + b1 (times sigmoid(gate) when the
    block is context-gated; nets/resnet.py:38-57), as ONE autograd node: the GEMMs stay library calls (weight gradients
    through csrc/linear_wgrad.hip), every elementwise piece of the forward and of the backward is a fused map of
    csrc/resblock_ops.hip, and only relu(h), relu(a), the second Linear's output and the gate logits are kept."""

    @staticmethod
    def forward(ctx, h, gate, w0, b0, w1, b1):
        fused_relu = (_f16x3_ok(h, w0.shape[1], w0.shape[0]) and _f16x3_ok(h, w1.shape[1], w1.shape[0])
                      and bool(_lib.lib().vcnf_linear_wgrad_supported(w0.shape[1], w0.shape[0])))
        ctx.fused_relu = fused_relu
        if fused_relu:
            # both ReLUs ride on the split-half kernels: relu(h) is applied while h is read, relu(a) before a is stored -
            # neither activation gets a pass over memory of its own; h itself is kept for the backward pass (its sign
            # is relu(h)'s mask, the weight-gradient kernel applies the ReLU on load)
            t0 = h
            t1 = _lib.linear_f16x3(h, w0, b0, relu_in=True, relu_out=True)
        else:
            t0 = torch.relu(h)
            t1 = torch.relu_(_fwd(t0, w0, b0))
        c = _fwd(t1, w1, b1)
        if gate is not None:
            out = _lib.resblock_op(0, h, c, gate)
            ctx.save_for_backward(t0, t1, w0, w1, c, gate)
        else:
            out = h + c
            ctx.save_for_backward(t0, t1, w0, w1)
        ctx.gated = gate is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.gated:
            t0, t1, w0, w1, c, gate = ctx.saved_tensors
            g_c, g_gate = _lib.resblock_op(1, g, c, gate, two_outputs=True)
        else:
            t0, t1, w0, w1 = ctx.saved_tensors
            g_c, g_gate = g.contiguous(), None
        need = ctx.needs_input_grad
        # one reduction per cotangent: its weight-gradient and input-gradient launches share it
        am_c = _cot_amax(g_c, w1.shape[1], wgrad=need[4] or need[5])
        gw1, gb1 = _wgrad_or_torch(t1, g_c, amax=am_c) if (need[4] or need[5]) else (None, None)
        sq1 = w1.shape[0] == w1.shape[1] and _f16x3_ok(g_c, w1.shape[0], w1.shape[1])
        # square layers: the ReLU's backward (and, below, the skip connection's gradient) applied as the split-half kernel
        # stores the input gradient - no elementwise pass of their own
        g_a = (_lib.linear_f16x3(g_c, w1, None, input_grad=True, mask=t1, amax=am_c) if sq1
               else _lib.resblock_op(2, _dgrad(g_c, w1, am_c), t1))
        am_a = _cot_amax(g_a, w0.shape[1], wgrad=need[2] or need[3], dgrad=need[0])
        if ctx.fused_relu:          # t0 is the block input h: relu on load
            gw0, gb0 = _lib.linear_wgrad(t0, g_a, f16x3=TRAIN_MATRIX_PATH == 'fp16x3', relu_x=True, amax=am_a) if (need[2] or need[3]) else (None, None)
        else:
            gw0, gb0 = _wgrad_or_torch(t0, g_a, amax=am_a) if (need[2] or need[3]) else (None, None)
        sq0 = w0.shape[0] == w0.shape[1] and _f16x3_ok(g_a, w0.shape[0], w0.shape[1])
        if not need[0]:
            g_h = None
        elif sq0:
            g_h = _lib.linear_f16x3(g_a, w0, None, input_grad=True, mask=t0, addend=g, amax=am_a)
        else:
            g_h = _lib.resblock_op(3, _dgrad(g_a, w0, am_a), t0, g)
        return g_h, (g_gate if ctx.gated and need[1] else None), gw0, gb0, gw1, gb1


def residual_block(block, inputs, context):
    """``block(inputs, context)`` through ResBlockFn when the block is the plain training configuration this node
    covers (ReLU, no batch norm, inactive dropout, fp32 on the GPU, a batch at which the fused maps pay); else None."""
    from .fused import _is_relu
    if not (torch.is_grad_enabled() and inputs.is_cuda and inputs.dim() == 2 and inputs.dtype == torch.float32
            and inputs.shape[0] >= WGRAD_MIN_BATCH and not block.use_batch_norm and _is_relu(block.activation)
            and not (block.dropout.p > 0 and block.training)):
        return None
    l0, l1 = block.linear_layers
    if not (type(l0) is torch.nn.Linear and type(l1) is torch.nn.Linear and l0.bias is not None and l1.bias is not None):
        return None
    if not (inputs.requires_grad or l0.weight.requires_grad or l1.weight.requires_grad):
        return None
    gate = linear(block.context_layer, context) if context is not None else None
    return ResBlockFn.apply(inputs, gate, l0.weight, l0.bias, l1.weight, l1.bias)
