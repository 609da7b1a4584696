"""Host side of csrc/vae_ends.hip: the three end caps of the flow VAE - the reparametrised draw of the amortised Gaussian
encoder with its log q, the Gaussian log-likelihood (the encoder's ``log_prob(z, x)`` and the Gaussian decoder) and the
Bernoulli log-likelihood - each as one kernel launch and one autograd node, or as the torch composition of the same
arithmetic.

A parameter tensor ``h`` is a net's output [rows, 2 C, ...]: the mean in the first half of the channels, the log variance
in the second, which as a contiguous row is [mean (D) | lv (D)] with D = C x the trailing sizes.  What the S samples of a
data item share (``h`` of the encoder, ``x`` of the decoders) is never repeated on the kernel path.

The kernels run when every tensor is fp32 or fp64 (one dtype) on one HIP device and, whenever autograd records the call,
S <= ``_lib.VAE_MAX_SAMPLES`` (a lane of the VJP kernels walks the S rows of an item).  Everything else - CPU tensors,
half precision, mixed dtypes, a draw ``eps`` or Bernoulli data ``x`` that requires grad (the kernels have no gradient for
them), S over the limit, ``fuse=False`` - evaluates the composition: nothing raises and no gradient is silently zero.
"""
import math

import torch

from . import _lib
from .autograd import VaeBernoulliLogProbFn, VaeEncodeFn, VaeGaussLogProbFn, needs_grad

LOG_2PI = math.log(2 * math.pi)


def on_kernels(*tensors):
    """Every tensor is fp32 or fp64, of one dtype, on one HIP device."""
    first = tensors[0]
    return first.is_cuda and first.dtype in (torch.float32, torch.float64) and \
        all(t.dtype == first.dtype and t.device == first.device for t in tensors[1:])


def _fits(samples, *tensors):
    """The VJP kernels cover the call: nothing to differentiate, or at most VAE_MAX_SAMPLES rows per item."""
    return samples <= _lib.VAE_MAX_SAMPLES or not needs_grad(*tensors)


def split(h):
    """(mean, log variance) of a parameter tensor [rows, 2 C, ...]."""
    if h.dim() < 2 or h.shape[1] % 2:
        raise ValueError("expected [mean | log variance] along dim 1 of the net's output, got %s" % (tuple(h.shape),))
    c = h.shape[1] // 2
    return h[:, :c], h[:, c:]


def _feature_dims(t, first):
    return list(range(first, t.dim()))


def encode(h, eps, fuse=True):
    """(z like eps, log q [B, S]) for h [B, 2 C, ...] and the standard-normal draw eps [B, S, C, ...]:
    z = mean + exp(lv / 2) eps, log q = -D/2 log 2 pi - sum (lv / 2 + eps^2 / 2)."""
    if fuse and on_kernels(h, eps) and not needs_grad(eps) and _fits(eps.shape[1], h):
        if needs_grad(h):
            return VaeEncodeFn.apply(h, eps)
        return _lib.vae_encode(h.detach(), eps)
    mean, lv = split(h)
    mean, lv = mean.unsqueeze(1), lv.unsqueeze(1)
    z = mean + torch.exp(0.5 * lv) * eps
    d = z[0, 0].numel()
    return z, -0.5 * d * LOG_2PI - torch.sum(0.5 * lv + 0.5 * eps ** 2, _feature_dims(z, 2))


def gauss_log_prob(v, h, v_div=1, h_div=1, fuse=True):
    """log density [N] of v [N / v_div, C, ...] under the Gaussians of h [N / h_div, 2 C, ...] (one divisor is 1; row n
    reads v[n // v_div] and h[n // h_div]): -D/2 log 2 pi - 1/2 sum (lv + (v - mean)^2 exp(-lv))."""
    if fuse and on_kernels(v, h) and _fits(max(v_div, h_div), v, h):
        if needs_grad(v, h):
            return VaeGaussLogProbFn.apply(v, h, v_div, h_div)
        return _lib.vae_gauss_log_prob(v.detach(), h.detach(), v_div, h_div)
    mean, lv = split(h)
    if v_div > 1:
        v = v.repeat_interleave(v_div, 0)
    if h_div > 1:
        mean, lv = mean.repeat_interleave(h_div, 0), lv.repeat_interleave(h_div, 0)
    d = v[0].numel()
    return -0.5 * d * LOG_2PI - 0.5 * torch.sum(lv + (v - mean) ** 2 * torch.exp(-lv), _feature_dims(v, 1))


def log_sigmoid(a):
    """log sigmoid(a) = -max(-a, 0) - log1p(exp(-|a|))."""
    return -torch.relu(-a) - torch.log1p(torch.exp(-torch.abs(a)))


def bernoulli_log_prob(x, score, x_div=1, fuse=True):
    """log likelihood [N] of the data x [N / x_div, ...] in [0, 1] under the scores [N, ...] (row n reads x[n // x_div]):
    sum (x log sigmoid(a) + (1 - x) log sigmoid(-a))."""
    if fuse and on_kernels(x, score) and not needs_grad(x) and _fits(x_div, score):
        if needs_grad(score):
            return VaeBernoulliLogProbFn.apply(x, score, x_div)
        return _lib.vae_bernoulli_log_prob(x, score.detach(), x_div)
    if x_div > 1:
        x = x.repeat_interleave(x_div, 0)
    x = x.reshape(score.shape)
    return torch.sum(x * log_sigmoid(score) + (1 - x) * log_sigmoid(-score), _feature_dims(score, 1))
