"""Dequantisation of categorical columns (the fork's normflow/nets/varquant.py; Ho et al. 2019, "Flow++"): integer codes
become points of the real line before the flows see them, and samples become codes again.

The fork's file is not available to this project: what is computed here is the published algorithm written per column,
and the tests compare it with a plain-torch restatement of the formulas below (tests/varquant_ref.py), not with the fork.

Rows are ``x [B, D]``; ``columns`` lists the C categorical columns and ``levels`` their numbers of levels K_c >= 1; a
categorical column holds the codes k = 0 .. K_c - 1 as floating values.  With a = alpha in [0, 1), sums over the
categorical columns in column order:

    prepare (draws u [B, C], uniform on [0, 1)):
        s = a/2 + (1 - a) u,   v = log(s) - log(1 - s),   ld = sum (log(1 - a) - log(s) - log(1 - s))
        ctx = 2 k / (K_c - 1) - 1     (0 where K_c = 1)
    merge (w [B, C]):
        variational:  n = sigmoid(w),  ld_n = sum (logsigmoid(w) + logsigmoid(-w))
        uniform:      n = w,           ld_n = 0
        y = (k + n) / K_c,   s = a/2 + (1 - a) y,   out[:, column] = log(s) - log(1 - s),   other columns as they are
        ld = ld_n + sum (log(1 - a) - log(K_c) - log(s) - log(1 - s))
    quantize (z [B, D]):
        t = z[:, column],   y = (sigmoid(t) - a/2) / (1 - a),   code = min(max(floor(y K_c), 0), K_c - 1)
        ld = sum (logsigmoid(t) + logsigmoid(-t) - log(1 - a) + log(K_c))      (the log-det of t -> y K_c)

``Dequantization`` merges the draws themselves: ONE launch of vcnf_dequant_merge_* (csrc/dequant.hip).
``VariationalDequantization`` is prepare (one launch), its flows in the forward direction on ``v`` with the context
``ctx`` (a flow with ``takes_context`` gets it; consecutive flows of one single-launch family are one launch, as in
``NormalizingFlow``), then merge (one launch); its log-det is the sum of the three, the quantity a model adds to
``log q`` of the transformed row for one draw of the variational bound.  Under autograd the flows go through the plain
``(z, log_det)`` contract and merge is one node (``autograd.DequantMergeFn``) whose backward is one launch.  The kernels
serve contiguous fp32 / fp64 rows on the device; everything else (CPU tensors, half precision, non-contiguous rows, a
draw or a sample that requires grad) evaluates the same formulas as a torch composition, differentiable in ``w``.

A code that is not integral or lies outside 0 .. K_c - 1 is not detected: it gives the formula's value.  ``alpha`` is a
plain attribute: it is not trainable and nothing of it enters the state dict."""
import math

import torch
from torch import nn
from torch.nn import functional as F

from .. import _lib, autograd
from ..core import _FlowWalks
from ..flows.base import fold_log_det


def _col_sum(t):
    """Sum over the columns of t [B, C] in column order."""
    total = torch.zeros(len(t), dtype=t.dtype, device=t.device)
    for c in range(t.shape[1]):
        total = total + t[:, c]
    return total


def _level_row(levels, like):
    return torch.tensor(list(levels), dtype=like.dtype, device=like.device)


def torch_prepare(x, columns, levels, u, alpha):
    """(v, ctx, ld) of the formulas above, one torch op per step."""
    k, big_k = x[:, list(columns)], _level_row(levels, x)
    s = alpha / 2 + (1 - alpha) * u
    log_s, log_t = torch.log(s), torch.log(1 - s)
    ctx = torch.where(big_k > 1, 2 * k / (big_k - 1) - 1, torch.zeros_like(k))
    return log_s - log_t, ctx, _col_sum(math.log(1 - alpha) - log_s - log_t)


def torch_merge(x, columns, levels, w, noise_is_logit, alpha):
    """(out, ld) of the formulas above, one torch op per step; differentiable in w and in the continuous columns of x."""
    k, big_k = x[:, list(columns)], _level_row(levels, x)
    if noise_is_logit:
        n, ld_n = torch.sigmoid(w), _col_sum(F.logsigmoid(w) + F.logsigmoid(-w))
    else:
        n, ld_n = w, 0
    y = (k.detach() + n) / big_k
    s = alpha / 2 + (1 - alpha) * y
    log_s, log_t = torch.log(s), torch.log(1 - s)
    out = x.clone()
    out[:, list(columns)] = log_s - log_t
    return out, ld_n + _col_sum(math.log(1 - alpha) - torch.log(big_k) - log_s - log_t)


def torch_quantize(z, columns, levels, alpha):
    """(codes, ld) of the formulas above, one torch op per step."""
    t, big_k = z[:, list(columns)], _level_row(levels, z)
    y = (torch.sigmoid(t) - alpha / 2) / (1 - alpha)
    code = torch.minimum(torch.maximum(torch.floor(y * big_k), torch.zeros_like(big_k)), big_k - 1)
    out = z.clone()
    out[:, list(columns)] = code
    return out, _col_sum(F.logsigmoid(t) + F.logsigmoid(-t) - math.log(1 - alpha) + torch.log(big_k))


class Dequantization(nn.Module):
    """Uniform dequantisation: the draws u ~ U[0, 1) are the noise.  ``use_kernels = False`` keeps every call on the torch
    composition."""

    noise_is_logit = False

    def __init__(self, alpha=1e-5):
        super().__init__()
        if not 0 <= alpha < 1:
            raise ValueError("%s: alpha must lie in [0, 1), got %r" % (type(self).__name__, alpha))
        self.alpha = float(alpha)
        self.use_kernels = True

    def _on_kernel(self, x):
        return self.use_kernels and x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.dim() == 2 \
            and x.shape[1] >= 1 and x.is_contiguous()

    @staticmethod
    def _draws(x, columns, noise):
        """The uniform draws [B, C] in the rows' dtype on their device: the caller's, or one ``torch.rand``."""
        if x.dim() != 2:
            raise ValueError("categorical rows must be [batch, features], got %s" % (tuple(x.shape),))
        shape = (len(x), len(columns))
        if noise is None:
            return torch.rand(shape, dtype=x.dtype, device=x.device)
        if tuple(noise.shape) != shape or noise.dtype != x.dtype or noise.device != x.device:
            raise ValueError("noise must be uniform draws %s in the rows' dtype %s on their device" % (list(shape), x.dtype))
        return noise

    def _merge(self, x, columns, levels, w, log_q, sign=1.0):
        """(out, log_q + sign * ld) of merge, accumulating in place when ``log_q`` is given."""
        if not (self._on_kernel(x) and w.is_cuda and w.dtype == x.dtype):
            return fold_log_det(*torch_merge(x, columns, levels, w, self.noise_is_logit, self.alpha), log_q, sign)
        slot, lv = _lib.column_tables(columns, levels, x.shape[1], x.device)
        w = w.contiguous()
        if autograd.needs_grad(x, w, log_q):
            out, ld = autograd.DequantMergeFn.apply(x, w, slot, lv, self.noise_is_logit, self.alpha)
            return fold_log_det(out, ld, log_q, sign)
        return _lib.dequant_merge(x, slot, lv, w, self.noise_is_logit, self.alpha, logdet=log_q, sign=sign)

    def dequantize(self, x, columns, levels, noise=None, log_q=None):
        """(xt, ld): the rows with their categorical columns made continuous and the log-det to add to ``log q(xt)``;
        ``log_q``: add it into this [B] tensor in place and return it.  ``noise``: uniform draws [B, C]."""
        return self._merge(x, columns, levels, self._draws(x, columns, noise), log_q)

    def quantize(self, z, columns, levels):
        """(x, ld): the categorical columns of z as integer codes and the log-det of the continuous map t -> y K_c in
        front of the floor, which a sampling pass subtracts."""
        if self._on_kernel(z) and not autograd.needs_grad(z):
            slot, lv = _lib.column_tables(columns, levels, z.shape[1], z.device)
            return _lib.quantize(z, slot, lv, self.alpha)
        return torch_quantize(z, columns, levels, self.alpha)


class VariationalDequantization(_FlowWalks, Dequantization):
    """Variational dequantisation: the noise is sigmoid(var_flows(logit(u) | ctx)), a learned distribution on [0, 1)
    conditioned on the row's categories.  ``flows`` holds ``var_flows``; the switches of the single-launch families
    (``fuse_rqs_stacks`` ...) are NormalizingFlow's."""

    noise_is_logit = True

    def __init__(self, var_flows, alpha=1e-5):
        super().__init__(alpha)
        self.flows = nn.ModuleList(var_flows)
        self._init_stack_switches()

    def dequantize(self, x, columns, levels, noise=None, log_q=None):
        u = self._draws(x, columns, noise)
        training = torch.is_grad_enabled() and (autograd.needs_grad(x, u, log_q) or any(p.requires_grad for p in self.parameters()))
        if self._on_kernel(x) and not autograd.needs_grad(x, u):
            slot, lv = _lib.column_tables(columns, levels, x.shape[1], x.device)
            # the walks subtract a forward log-det: the three parts are gathered with the opposite sign
            v, ctx, neg = _lib.dequant_prepare(x, slot, lv, u.contiguous(), self.alpha, sign=-1.0)
        else:
            v, ctx, ld = torch_prepare(x, columns, levels, u, self.alpha)
            neg = -ld
        if training:
            w, neg = self._plain_walk(v, neg, ctx, False)
        else:
            w, neg = self._walk(v, neg, ctx, False)
        out, neg = self._merge(x, columns, levels, w, neg, -1.0)
        if log_q is None:
            return out, (-neg if training else neg.neg_())
        return out, log_q.sub_(neg)
