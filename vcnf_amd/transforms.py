"""Transforms between data space and the space a flow models (normflow 1.2 transforms.py): ``Logit`` maps [0, 1] data
to the real line through ``alpha + (1 - 2 alpha) x``, ``Shift`` moves it by a constant.  They go into the ``transform=``
slot of ``MultiscaleFlow`` or, being ``Flow``s, into a ``NormalizingFlow``'s list.

With ``beta = 1 - 2 alpha`` and D elements per item, ``Logit`` is

    forward(z)  (sampling):  y = (sigmoid(z) - alpha) / beta
                             log_det = -D log(beta) + sum(logsigmoid(z) + logsigmoid(-z))
    inverse(x)  (density):   u = alpha + beta x,  z = log(u) - log(1 - u)
                             log_det = D log(beta) - sum(log(u)) - sum(log(1 - u))

On the device a direction is ONE launch of vcnf_logit_* (csrc/logit.hip) over a contiguous fp32 / fp64 tensor [B, ...],
and under autograd one node whose backward is one launch; an input that does not require grad (data) gets no node.
``forward_into`` / ``inverse_into`` (what NormalizingFlow calls) add the log-det into ``log_q`` inside the kernel.
``inverse_u8`` starts from the bytes of an image: dequantisation noise, scaling and the density direction in one launch.
The same formulas as a torch composition, differentiable in the input, serve what the kernel does not: CPU tensors,
half precision and non-contiguous inputs.  ``alpha`` is a plain attribute: nothing enters the state dict and it is not
trainable."""
import math

import torch
from torch.nn import functional as F

from .flows.base import Flow, fold_log_det
from . import _lib, autograd


def _row_sum(t):
    return t.reshape(len(t), math.prod(t.shape[1:])).sum(1)


class Logit(Flow):
    def __init__(self, alpha=0.05):
        super().__init__()
        if not 0 <= alpha < 0.5:
            raise ValueError("Logit: alpha must lie in [0, 0.5), got %r" % (alpha,))
        self.alpha = float(alpha)

    def _torch(self, x, inverse):
        """The formulas above, one torch op per step."""
        alpha, beta = self.alpha, 1 - 2 * self.alpha
        d = math.prod(x.shape[1:])
        if inverse:
            u = alpha + beta * x
            log_u, log_v = torch.log(u), torch.log(1 - u)
            return log_u - log_v, d * math.log(beta) - _row_sum(log_u) - _row_sum(log_v)
        y = (torch.sigmoid(x) - alpha) / beta
        return y, -d * math.log(beta) + _row_sum(F.logsigmoid(x) + F.logsigmoid(-x))

    @staticmethod
    def _on_kernel(x):
        return x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.dim() >= 1 and math.prod(x.shape[1:]) >= 1 \
            and x.is_contiguous()

    def _run(self, x, inverse, log_q=None, sign=1.0):
        if not self._on_kernel(x):
            return fold_log_det(*self._torch(x, inverse), log_q, sign)
        if autograd.needs_grad(x, log_q):
            return fold_log_det(*autograd.LogitFn.apply(x, self.alpha, inverse), log_q, sign)
        return _lib.logit(x, self.alpha, inverse, logdet=log_q, sign=sign)

    def forward(self, z):
        return self._run(z, False)

    def inverse(self, x):
        return self._run(x, True)

    def forward_into(self, z, log_q):
        return self._run(z, False, log_q, -1.0)[0]

    def inverse_into(self, x, log_q):
        return self._run(x, True, log_q, 1.0)[0]

    def inverse_u8(self, x_u8, noise=None, jitter=1 / 256., scale=255 / 256., dtype=torch.float32):
        """(z, log_det) of the density direction at ``(x_u8 / 255 + noise * jitter) * scale``: bytes to the flow's input
        with uniform dequantisation.  ``noise``: uniform [0, 1) values of the bytes' shape in ``dtype`` on their device;
        None draws them with one ``torch.rand``.  One launch for a contiguous uint8 device tensor; the same chain as a
        torch composition elsewhere."""
        if x_u8.dtype != torch.uint8:
            raise TypeError("Logit.inverse_u8 takes a torch.uint8 tensor, got %s" % x_u8.dtype)
        if noise is None:
            noise = torch.rand(x_u8.shape, dtype=dtype, device=x_u8.device)
        elif noise.shape != x_u8.shape or noise.dtype != dtype or noise.device != x_u8.device:
            raise ValueError("Logit.inverse_u8: noise must have the bytes' shape and device and the dtype %s" % dtype)
        if self._on_kernel(noise) and x_u8.is_contiguous() and not autograd.needs_grad(noise):
            return _lib.logit_inverse_u8(x_u8, noise, jitter, scale, self.alpha)
        return self.inverse((x_u8.to(dtype) / 255 + noise * jitter) * scale)


class Shift(Flow):
    """``forward: z - shift``, ``inverse: z + shift``, log-det zero.  The results are new tensors (the reference's
    ``z -= shift`` writes into the caller's)."""

    def __init__(self, shift=0.):
        super().__init__()
        self.shift = shift

    def forward(self, z):
        return z - self.shift, torch.zeros(len(z), dtype=z.dtype, device=z.device)

    def inverse(self, z):
        return z + self.shift, torch.zeros(len(z), dtype=z.dtype, device=z.device)
