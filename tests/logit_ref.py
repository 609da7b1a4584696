"""The image data end caps restated in plain torch from normflow 1.2 (transforms.py: Logit, Shift; utils/preprocessing.py:
Logit, Jitter, Scale) and the byte chain in front of them as a torch composition: what the logit tests compare vcnf_amd
with.  One torch op per step, Python scalars as operands."""
import math

import torch
from torch import nn
from torch.nn import functional as F


def sum_except_batch(t):
    return t.reshape(len(t), math.prod(t.shape[1:])).sum(1)


class LogitRef(nn.Module):
    def __init__(self, alpha=0.05):
        super().__init__()
        self.alpha = alpha

    def forward(self, z):
        beta = 1 - 2 * self.alpha
        d = math.prod(z.shape[1:])
        ls = sum_except_batch(F.logsigmoid(z) + F.logsigmoid(-z))
        y = (torch.sigmoid(z) - self.alpha) / beta
        return y, -d * math.log(beta) + ls

    def inverse(self, x):
        beta = 1 - 2 * self.alpha
        d = math.prod(x.shape[1:])
        u = self.alpha + beta * x
        log_u, log_v = torch.log(u), torch.log(1 - u)
        return log_u - log_v, d * math.log(beta) - sum_except_batch(log_u) - sum_except_batch(log_v)


class ShiftRef(nn.Module):
    def __init__(self, shift=0.):
        super().__init__()
        self.shift = shift

    def forward(self, z):
        return z - self.shift, torch.zeros(len(z), dtype=z.dtype, device=z.device)

    def inverse(self, z):
        return z + self.shift, torch.zeros(len(z), dtype=z.dtype, device=z.device)


class PreLogit:
    def __init__(self, alpha=0):
        self.alpha = alpha

    def __call__(self, x):
        x_ = self.alpha + (1 - self.alpha) * x
        return torch.log(x_ / (1 - x_))

    def inverse(self, x):
        return (torch.sigmoid(x) - self.alpha) / (1 - self.alpha)


class Jitter:
    def __init__(self, scale=1. / 256):
        self.scale = scale

    def __call__(self, x):
        return x + torch.rand_like(x) * self.scale


class Scale:
    def __init__(self, scale=255. / 256):
        self.scale = scale

    def __call__(self, x):
        return x * self.scale


def bytes_to_unit(x_u8, noise, jitter=1 / 256., scale=255 / 256.):
    """bytes -> jitter -> scale with the uniform draws supplied, in the dtype of ``noise``."""
    x = x_u8.to(noise.dtype) / 255
    x = x + noise * jitter
    return x * scale


def inverse_u8(x_u8, noise, alpha, jitter=1 / 256., scale=255 / 256.):
    return LogitRef(alpha).inverse(bytes_to_unit(x_u8, noise, jitter, scale))


def inverse_vjp(x, alpha, g_z, g_ld):
    """The closed form of the density direction's VJP."""
    beta = 1 - 2 * alpha
    u = alpha + beta * x
    g = g_ld.reshape((-1,) + (1,) * (x.dim() - 1))
    return beta / (u * (1 - u)) * (g_z - g * (1 - 2 * u))


def forward_vjp(z, alpha, g_y, g_ld):
    """The closed form of the sampling direction's VJP."""
    beta = 1 - 2 * alpha
    s = torch.sigmoid(z)
    g = g_ld.reshape((-1,) + (1,) * (z.dim() - 1))
    return g_y * s * (1 - s) / beta + g * (1 - 2 * s)


def bits_per_dim(log_prob, dims, levels=256):
    return -log_prob / (dims * math.log(2)) + math.log2(levels)
