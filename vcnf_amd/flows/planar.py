"""Planar flow (Rezende & Mohamed 2015): z' = z + u_hat h(w.z + b).  ``forward`` (and the algebraic ``inverse`` of the
leaky_relu variant) is csrc/planar_radial.hip with a run of one layer (vcnf_amd.fused_planar); NormalizingFlow takes
consecutive Planar / Radial layers in one launch.  Beyond the kernel's feature limit, and for ``inverse`` under
autograd, the layer evaluates the reference's own composition in torch.
Reference: normflow/flows/planar.py."""
import numpy as np
import torch
from torch import nn

from .base import Flow
from .. import autograd

NEGATIVE_SLOPE = 0.2


def _sum(t):
    return t.reshape(len(t), -1).sum(1)


def _slope_where_negative(lin):
    """leaky_relu's derivative at lin, in lin's dtype (a bool tensor times a Python float would be fp32)."""
    return torch.where(lin < 0, torch.full_like(lin, NEGATIVE_SLOPE), torch.ones_like(lin))


class Planar(Flow):
    def __init__(self, shape, act="tanh", u=None, w=None, b=None):
        super().__init__()
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        lim_w = np.sqrt(2.0 / np.prod(shape))
        lim_u = np.sqrt(2)
        if u is not None:
            self.u = nn.Parameter(u)
        else:
            self.u = nn.Parameter(torch.empty(shape)[None])
            nn.init.uniform_(self.u, -lim_u, lim_u)
        if w is not None:
            self.w = nn.Parameter(w)
        else:
            self.w = nn.Parameter(torch.empty(shape)[None])
            nn.init.uniform_(self.w, -lim_w, lim_w)
        self.b = nn.Parameter(b) if b is not None else nn.Parameter(torch.zeros(1))
        if act not in ("tanh", "leaky_relu"):
            raise NotImplementedError('Nonlinearity is not implemented.')
        self.act = act

    def u_hat(self):
        """u moved along w so that w.u_hat >= -1: the map stays invertible."""
        inner = torch.sum(self.w * self.u)
        return self.u + (torch.log(1 + torch.exp(inner)) - 1 - inner) * self.w / torch.sum(self.w ** 2)

    def _torch_forward(self, z):
        dims = (-1,) + (1,) * (z.dim() - 1)
        lin = _sum(self.w * z) + self.b
        u = self.u_hat()
        if self.act == "tanh":
            h, h_ = torch.tanh(lin), 1 / torch.cosh(lin) ** 2
        else:
            h_ = _slope_where_negative(lin)
            h = h_ * lin
        return z + u * h.reshape(dims), torch.log(torch.abs(1 + torch.sum(self.w * u) * h_))

    def _torch_inverse(self, z):
        dims = (-1,) + (1,) * (z.dim() - 1)
        lin = _sum(self.w * z) + self.b
        a = _slope_where_negative(lin)
        u = a.reshape(dims) * self.u_hat()
        inner = _sum(self.w * u)
        return z - u * (lin / (1 + inner)).reshape(dims), -torch.log(torch.abs(1 + inner))

    def forward(self, z):
        from .. import fused_planar
        if fused_planar.covers(self, z):
            return fused_planar.run([self], z, False, None, 1.0)
        return self._torch_forward(z)

    def inverse(self, z):
        if self.act != "leaky_relu":
            raise NotImplementedError('This flow has no algebraic inverse.')
        from .. import fused_planar
        if fused_planar.covers(self, z) and not autograd.needs_grad(z, self.u, self.w, self.b):
            return fused_planar.run([self], z, True, None, 1.0)
        return self._torch_inverse(z)
