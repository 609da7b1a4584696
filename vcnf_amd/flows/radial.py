"""Radial flow (Rezende & Mohamed 2015): z' = z + h(r) (z - z_0), r = |z - z_0|, h = beta / (|alpha| + r).  ``forward``
is csrc/planar_radial.hip with a run of one layer (vcnf_amd.fused_planar); NormalizingFlow takes consecutive Planar /
Radial layers in one launch.  Beyond the kernel's feature limit the layer evaluates the reference's own composition in
torch.  There is no algebraic inverse.
Reference: normflow/flows/radial.py."""
import numpy as np
import torch
from torch import nn

from .base import Flow


class Radial(Flow):
    def __init__(self, shape, z_0=None):
        super().__init__()
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.d_cpu = torch.prod(torch.tensor(shape))
        self.register_buffer('d', self.d_cpu)
        lim = 1.0 / np.prod(shape)
        self.beta = nn.Parameter(torch.empty(1))
        nn.init.uniform_(self.beta, -lim - 1.0, lim - 1.0)
        self.alpha = nn.Parameter(torch.empty(1))
        nn.init.uniform_(self.alpha, -lim, lim)
        self.z_0 = nn.Parameter(z_0) if z_0 is not None else nn.Parameter(torch.randn(shape)[None])

    def _torch_forward(self, z):
        beta = torch.log(1 + torch.exp(self.beta)) - torch.abs(self.alpha)
        dz = z - self.z_0
        r = torch.linalg.vector_norm(dz, dim=list(range(1, self.z_0.dim())), keepdim=True)
        h_arr = beta / (torch.abs(self.alpha) + r)
        h_arr_ = -beta * r / (torch.abs(self.alpha) + r) ** 2
        log_det = (self.d_cpu - 1) * torch.log(1 + h_arr) + torch.log(1 + h_arr + h_arr_)
        return z + h_arr * dz, log_det.reshape(-1)

    def forward(self, z):
        from .. import fused_planar
        if fused_planar.covers(self, z):
            return fused_planar.run([self], z, False, None, 1.0)
        return self._torch_forward(z)
