"""normflow 1.2's flows/periodic.py and the UniformGaussian of its distributions/base.py restated in plain torch: what
the periodic tests compare vcnf_amd with.  ``with_noise`` is the reference's ``sample`` with its two draws supplied as one
[B, ndim] tensor in the order drawn (uniform columns first)."""
import math

import torch
from torch import nn


class PeriodicWrap(nn.Module):
    def __init__(self, ind, bound=1.0):
        super().__init__()
        self.ind = ind
        if torch.is_tensor(bound):
            self.register_buffer("bound", bound)
        else:
            self.bound = bound

    def forward(self, z):
        return z, torch.zeros(len(z), dtype=z.dtype, device=z.device)

    def inverse(self, z):
        z_ = z.clone()
        z_[..., self.ind] = torch.remainder(z_[..., self.ind] + self.bound, 2 * self.bound) - self.bound
        return z_, torch.zeros(len(z), dtype=z.dtype, device=z.device)


class PeriodicShift(nn.Module):
    def __init__(self, ind, bound=1.0, shift=0.0):
        super().__init__()
        self.ind = ind
        if torch.is_tensor(bound):
            self.register_buffer("bound", bound)
        else:
            self.bound = bound
        if torch.is_tensor(shift):
            self.register_buffer("shift", shift)
        else:
            self.shift = shift

    def forward(self, z):
        z_ = z.clone()
        z_[..., self.ind] = torch.remainder(z_[..., self.ind] + self.shift + self.bound, 2 * self.bound) - self.bound
        return z_, torch.zeros(len(z), dtype=z.dtype, device=z.device)

    def inverse(self, z):
        z_ = z.clone()
        z_[..., self.ind] = torch.remainder(z_[..., self.ind] - self.shift + self.bound, 2 * self.bound) - self.bound
        return z_, torch.zeros(len(z), dtype=z.dtype, device=z.device)


class UniformGaussian(nn.Module):
    def __init__(self, ndim, ind, scale=None):
        super().__init__()
        self.ndim = ndim
        if isinstance(ind, int):
            ind = [ind]
        if torch.is_tensor(ind):
            self.register_buffer("ind", ind.to(torch.long))
        else:
            self.register_buffer("ind", torch.tensor(ind, dtype=torch.long))
        ind_ = []
        for i in range(self.ndim):
            if i not in self.ind:
                ind_ += [i]
        self.register_buffer("ind_", torch.tensor(ind_, dtype=torch.long))
        perm_ = torch.cat((self.ind, self.ind_))
        inv_perm_ = torch.zeros_like(perm_)
        for i in range(self.ndim):
            inv_perm_[perm_[i]] = i
        self.register_buffer("inv_perm", inv_perm_)
        if scale is None:
            self.register_buffer("scale", torch.ones(self.ndim))
        else:
            self.register_buffer("scale", scale)

    def forward(self, num_samples=1):
        z = self.sample(num_samples)
        return z, self.log_prob(z)

    def sample(self, num_samples=1):
        eps_u = torch.rand((num_samples, len(self.ind)), dtype=self.scale.dtype, device=self.scale.device) - 0.5
        eps_g = torch.randn((num_samples, len(self.ind_)), dtype=self.scale.dtype, device=self.scale.device)
        z = torch.cat((eps_u, eps_g), -1)
        z = z[..., self.inv_perm]
        return self.scale * z

    def with_noise(self, eps):
        k = len(self.ind)
        z = torch.cat((eps[..., :k] - 0.5, eps[..., k:]), -1)
        z = self.scale * z[..., self.inv_perm]
        return z, self.log_prob(z)

    def log_prob(self, z):
        log_p_u = torch.broadcast_to(-torch.log(self.scale[self.ind]), (len(z), -1))
        log_p_g = -0.5 * math.log(2 * math.pi) - torch.log(self.scale[self.ind_]) \
            - 0.5 * torch.pow(z[..., self.ind_] / self.scale[self.ind_], 2)
        return torch.sum(log_p_u, -1) + torch.sum(log_p_g, -1)
