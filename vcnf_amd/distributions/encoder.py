"""Encoders q(z | x) of the flow VAE.  ``forward(x, num_samples)`` returns (z [B, S, ...], log q [B, S]) and
``log_prob(z, x)`` log q [B, S] for z [B, S, ...].  ``Dirac``, ``Uniform`` and ``ConstDiagGaussian`` are plain torch;
``NNDiagGaussian`` runs its draw and its density on csrc/vae_ends.hip (vcnf_amd.vae_ends).
Reference: normflow/distributions/encoder.py."""
import numpy as np
import torch
from torch import nn

from .. import vae_ends


def _zeros_like_samples(z, value=0.0):
    """[B, S] filled with ``value``, where z lives (the reference creates it on the CPU)."""
    return torch.full(z.shape[:2], value, dtype=z.dtype, device=z.device)


class BaseEncoder(nn.Module):
    """Base distribution of a flow VAE: a conditional distribution q(z | x)."""

    def forward(self, x, num_samples=1):
        """(z [B, S, ...], log q(z | x) [B, S]) for a batch x [B, ...]."""
        raise NotImplementedError

    def log_prob(self, z, x):
        """log q(z | x) [B, S] of z [B, S, ...]."""
        raise NotImplementedError


class Dirac(BaseEncoder):
    """z = x, repeated num_samples times; log q = 0."""

    def forward(self, x, num_samples=1):
        z = x.unsqueeze(1).repeat(1, num_samples, *([1] * (x.dim() - 1)))
        return z, _zeros_like_samples(z)

    def log_prob(self, z, x):
        return _zeros_like_samples(z)


class Uniform(BaseEncoder):
    """z uniform on [zmin, zmax) in the shape of x; log q = -log(zmax - zmin)."""

    def __init__(self, zmin=0.0, zmax=1.0):
        super().__init__()
        self.zmin = zmin
        self.zmax = zmax
        self.log_q = -np.log(zmax - zmin)

    def forward(self, x, num_samples=1):
        z = x.unsqueeze(1).repeat(1, num_samples, *([1] * (x.dim() - 1))).uniform_(self.zmin, self.zmax)
        return z, _zeros_like_samples(z, self.log_q)

    def log_prob(self, z, x):
        return _zeros_like_samples(z, self.log_q)


class ConstDiagGaussian(BaseEncoder):
    """Diagonal Gaussian that does not depend on x: parameters ``loc`` and ``scale`` (the standard deviation) of shape
    (1, 1, d)."""

    def __init__(self, loc, scale):
        super().__init__()
        loc, scale = (t.detach() if torch.is_tensor(t) else torch.as_tensor(t, dtype=torch.get_default_dtype())
                      for t in (loc, scale))
        self.d = loc.numel()
        self.loc = nn.Parameter(loc.reshape(1, 1, self.d).clone())
        self.scale = nn.Parameter(scale.to(loc.dtype).reshape(1, 1, -1).expand(1, 1, self.d).clone())

    def forward(self, x=None, num_samples=1):
        batch = len(x) if x is not None else 1
        eps = torch.randn((batch, num_samples, self.d), dtype=self.loc.dtype, device=self.loc.device)
        z = self.loc + self.scale * eps
        log_q = -0.5 * self.d * vae_ends.LOG_2PI - torch.sum(torch.log(self.scale) + 0.5 * eps ** 2, 2)
        return z, log_q

    def log_prob(self, z, x):
        if z.dim() == 1:
            z = z.unsqueeze(0)
        if z.dim() == 2:
            z = z.unsqueeze(0)
        return -0.5 * self.d * vae_ends.LOG_2PI - torch.sum(torch.log(self.scale) + 0.5 * ((z - self.loc) / self.scale) ** 2, 2)


class NNDiagGaussian(BaseEncoder):
    """Diagonal Gaussian whose mean and log variance are the two halves (along dim 1) of ``net(x)``.  The draw with its
    log q, and ``log_prob``, are one kernel launch and one autograd node each; ``fuse=False`` (keyword only, not in the
    reference) forces the torch composition, which also serves whatever the kernels do not cover (vcnf_amd.vae_ends)."""

    def __init__(self, net, *, fuse=True):
        super().__init__()
        self.net = net
        self.fuse = bool(fuse)

    def forward(self, x, num_samples=1):
        h = self.net(x)
        mean, _ = vae_ends.split(h)
        eps = torch.randn((len(x), num_samples) + tuple(mean.shape[1:]), dtype=h.dtype, device=h.device)
        return vae_ends.encode(h, eps, self.fuse)

    def log_prob(self, z, x):
        """z [B, S, ...] (or [B, ...]: one sample per item) -> [B, S]."""
        h = self.net(x)
        if z.dim() == h.dim():
            z = z.unsqueeze(1)
        b, s = z.shape[:2]
        return vae_ends.gauss_log_prob(z.reshape((b * s,) + tuple(z.shape[2:])), h, 1, s, self.fuse).reshape(b, s)
