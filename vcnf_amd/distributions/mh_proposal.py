"""Proposal distributions of the Metropolis-Hastings layer (normflow 1.2, distributions/mh_proposal.py): the base class
and the diagonal Gaussian random walk.  Constructor arguments, attribute and buffer names are the reference's.  These are
a draw and a handful of elementwise ops in torch on whatever device ``z`` is on; with a kernel target the layer itself
(vcnf_amd.flows.MetropolisHastings) takes the draws and the proposal's ``scale`` into one launch of csrc/stochastic.hip."""
import numpy as np
import torch
from torch import nn


class MHProposal(nn.Module):
    """Proposal distribution for the Metropolis Hastings algorithm."""

    def __init__(self):
        super().__init__()

    def sample(self, z):
        """Sample a new state z_ given z."""
        raise NotImplementedError

    def log_prob(self, z_, z):
        """log p(z_ | z)."""
        raise NotImplementedError

    def forward(self, z):
        """(z_, log p(z | z_) - log p(z_ | z)) for a fresh proposal."""
        raise NotImplementedError


class DiagGaussianProposal(MHProposal):
    """Diagonal Gaussian centred at the previous sample: z_ = eps scale + z.  ``scale`` broadcasts against z; it is kept
    as the buffer ``scale`` with a leading batch dimension, as the reference does."""

    def __init__(self, shape, scale):
        super().__init__()
        self.shape = shape
        self.scale_cpu = torch.tensor(scale)
        self.register_buffer("scale", self.scale_cpu.unsqueeze(0))

    def sample(self, z):
        num_samples = len(z)
        eps = torch.randn((num_samples,) + self.shape, dtype=z.dtype, device=z.device)
        z_ = eps * self.scale + z
        return z_

    def log_prob(self, z_, z):
        log_p = - 0.5 * np.prod(self.shape) * np.log(2 * np.pi) \
                - torch.sum(torch.log(self.scale) + 0.5 * torch.pow((z_ - z) / self.scale, 2), list(range(1, z.dim())))
        return log_p

    def forward(self, z):
        num_samples = len(z)
        eps = torch.randn((num_samples,) + self.shape, dtype=z.dtype, device=z.device)
        z_ = eps * self.scale + z
        log_p_diff = torch.zeros(num_samples, dtype=z.dtype, device=z.device)
        return z_, log_p_diff
