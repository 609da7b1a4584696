"""Stochastic layers (normflow 1.2, flows/stochastic.py): a Metropolis-Hastings random walk and Hamiltonian Monte Carlo
with a learnable step size and mass.  Names, arguments and parameter names are the reference's; both layers are their
own inverses.

Two paths, chosen per call.  With one of the kernel densities (TwoMoons, CircularGaussianMixture, RingMixture, or the
energies TwoModes, Sinusoidal, Sinusoidal_gap, Sinusoidal_split, Smiley of distributions/prior.py), ``z`` [B, 2] fp32 or
fp64 on the device and - for the walk - a DiagGaussianProposal over (2,), the layer is one launch of
csrc/stochastic.hip (vcnf_amd.fused_stochastic); NormalizingFlow takes consecutive HMC layers of one target and step
count in one launch.  Anything else - another Target subclass, another proposal, other shapes - evaluates the
reference's composition in torch, HMC with its score through ``autograd.grad`` on ``target.log_prob``.  Both paths draw
from torch's generator in the reference's order (HMC: ``randn_like(z)``, then ``rand`` of [B]; the walk, per step: the
proposal's ``randn``, then ``rand`` of [B]), so a seed gives the same chain on either."""
import torch

from .base import Flow


class MetropolisHastings(Flow):
    """Sampling through Metropolis Hastings: ``steps`` random-walk steps of ``proposal`` towards ``dist``.  The layer's
    log_det is zero; under autograd it is the identity in z."""

    def __init__(self, dist, proposal, steps):
        super().__init__()
        self.dist = dist
        self.proposal = proposal
        self.steps = steps

    def _torch_forward(self, z):
        num_samples = len(z)
        log_det = torch.zeros(num_samples, dtype=z.dtype, device=z.device)
        log_p = self.dist.log_prob(z)
        for i in range(self.steps):
            z_, log_p_diff = self.proposal(z)
            log_p_ = self.dist.log_prob(z_)
            w = torch.rand(num_samples, dtype=z.dtype, device=z.device)
            log_w_accept = log_p_ - log_p + log_p_diff
            w_accept = torch.clamp(torch.exp(log_w_accept), max=1)
            accept = w <= w_accept
            z = torch.where(accept.unsqueeze(1), z_, z)
            log_p = torch.where(accept, log_p_, log_p)
        return z, log_det

    def forward(self, z):
        from .. import fused_stochastic
        if fused_stochastic.covers_walk(self, z):
            return fused_stochastic.walk(self, z)
        return self._torch_forward(z)

    def inverse(self, z):
        return self.forward(z)


class HamiltonianMonteCarlo(Flow):
    """Flow layer using the HMC proposal of Stochastic Normalising Flows (arXiv 2002.06707): ``steps`` leapfrog steps
    towards ``target`` with the step sizes exp(log_step_size) and the masses exp(log_mass), then the accept / reject
    decision; log_det = log p(z) - log p(z_out)."""

    def __init__(self, target, steps, log_step_size, log_mass):
        super().__init__()
        self.target = target
        self.steps = steps
        self.register_parameter('log_step_size', torch.nn.Parameter(log_step_size))
        self.register_parameter('log_mass', torch.nn.Parameter(log_mass))

    def gradlogP(self, z):
        with torch.enable_grad():
            z_ = z.detach().requires_grad_()
            logp = self.target.log_prob(z_)
            return torch.autograd.grad(logp, z_, grad_outputs=torch.ones_like(logp))[0]

    def _torch_forward(self, z):
        p = torch.randn_like(z) * torch.exp(0.5 * self.log_mass)
        z_new = z.clone()
        p_new = p.clone()
        step_size = torch.exp(self.log_step_size)
        for i in range(self.steps):
            p_half = p_new - (step_size / 2.0) * -self.gradlogP(z_new)
            z_new = z_new + step_size * (p_half / torch.exp(self.log_mass))
            p_new = p_half - (step_size / 2.0) * -self.gradlogP(z_new)
        probabilities = torch.exp(
            self.target.log_prob(z_new) - self.target.log_prob(z)
            - 0.5 * torch.sum(p_new ** 2 / torch.exp(self.log_mass), 1)
            + 0.5 * torch.sum(p ** 2 / torch.exp(self.log_mass), 1))
        uniforms = torch.rand_like(probabilities)
        mask = uniforms < probabilities
        z_out = torch.where(mask.unsqueeze(1), z_new, z)
        return z_out, self.target.log_prob(z) - self.target.log_prob(z_out)

    def forward(self, z):
        from .. import fused_stochastic
        if fused_stochastic.covers(self, z):
            return fused_stochastic.run([self], z, None, 1.0)
        return self._torch_forward(z)

    def inverse(self, z):
        return self.forward(z)
