"""normflow 1.2, sampling/hais.py: Hamiltonian annealed importance sampling (Sohl-Dickstein and Culpepper, 2012)."""
import torch

from .. import fused_stochastic
from ..distributions.linear_interpolation import LinearInterpolation
from ..flows.stochastic import HamiltonianMonteCarlo


class HAIS:
    """Annealed importance sampling from ``prior`` to ``target`` with one HamiltonianMonteCarlo layer per inner beta:
    ``betas`` runs from 1 = betas[0] down to 0 = betas[n], and layer j targets the LinearInterpolation of target and
    prior with the weight betas[n - 1 - j].  A plain object, as in the reference; names and arguments are its own.

    ``fuse`` (keyword only, not in the reference): where the kernel covers the layers - a kernel target, a DiagGaussian
    prior over (2,), samples on the device (vcnf_amd.fused_stochastic) - ``sample`` takes each run of them in one launch
    of vcnf_hmc_annealed_stack_*, and outside autograd the last term of the weights, log p(samples), from that launch as
    well.  With ``fuse=False`` it walks the layers of such a run one by one, each its own launch, and adds their log-dets
    in the run's order, so both settings give the same samples and weights bit for bit under one seed.  Layers the
    kernel does not cover evaluate their torch composition and add to the weights as the reference writes it."""

    def __init__(self, betas, prior, target, num_leapfrog, step_size, log_mass, *, fuse=True):
        self.prior = prior
        self.target = target
        self.fuse = fuse
        self.layers = []
        n = betas.shape[0] - 1
        for i in range(n - 1, 0, -1):
            intermediate_target = LinearInterpolation(self.target, self.prior, betas[i])
            self.layers += [HamiltonianMonteCarlo(intermediate_target, num_leapfrog, torch.log(step_size), log_mass)]

    def sample(self, num_samples):
        """(samples, log_weights) of ``num_samples`` annealed chains."""
        samples, log_weights = self.prior.forward(num_samples)
        log_weights = -log_weights
        last = None                                   # log p(samples) where the final launch has written it
        i, n = 0, len(self.layers)
        while i < n:
            plan = fused_stochastic.plan(self.layers, i, samples)
            if plan is None:
                samples, add = self.layers[i].forward(samples)
                i += 1
            else:
                end, flows = plan
                if self.fuse:
                    want = end == n and fused_stochastic.annealed(flows[0].target) and not torch.is_grad_enabled()
                    samples, add, recorded, *rest = fused_stochastic.launch(flows, samples, want_logp=want)
                    last = rest[0] if rest else None
                else:
                    samples, add = flows[0].forward(samples)
                    for layer in flows[1:]:
                        samples, more = layer.forward(samples)
                        add = add + more
                i = end
            log_weights += add
        log_weights += self.target.log_prob(samples) if last is None else last
        return samples, log_weights
