"""Decoders p(x | z) of the flow VAE.  ``log_prob(x, z)`` takes the data x [B, ...] and the latents z [B S, ...] (the S
samples of an item in consecutive rows) and returns [B S]; x is shared by its S rows, never repeated on the kernel path
(csrc/vae_ends.hip through vcnf_amd.vae_ends).
Reference: normflow/distributions/decoder.py.  Deliberate deviation: the Gaussian decoder's 2 pi constant counts the
elements of a data item."""
import torch
from torch import nn

from .. import vae_ends


def _samples_per_item(x, z):
    if len(x) == 0 or len(z) % len(x):
        raise ValueError("%d latent rows for %d data items" % (len(z), len(x)))
    return len(z) // len(x)


class BaseDecoder(nn.Module):
    def forward(self, z):
        """The parameters of p(x | z) for latents z [N, ...]."""
        raise NotImplementedError

    def log_prob(self, x, z):
        """log p(x | z) [B S] for x [B, ...] and z [B S, ...]."""
        raise NotImplementedError


class NNDiagGaussianDecoder(BaseDecoder):
    """Diagonal Gaussian whose mean and log variance are the two halves (along dim 1) of ``net(z)``.  ``fuse=False``
    (keyword only, not in the reference) forces the torch composition."""

    def __init__(self, net, *, fuse=True):
        super().__init__()
        self.net = net
        self.fuse = bool(fuse)

    def forward(self, z):
        mean, lv = vae_ends.split(self.net(z))
        return mean, torch.exp(0.5 * lv)

    def log_prob(self, x, z):
        return vae_ends.gauss_log_prob(x, self.net(z), _samples_per_item(x, z), 1, self.fuse)


class NNBernoulliDecoder(BaseDecoder):
    """Bernoulli with the scores (logits) ``net(z)``; x may hold any values in [0, 1].  ``fuse=False`` (keyword only,
    not in the reference) forces the torch composition."""

    def __init__(self, net, *, fuse=True):
        super().__init__()
        self.net = net
        self.fuse = bool(fuse)

    def forward(self, z):
        return torch.sigmoid(self.net(z))

    def log_prob(self, x, z):
        return vae_ends.bernoulli_log_prob(x, self.net(z), _samples_per_item(x, z), self.fuse)
