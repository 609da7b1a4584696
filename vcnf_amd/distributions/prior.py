"""Energy densities of normflow 1.2 (normflows/distributions/prior.py), the test energies of Rezende & Mohamed that the
reference's planar and radial examples train ``reverse_kld`` against: TwoModes, Sinusoidal, Sinusoidal_gap,
Sinusoidal_split and Smiley, with their base class.  As in the reference they are plain objects, not modules; their
parameters are Python numbers kept as attributes of the reference's names and may be reassigned.

On a device tensor ``z`` [B, 2] in fp32 or fp64, ``log_prob`` is one launch of vcnf_target_log_prob_*
(csrc/target_density.hip) and under autograd one node whose backward is a multiply by the score the launch wrote, as
for the targets of target.py; the stochastic layers and the HAIS sampler evaluate the same device functions inside their
own kernels (vcnf_amd.fused_stochastic).  Everything else - host tensors, half precision, other shapes - evaluates the
same formulas (include/vcnf_hip.h) as a torch composition, differentiable in ``z``.  One departure from the reference:
the two-branch log of Sinusoidal_gap and Sinusoidal_split is ``torch.logaddexp``, on either path, where the reference's
log(exp a + exp b) is -inf in fp32 a few scales off both ridges.  ImagePrior is out of scope."""
import numpy as np
import torch

from .target import _KernelDensity
from .. import _lib


def _kernel_inputs(z):
    return torch.is_tensor(z) and z.is_cuda and z.dim() == 2 and z.shape[1] == 2 and z.dtype in (torch.float32, torch.float64)


class PriorDistribution:
    def __init__(self):
        raise NotImplementedError

    def log_prob(self, z):
        """
        :param z: value or batch of latent variable
        :return: log probability of the distribution for z
        """
        raise NotImplementedError


class _KernelPrior(_KernelDensity, PriorDistribution):
    """Shared end of the five energies: the kernel on device inputs [B, 2], the torch composition otherwise.  A subclass
    sets ``_family`` and provides ``_parameters`` (scale, the table's numbers) and ``_torch_log_prob``."""

    def __init__(self):
        self._cast = {}

    def _parameters(self):
        raise NotImplementedError

    def _constants(self):
        scale, numbers = self._parameters()
        key = (float(scale),) + tuple(float(v) for v in numbers)
        if key[0] == 0.0 or (isinstance(self, Sinusoidal) and key[1] == 0.0):
            raise ValueError("%s: scale and period must not be 0" % type(self).__name__)
        return key, key[1:] or None, key[0]

    def log_prob(self, z):
        """log p(z) of z [B, 2]: one launch on the device (differentiable in z, once), the torch composition elsewhere."""
        if _kernel_inputs(z):
            return self._kernel_log_prob(z)
        return self._torch_log_prob(z)

    def score(self, z):
        """d log p / d z [B, 2] from the launch that evaluates log p; no autograd."""
        return self._kernel_score(z)


class TwoModes(_KernelPrior):
    """Distribution with two modes: ``loc`` the distance of the modes from the origin, ``scale`` their width
    (prior.py TwoModes).  TwoModes(2, 0.1) is the density of TwoMoons."""
    _family = _lib.TARGET_TWO_MODES

    def __init__(self, loc, scale):
        super().__init__()
        self.loc = loc
        self.scale = scale

    def _parameters(self):
        return self.scale, (self.loc,)

    def _torch_log_prob(self, z):
        a = torch.abs(z[:, 0])
        eps = abs(self.loc)
        return (-0.5 * ((torch.norm(z, dim=1) - self.loc) / (2 * self.scale)) ** 2
                - 0.5 * ((a - eps) / (3 * self.scale)) ** 2
                + torch.log1p(torch.exp(-2 * a * eps / (3 * self.scale) ** 2)))


class Sinusoidal(_KernelPrior):
    """Sinusoidal ridge z1 = sin(2 pi z0 / period) of width ``scale`` (prior.py Sinusoidal)."""
    _family = _lib.TARGET_SINUSOIDAL

    def __init__(self, scale, period):
        super().__init__()
        self.scale = scale
        self.period = period

    def _parameters(self):
        return self.scale, (self.period,)

    def _offset(self, z0):
        """The second ridge's offset w(z0), or None for the single ridge."""
        return None

    def _torch_log_prob(self, z):
        if z.dim() > 1:                     # the last axis first, as the reference moves it
            z_ = z.permute((z.dim() - 1,) + tuple(range(0, z.dim() - 1)))
        else:
            z_ = z
        d = z_[1] - torch.sin(2 * np.pi / self.period * z_[0])
        tail = 0.5 * (z_ ** 4).sum(0) / (20 * self.scale) ** 4
        w = self._offset(z_[0])
        if w is None:
            return -0.5 * (d / self.scale) ** 2 - tail
        return torch.logaddexp(-0.5 * (d / self.scale) ** 2, -0.5 * ((d + w) / self.scale) ** 2) - tail


class Sinusoidal_gap(Sinusoidal):
    """The sinusoidal ridge with a gap: a second ridge offset by w2_amp exp(-((z0 - w2_mu) / w2_scale)^2 / 2)
    (prior.py Sinusoidal_gap)."""
    _family = _lib.TARGET_SINUSOIDAL_GAP

    def __init__(self, scale, period):
        super().__init__(scale, period)
        self.w2_scale = 0.6
        self.w2_amp = 3.0
        self.w2_mu = 1.0

    def _parameters(self):
        return self.scale, (self.period, self.w2_amp, self.w2_mu, self.w2_scale)

    def _offset(self, z0):
        return self.w2_amp * torch.exp(-0.5 * ((z0 - self.w2_mu) / self.w2_scale) ** 2)


class Sinusoidal_split(Sinusoidal):
    """The sinusoidal ridge that splits in two: a second ridge offset by w3_amp sigmoid((z0 - w3_mu) / w3_scale)
    (prior.py Sinusoidal_split)."""
    _family = _lib.TARGET_SINUSOIDAL_SPLIT

    def __init__(self, scale, period):
        super().__init__(scale, period)
        self.w3_scale = 0.3
        self.w3_amp = 3.0
        self.w3_mu = 1.0

    def _parameters(self):
        return self.scale, (self.period, self.w3_amp, self.w3_mu, self.w3_scale)

    def _offset(self, z0):
        return self.w3_amp * torch.sigmoid((z0 - self.w3_mu) / self.w3_scale)


class Smiley(_KernelPrior):
    """A ring of radius 2 cut by the band |z1 + 0.8| = 1.2, of width ``scale`` (prior.py Smiley)."""
    _family = _lib.TARGET_SMILEY

    def __init__(self, scale):
        super().__init__()
        self.scale = scale

    def _parameters(self):
        return self.scale, ()

    def _torch_log_prob(self, z):
        return (-0.5 * ((torch.norm(z, dim=1) - 2) / (2 * self.scale)) ** 2
                - 0.5 * ((torch.abs(z[:, 1] + 0.8) - 1.2) / (2 * self.scale)) ** 2)
