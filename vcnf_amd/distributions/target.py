"""Target distributions of the reverse-KL objectives: the three 2-D targets of normflow 1.2
(normflows/distributions/target.py) - TwoMoons, CircularGaussianMixture and RingMixture - with their base class.
Constructor arguments, attribute names and state_dict keys are the reference's.  Density and score d log p / d z come
from one launch of vcnf_target_log_prob_* (csrc/target_density.hip) in fp32 or fp64, picked by ``z``; under autograd
``log_prob`` is one node whose backward is a multiply by the score the forward launch wrote.  The targets have no
parameters.  The stochastic layers (vcnf_amd.flows.stochastic) evaluate the same device functions inside their own
kernels (csrc/target_math.hpp).  The energy densities of the reference's prior.py are in prior.py, on the same kernels.
The fork's other targets (NealsFunnel, ...) and n_dims != 2 are out of scope."""
import numpy as np
import torch
from torch import nn

from .. import _lib, autograd


class Target(nn.Module):
    """Sample target distributions to test models: a density on the proposal box prop_shift + prop_scale [0, 1]^n_dims
    that rejection sampling draws from.  A subclass sets ``n_dims`` and ``max_log_prob`` and provides ``log_prob``."""

    def __init__(self, prop_scale=torch.tensor(6.), prop_shift=torch.tensor(-3.)):
        super().__init__()
        self.register_buffer("prop_scale", prop_scale)
        self.register_buffer("prop_shift", prop_shift)

    def log_prob(self, z):
        raise NotImplementedError('The log probability is not implemented yet.')

    def _accept(self, eps, u):
        """(proposals z_, accept mask) for the uniform draws eps [N, n_dims] and u [N] of one rejection step."""
        z_ = self.prop_scale * eps + self.prop_shift
        return z_, torch.exp(self.log_prob(z_) - self.max_log_prob) > u

    def rejection_sampling(self, num_steps=1):
        """The accepted of ``num_steps`` proposals; draws eps [num_steps, n_dims], then u [num_steps], with torch.rand in
        the dtype and on the device of ``prop_scale``."""
        like = dict(dtype=self.prop_scale.dtype, device=self.prop_scale.device)
        eps = torch.rand((num_steps, self.n_dims), **like)
        u = torch.rand(num_steps, **like)
        z_, accept = self._accept(eps, u)
        return z_[accept, :]

    def sample(self, num_samples=1):
        """[num_samples, n_dims]: rejection steps of num_samples proposals each until enough are accepted."""
        z = torch.zeros((0, self.n_dims), dtype=self.prop_scale.dtype, device=self.prop_scale.device)
        while len(z) < num_samples:
            z_ = self.rejection_sampling(num_samples)
            z = torch.cat([z, z_[:num_samples - len(z), :]], 0)
        return z


class _KernelDensity:
    """What the densities of csrc/target_math.hpp share on the host - the targets here and the energy densities of
    prior.py: ``z`` checked, the constant table cast once per dtype and device, and the call of the kernel with or without
    autograd.  A class sets ``_family`` and provides ``_constants``; ``_cast`` is its dict."""
    _family = None

    def _constants(self):
        """(key, table or None, scale): the table (an fp64 tensor or a tuple of numbers) and the scale of the kernel's
        operands, and what they were computed from - a cast is served again while the key compares equal."""
        raise NotImplementedError

    def _operands(self, z):
        """(table or None, scale) in z's dtype on z's device."""
        _lib.require_device(z, f64=True, allow_grad=True)
        if z.dtype not in (torch.float32, torch.float64):
            raise _lib.VcnfError("%s.log_prob takes fp32 or fp64 inputs (got %s)" % (type(self).__name__, z.dtype))
        key, table, scale = self._constants()
        if table is None:
            return None, float(scale)
        slot = (z.dtype, z.device)
        if slot not in self._cast or self._cast[slot][0] != key:
            table = torch.as_tensor(table, dtype=torch.float64).to(device=z.device, dtype=z.dtype).contiguous()
            self._cast[slot] = (key, table, float(scale))
        return self._cast[slot][1:]

    def _kernel_log_prob(self, z):
        table, scale = self._operands(z)
        if autograd.needs_grad(z):
            return autograd.TargetLogProbFn.apply(z, table, self._family, scale)
        return _lib.target_log_prob(z, self._family, table, scale)[0]

    def _kernel_score(self, z):
        table, scale = self._operands(z)
        return _lib.target_log_prob(z, self._family, table, scale, want_score=True)[1]


class _KernelTarget(_KernelDensity, Target):
    """Shared end of the three targets.  A subclass sets ``_family`` and, for a mixture, the non-persistent fp64 buffer
    ``table`` and ``scale``; whatever replaces a buffer clears the casts."""

    def __init__(self):
        super().__init__()
        self._cast = {}
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._cast.clear())

    def _apply(self, fn, *args, **kwargs):
        self._cast = {}                     # .to() / .double() / .cuda() replace the buffers the casts came from
        return super()._apply(fn, *args, **kwargs)

    def _constants(self):
        table = getattr(self, "table", None)
        return None, table, 0.0 if table is None else self.scale

    def log_prob(self, z):
        """log p(z) [B] of z [B, 2] on the device; differentiable in z (once)."""
        return self._kernel_log_prob(z)

    def score(self, z):
        """d log p / d z [B, 2] from the launch that evaluates log p; no autograd."""
        return self._kernel_score(z)


class TwoMoons(_KernelTarget):
    """Bimodal two-dimensional distribution (target.py TwoMoons):
    log p = -((|z| - 2) / 0.2)^2 / 2 - ((|z0| - 2) / 0.3)^2 / 2 + log(1 + exp(-4 |z0| / 0.09))."""
    _family = _lib.TARGET_TWO_MOONS

    def __init__(self):
        super().__init__()
        self.n_dims = 2
        self.max_log_prob = 0.


class CircularGaussianMixture(_KernelTarget):
    """Two-dimensional Gaussian mixture with ``n_modes`` modes of standard deviation ``scale`` = 2/3 sin(pi / n_modes) on a
    circle of radius 2 (target.py CircularGaussianMixture).  ``scale`` is a buffer as in the reference (fp64, as the
    reference's expression creates it); the centres, computed in fp64 on the host, are the non-persistent buffer
    ``table`` [n_modes, 2].  Draws have the dtype of ``prop_scale``."""
    _family = _lib.TARGET_CIRCULAR_GMM

    def __init__(self, n_modes=8):
        super().__init__()
        self.n_modes = n_modes
        self.n_dims = 2
        self.register_buffer("scale", torch.tensor(2 / 3 * np.sin(np.pi / self.n_modes)))
        phi = 2 * np.pi / self.n_modes * np.arange(self.n_modes)
        self.register_buffer("table", torch.from_numpy(np.stack((2 * np.sin(phi), 2 * np.cos(phi)), 1)), persistent=False)

    def sample(self, num_samples=1):
        """eps ~ N(0, 1) [num_samples, 2], then the mode indices with torch.randint: z = eps scale + centre[index]."""
        like = dict(dtype=self.prop_scale.dtype, device=self.prop_scale.device)
        eps = torch.randn((num_samples, self.n_dims), **like)
        index = torch.randint(0, self.n_modes, (num_samples,), device=like["device"])
        return eps * self.scale.to(**like) + self.table.to(**like)[index]


class RingMixture(_KernelTarget):
    """Mixture of ``n_rings`` ring distributions of radii 2 (i + 1) / n_rings and width ``scale`` = 1 / 4 / n_rings in two
    dimensions (target.py RingMixture); the radii, in fp64, are the non-persistent buffer ``table`` [n_rings]."""
    _family = _lib.TARGET_RING_MIXTURE

    def __init__(self, n_rings=2):
        super().__init__()
        self.n_dims = 2
        self.max_log_prob = 0.
        self.n_rings = n_rings
        self.scale = 1 / 4 / self.n_rings
        self.register_buffer("table", torch.from_numpy(2 / self.n_rings * (np.arange(self.n_rings) + 1.0)), persistent=False)
