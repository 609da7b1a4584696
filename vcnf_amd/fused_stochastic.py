"""Host side of csrc/stochastic.hip: runs of consecutive ``HamiltonianMonteCarlo`` layers in ONE launch, and the walk of
a ``MetropolisHastings`` layer.

``plan`` finds the longest stretch of HMC layers that share the target object and the step count and whose parameters
have the inputs' dtype and device (one layer is enough for a run; the layers are their own inverses, so a density pass
forms the same runs in its own order).  ``operands`` turns the run's parameters into the kernel's operands - exp of the
log step sizes and masses, one row [2] per layer - with three batched torch ops on ``torch.stack`` of the parameters,
differentiable, so autograd carries the kernel's operand gradients on to the parameters.  ``draws`` takes the run's
random numbers from torch's generator in the reference's order, layer by layer into preallocated buffers: ``randn`` of
the layer's [B, 2], then ``rand`` of its [B]; a seed gives the chain that the layers give one by one, on the kernel or
in torch.

Annealed layers - the layers of ``vcnf_amd.sampling.HAIS``, whose target is the ``LinearInterpolation`` of a kernel target
and a ``DiagGaussian`` prior over (2,) with a weight ``alpha`` - form runs of their own: consecutive layers that share the
target object, the prior object and the step count go to vcnf_hmc_annealed_stack_*, with their alphas as the operand
``beta`` [K] (``betas``) and the prior's parameters as constants.  A run never mixes plain and annealed layers.  The kernel
has no gradient for the prior, so while autograd records, a prior whose parameters require grad sends the layer to its
torch composition.  ``launch`` can also return the target's log p at the run's output, which the kernel carries anyway:
the last term of the sampler's log weights.
"""
import numbers

import torch

from . import _lib
from .autograd import HmcAnnealedStackFn, HmcStackFn, MhWalkFn, needs_grad
from .distributions.base import DiagGaussian
from .distributions.linear_interpolation import LinearInterpolation
from .distributions.mh_proposal import DiagGaussianProposal
from .distributions.prior import Sinusoidal, Sinusoidal_gap, Sinusoidal_split, Smiley, TwoModes
from .distributions.target import CircularGaussianMixture, RingMixture, TwoMoons
from .flows.base import fold_log_det
from .flows.stochastic import HamiltonianMonteCarlo
from .stacks import add_log_det

MAX_POINTS = _lib.STOCH_MAX_POINTS          # n_layers (steps + 1) of one launch: the entry point's limit


def kernel_target(target):
    """One of the densities of csrc/target_math.hpp - the three targets of distributions/target.py or the five energies
    of distributions/prior.py; a subclass is not (what it overrides is unknown here)."""
    return type(target) in (TwoMoons, CircularGaussianMixture, RingMixture,
                            TwoModes, Sinusoidal, Sinusoidal_gap, Sinusoidal_split, Smiley)


def annealed(target):
    """Whether ``target`` is the bridge of an annealed layer: exactly a LinearInterpolation."""
    return type(target) is LinearInterpolation


def _kernel_bridge(bridge, z):
    """Whether the kernel evaluates the LinearInterpolation ``bridge`` on the kernel inputs ``z``: a kernel target against
    exactly a DiagGaussian over (2,) without a temperature whose parameters are like z - and are constants while autograd
    records, since the kernel has no gradient for them - with a weight that is a number or a one-element tensor that
    does not require grad."""
    prior, alpha = bridge.dist2, bridge.alpha
    if not (kernel_target(bridge.dist1) and type(prior) is DiagGaussian and tuple(prior.shape) == (2,) and prior.temperature is None):
        return False
    if torch.is_tensor(alpha):
        if alpha.numel() != 1 or alpha.requires_grad or not alpha.is_floating_point():
            return False
    elif isinstance(alpha, bool) or not isinstance(alpha, numbers.Real):
        return False
    recording = torch.is_grad_enabled()
    return all(p.dtype == z.dtype and p.device == z.device and not (recording and p.requires_grad)
               for p in (prior.loc, prior.log_scale))


def _kernel_inputs(z):
    return torch.is_tensor(z) and z.is_cuda and z.dim() == 2 and z.shape[1] == 2 and z.dtype in (torch.float32, torch.float64)


def _steps(flow):
    """A step count one launch takes: beyond the entry point's limit the layer evaluates its torch composition."""
    return isinstance(flow.steps, int) and not isinstance(flow.steps, bool) and 0 <= flow.steps < MAX_POINTS


def covers(flow, z):
    """Whether the kernel evaluates the HMC layer ``flow`` on inputs like ``z``; otherwise the layer takes its torch
    composition."""
    if not (type(flow) is HamiltonianMonteCarlo and _kernel_inputs(z) and _steps(flow)):
        return False
    target = flow.target
    return ((_kernel_bridge(target, z) if annealed(target) else kernel_target(target))
            and all(p.dtype == z.dtype and p.device == z.device and p.numel() in (1, 2)
                    for p in (flow.log_step_size, flow.log_mass)))


def covers_walk(flow, z):
    """Whether the kernel evaluates the Metropolis-Hastings layer ``flow`` on inputs like ``z``."""
    prop = flow.proposal
    return (kernel_target(flow.dist) and _kernel_inputs(z) and _steps(flow) and type(prop) is DiagGaussianProposal
            and tuple(prop.shape) == (2,) and prop.scale.device == z.device and prop.scale.is_floating_point()
            and prop.scale.numel() in (1, 2))


def plan(order, start, z):
    """(end, flows): the longest run order[start:end] one launch evaluates, or None.  The layers of a run share the step
    count and the target object - annealed layers the two objects their bridges join - so a run is plain or annealed."""
    if not covers(order[start], z):
        return None
    first = order[start]
    most = MAX_POINTS // (first.steps + 1)           # >= 1: covers() holds steps + 1 to the limit
    end = start + 1
    while end < len(order) and end - start < most and covers(order[end], z) and _same_target(order[end].target, first.target) \
            and order[end].steps == first.steps:
        end += 1
    return end, order[start:end]


def _same_target(a, b):
    if annealed(a) or annealed(b):
        return annealed(a) and annealed(b) and a.dist1 is b.dist1 and a.dist2 is b.dist2
    return a is b


def stack_run(owner, order, start, z, context, density):
    """NormalizingFlow's planner for this family (the contract: vcnf_amd.stacks); the same in both pass
    directions."""
    p = plan(order, start, z)
    if p is None:
        return None
    end, flows = p
    return end, lambda z, log_q, sign: run(flows, z, log_q, sign)


stack_run.differentiable = True       # NormalizingFlow's plain walk (the one autograd records) takes these runs too


def operands(flows):
    """(step [K, 2], mass [K, 2], sqrt_mass [K, 2]) of a run, as include/vcnf_hip.h describes them."""
    log_step = torch.stack([f.log_step_size.reshape(-1).expand(2) for f in flows])
    log_mass = torch.stack([f.log_mass.reshape(-1).expand(2) for f in flows])
    return torch.exp(log_step), torch.exp(log_mass), torch.exp(0.5 * log_mass)


def draws(z, n_layers):
    """(noise [K, B, 2], unif [K, B]) in the order the layers draw them one by one."""
    noise = torch.empty((n_layers,) + tuple(z.shape), dtype=z.dtype, device=z.device)
    unif = torch.empty((n_layers, len(z)), dtype=z.dtype, device=z.device)
    for k in range(n_layers):
        noise[k].normal_()
        unif[k].uniform_()
    return noise, unif


def betas(flows, z):
    """beta [K] of an annealed run: the layers' alphas in z's dtype on z's device.  Alphas that are tensors on that
    device are stacked there, without a host synchronisation; numbers and host tensors make one host tensor."""
    alphas = [f.target.alpha for f in flows]
    if all(torch.is_tensor(a) and a.device == z.device for a in alphas):
        return torch.stack([a.detach().reshape(()) for a in alphas]).to(z.dtype)
    return torch.tensor([float(a) for a in alphas], dtype=torch.float64).to(device=z.device, dtype=z.dtype)


def launch(flows, z, want_logp=False):
    """One launch for the run: (z', log_det, recorded) and with ``want_logp`` - an annealed run outside autograd - also the
    target's log p at z'.  ``recorded``: the run is one autograd node (HmcStackFn, HmcAnnealedStackFn)."""
    target = flows[0].target
    bridge = annealed(target)
    kernel = target.dist1 if bridge else target
    table, scale = kernel._operands(z)
    step, mass, sqrt_mass = operands(flows)
    noise, unif = draws(z, len(flows))
    steps, family = flows[0].steps, kernel._family
    recorded = needs_grad(z, step, mass, sqrt_mass)
    if not bridge:
        if recorded:
            return HmcStackFn.apply(z, step, mass, sqrt_mass, noise, unif, steps, family, table, scale) + (True,)
        return _lib.hmc_stack(z, noise, unif, step, mass, sqrt_mass, steps, family, table, scale) + (False,)
    prior = (betas(flows, z), target.dist2.loc.detach().reshape(-1), target.dist2.log_scale.detach().reshape(-1))
    if recorded:
        return HmcAnnealedStackFn.apply(z, step, mass, sqrt_mass, noise, unif, *prior, steps, family, table, scale) + (True,)
    got = _lib.hmc_annealed_stack(z, noise, unif, step, mass, sqrt_mass, *prior, steps, family, table, scale, want_logp=want_logp)
    return got[:2] + (False,) + got[2:]


def run(flows, z, log_q, sign):
    """One launch for the run: (z', log_q + sign * log_det), or (z', sign * log_det) without a log_q.  With autograd
    recording the run is one node and log_q is not written in place."""
    out, ld, recorded = launch(flows, z)
    return add_log_det(out, ld, log_q, sign) if recorded else fold_log_det(out, ld, log_q, sign)


def walk(flow, z):
    """One launch for the layer's ``steps`` random-walk steps: (z', zeros [B])."""
    table, scale = flow.dist._operands(z)
    eps = torch.empty((flow.steps,) + tuple(z.shape), dtype=z.dtype, device=z.device)
    w = torch.empty((flow.steps, len(z)), dtype=z.dtype, device=z.device)
    for i in range(flow.steps):
        eps[i].normal_()
        w[i].uniform_()
    prop = flow.proposal.scale.detach().to(z.dtype).reshape(-1).expand(2).contiguous()
    if needs_grad(z):
        out = MhWalkFn.apply(z, eps, w, prop, flow.dist._family, table, scale)
    else:
        out = _lib.mh_walk(z, eps, w, prop, flow.dist._family, table, scale)
    return out, torch.zeros(len(z), dtype=z.dtype, device=z.device)
