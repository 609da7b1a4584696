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
"""
import torch

from . import _lib
from .autograd import HmcStackFn, MhWalkFn, needs_grad
from .distributions.mh_proposal import DiagGaussianProposal
from .distributions.target import CircularGaussianMixture, RingMixture, TwoMoons
from .flows.base import fold_log_det
from .flows.stochastic import HamiltonianMonteCarlo
from .stacks import add_log_det

MAX_POINTS = _lib.STOCH_MAX_POINTS          # n_layers (steps + 1) of one launch: the entry point's limit


def kernel_target(target):
    """One of the three targets of csrc/target_math.hpp; a subclass is not (what it overrides is unknown here)."""
    return type(target) in (TwoMoons, CircularGaussianMixture, RingMixture)


def _kernel_inputs(z):
    return torch.is_tensor(z) and z.is_cuda and z.dim() == 2 and z.shape[1] == 2 and z.dtype in (torch.float32, torch.float64)


def _steps(flow):
    """A step count one launch takes: beyond the entry point's limit the layer evaluates its torch composition."""
    return isinstance(flow.steps, int) and not isinstance(flow.steps, bool) and 0 <= flow.steps < MAX_POINTS


def covers(flow, z):
    """Whether the kernel evaluates the HMC layer ``flow`` on inputs like ``z``; otherwise the layer takes its torch
    composition."""
    return (type(flow) is HamiltonianMonteCarlo and kernel_target(flow.target) and _kernel_inputs(z) and _steps(flow)
            and all(p.dtype == z.dtype and p.device == z.device and p.numel() in (1, 2)
                    for p in (flow.log_step_size, flow.log_mass)))


def covers_walk(flow, z):
    """Whether the kernel evaluates the Metropolis-Hastings layer ``flow`` on inputs like ``z``."""
    prop = flow.proposal
    return (kernel_target(flow.dist) and _kernel_inputs(z) and _steps(flow) and type(prop) is DiagGaussianProposal
            and tuple(prop.shape) == (2,) and prop.scale.device == z.device and prop.scale.is_floating_point()
            and prop.scale.numel() in (1, 2))


def plan(order, start, z):
    """(end, flows): the longest run order[start:end] one launch evaluates, or None."""
    if not covers(order[start], z):
        return None
    first = order[start]
    most = MAX_POINTS // (first.steps + 1)           # >= 1: covers() holds steps + 1 to the limit
    end = start + 1
    while end < len(order) and end - start < most and covers(order[end], z) and order[end].target is first.target \
            and order[end].steps == first.steps:
        end += 1
    return end, order[start:end]


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


def run(flows, z, log_q, sign):
    """One launch for the run: (z', log_q + sign * log_det), or (z', sign * log_det) without a log_q.  With autograd
    recording the run is one node, HmcStackFn, and log_q is not written in place."""
    target = flows[0].target
    table, scale = target._operands(z)
    step, mass, sqrt_mass = operands(flows)
    noise, unif = draws(z, len(flows))
    if needs_grad(z, step, mass, sqrt_mass):
        out, ld = HmcStackFn.apply(z, step, mass, sqrt_mass, noise, unif, flows[0].steps, target._family, table, scale)
        return add_log_det(out, ld, log_q, sign)
    out, ld = _lib.hmc_stack(z, noise, unif, step, mass, sqrt_mass, flows[0].steps, target._family, table, scale)
    return fold_log_det(out, ld, log_q, sign)


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
